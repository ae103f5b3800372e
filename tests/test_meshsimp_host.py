"""Mesh welding and decimation without a GPU: the header-derived exports, the workspace size, every Python refusal, the replay's
own 3 x 3 solve against numpy.linalg.solve, and the clustering part of csrc/meshops_math.h on the host -
tests/meshsimp_host_main.cpp, a stand-alone program that clusters, collapses and places a mesh with the header's functions over
exact-size heap buffers, is built with g++ under AddressSanitizer and UBSan (without them when the sanitizer runtime cannot be
linked, as tests/test_meshops_host.py does) and must equal the numpy replay of tests/meshsimp_ref.py bit for bit in all three
placements: the device kernels call the same functions."""
import os
import subprocess

import numpy as np
import pytest

import mc_numpy as M
import meshops_ref as R
import meshsimp_ref as S

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "sw-nerf_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
NAMES = ["swnerf_mesh_simplify_workspace_bytes", "swnerf_mesh_cluster", "swnerf_mesh_collapse", "swnerf_mesh_collapse_emit"]
PLACE = {"weld": 0, "mean": 1, "quadric": 2}


spacing = S.spacing


def test_exports_come_from_the_header():
    from swnerf import _lib, mesh
    for n in NAMES:
        assert n in _lib.EXPORTS, n
    L = _lib.lib()
    assert all(hasattr(L, n) for n in NAMES)
    assert _lib.DEFINES["VERSION"] == 112
    assert (_lib.DEFINES["MESH_WELD"], _lib.DEFINES["MESH_MEAN"], _lib.DEFINES["MESH_QUADRIC"]) == (0, 1, 2)
    for n in ("cluster", "weld", "decimate", "decimation_cell"):
        assert callable(getattr(mesh, n))


def test_workspace_bytes():
    from swnerf import _lib
    ws = _lib.lib().swnerf_mesh_simplify_workspace_bytes
    old = _lib.lib().swnerf_mesh_workspace_bytes
    assert old(360, 716) == 3 * 1536 + 3072 + 256 + 512 + 10240      # the existing size function keeps its values
    for V, F in ((-1, 0), (0, -1), (2 ** 31, 1), (1, (2 ** 31 + 2) // 3), (2 ** 40, 2 ** 40)):
        assert ws(V, F) == 0, (V, F)
    sizes = [0, 1, 3, 31, 32, 33, 255, 256, 257, 360, 716, 100000, 2 ** 24, 2 ** 31 - 1]
    for V in sizes:
        prev = 0
        for F in [s for s in sizes if 3 * s < 2 ** 31]:
            b = ws(V, F)
            assert b > 0 and b % 256 == 0 and b >= prev, (V, F)
            prev = b
        assert ws(V, 0) >= 12 * 2 * V                                # a table of at least 2 V slots of 8 + 4 bytes
    for F in (0, 716):
        col = [ws(V, F) for V in sizes]
        assert col == sorted(col)


def test_python_refusals_need_no_gpu():
    from swnerf import mesh
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    f = np.array([[0, 1, 2], [1, 2, 3]], np.int32)
    m = mesh.Mesh(v, f, np.zeros_like(v))
    for bad in (0., -1., float("nan"), float("inf"), 1e-60, "x"):
        with pytest.raises(ValueError, match="finite positive"):
            mesh.cluster(v, bad)
        with pytest.raises(ValueError, match="finite positive"):
            mesh.decimate(m, cell=bad)
        with pytest.raises(ValueError, match="finite positive"):
            mesh.weld(m, tolerance=bad)
        with pytest.raises(ValueError, match="finite positive"):
            mesh.clean(m, weld=bad)
        with pytest.raises(ValueError, match="finite positive"):
            mesh.clean(m, decimate={"cell": bad})
    for call in (lambda c: mesh.cluster(v, c), lambda c: mesh.decimate(m, cell=c), lambda c: mesh.weld(m, tolerance=c),
                 lambda c: mesh.weld(v, c, faces=f), lambda c: mesh.decimate((v, f), cell=c)):
        with pytest.raises(ValueError, match="21 bits"):
            call(2.0 ** -21)                                         # extent 1: 2^21 cells an axis
    with pytest.raises(ValueError, match="exactly one"):
        mesh.decimate(m)
    with pytest.raises(ValueError, match="exactly one"):
        mesh.decimate(m, cell=0.5, target_faces=2)
    with pytest.raises(ValueError, match="exactly one"):
        mesh.clean(m, decimate={})
    with pytest.raises(ValueError, match="placement"):
        mesh.decimate(m, cell=0.5, placement="median")
    with pytest.raises(ValueError, match="placement"):
        mesh.clean(m, decimate={"cell": 0.5, "placement": "median"})
    for n in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="target_faces"):
            mesh.decimate(m, target_faces=n)
        with pytest.raises(ValueError, match="target_faces"):
            mesh.decimation_cell(m, n)
    with pytest.raises(ValueError, match="eps"):
        mesh.decimate(m, cell=0.5, eps=float("nan"))
    with pytest.raises(TypeError, match="decimate"):
        mesh.clean(m, decimate={"cells": 0.5})
    with pytest.raises(TypeError, match="decimate"):
        mesh.generate_mesh(None, None, None, clean={"decimate": 3})
    with pytest.raises(ValueError, match="finite positive"):
        mesh.generate_mesh(None, None, None, clean={"weld": -1.})
    with pytest.raises(TypeError, match="unknown clean option"):
        mesh.generate_mesh(None, None, None, clean={"welded": True})


def test_the_replay_shows_the_purpose():
    """sphere(32) at 2.5 spacings: the quadric representative keeps the volume the cluster mean loses (the replay alone, no GPU)"""
    field, h = M.sphere(32)
    v, f, _ = R.mc(field, 0., h)
    assert (len(v), len(f)) == (1608, 3212)
    vol = R.measure(v, f)["volume"]
    out = {p: S.simplify(v, f, h=2.5 * h, placement=p) for p in ("quadric", "mean")}
    err = {}
    for p, o in out.items():
        m = R.measure(o["verts"], o["faces"])
        assert m["closed"] and m["euler"] == 2, p
        err[p] = abs(m["volume"] - vol) / vol
    print(f"sphere(32) at 2.5 spacings: {len(v)} / {len(f)} -> {out['quadric']['V_out']} / {out['quadric']['F_out']}; volume off by "
          f"{100 * err['quadric']:.2f} % (quadric), {100 * err['mean']:.2f} % (mean)")
    assert out["quadric"]["F_out"] < len(f) // 4
    assert err["quadric"] < err["mean"] and err["quadric"] < 0.02


@pytest.mark.parametrize("name", ["sphere", "noise"])
@pytest.mark.parametrize("cells", [1.5, 2.5])
def test_the_replays_solve_agrees_with_linalg(name, cells):
    """y = adj(R) r / det(R) against numpy.linalg.solve on the same R and r for every cluster with tr > 0.  cond(R) <= (1 + 3 eps) /
    eps ~ 1003, so the fp64 error is about 1e-13 of |y| <= sqrt(3) h; the gate is 1e-10 h."""
    v, f, _ = R.fixtures()[name]
    h = cells * spacing(name)
    eps = 1e-3
    c = S.cluster(v, h)
    labels = np.unique(c["vlabel"])
    A, b = S.quadric_system(v, f, c["vlabel"])
    A, b, m = A[labels], b[labels], S.member_mean(v, c["vlabel"])[labels]
    y, det, tr, lam = S.quadric_solve(A, b, m, eps)
    on = tr > 0
    assert on.sum() > 10
    Rm = np.stack([np.stack([A[:, 0] + lam, A[:, 1], A[:, 2]], 1), np.stack([A[:, 1], A[:, 3] + lam, A[:, 4]], 1),
                   np.stack([A[:, 2], A[:, 4], A[:, 5] + lam], 1)], 1)
    rhs = -(np.einsum("nij,nj->ni", np.stack([np.stack([A[:, 0], A[:, 1], A[:, 2]], 1), np.stack([A[:, 1], A[:, 3], A[:, 4]], 1),
                                              np.stack([A[:, 2], A[:, 4], A[:, 5]], 1)], 1), m) + b)
    assert (det[on] > 0).all() and float(np.linalg.cond(Rm[on]).max()) <= 1.001 * (1 + 3 * eps) / eps
    want = np.linalg.solve(Rm[on], rhs[on][..., None])[..., 0]
    err = float(np.abs(y[on] - want).max())
    print(f"{name} at {cells} spacings: {int(on.sum())} clusters, max |y - solve| = {err:.3e}, gate = {1e-10 * h:.3e}")
    assert err <= 1e-10 * h


# --------------------------------------------------------------------------------------------- the header's clustering on the host
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("meshsimp_host") / "meshsimp_host_main")
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "meshsimp_host_main.cpp"), "-o", exe]
    r = subprocess.run(base + SAN, capture_output=True, text=True)
    if r.returncode != 0:
        assert "sanitize" in r.stderr or "asan" in r.stderr or "ubsan" in r.stderr, r.stderr      # only a failed sanitizer link falls back
        subprocess.run(base, check=True)
    return exe


def run_program(program, tmp_path, v, f, col, h, eps, placement, origin=None):
    V, F = len(v), len(f)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([V, F, col is not None, origin is not None], np.int32).tobytes() + np.ascontiguousarray(v, np.float32).tobytes() +
                 np.ascontiguousarray(f, np.int32).tobytes() + (b"" if col is None else np.ascontiguousarray(col, np.float32).tobytes()) +
                 (b"" if origin is None else np.asarray(origin, np.float32).tobytes()))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), repr(float(np.float32(h))), repr(float(eps)),
                        str(PLACE[placement])], capture_output=True, text=True, timeout=120, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, r.stderr[-3000:]
    raw = open(tmp_path / "out.bin", "rb").read()
    counts = np.frombuffer(raw, np.int32, 6, 0)
    if counts[1]:
        assert len(raw) == 24
        return dict(counts=counts)
    Vo, Fo = int(counts[2]), int(counts[3])
    at = 24
    out = dict(counts=counts, origin=np.frombuffer(raw, np.float32, 3, at))
    at += 12
    out["vlabel"] = np.frombuffer(raw, np.int32, V, at)
    at += 4 * V
    out["verts"] = np.frombuffer(raw, np.float32, 3 * Vo, at).reshape(Vo, 3)
    at += 12 * Vo
    out["faces"] = np.frombuffer(raw, np.int32, 3 * Fo, at).reshape(Fo, 3)
    at += 12 * Fo
    if col is not None:
        out["colors"] = np.frombuffer(raw, np.float32, 3 * Vo, at).reshape(Vo, 3)
        at += 12 * Vo
    assert at == len(raw)
    return out


@pytest.mark.parametrize("name", ["sphere", "noise", "open_sphere", "fan", "duplicated_face", "unreferenced", "repeated_index", "triangle", "empty",
                                  "floaters"])
@pytest.mark.parametrize("placement", ["weld", "mean", "quadric"])
@pytest.mark.parametrize("cells", [1.5, 2.5])
def test_header_functions_equal_the_replay_bit_for_bit(program, tmp_path, name, placement, cells):
    v, f, _ = R.fixtures()[name]
    col = np.random.default_rng(len(v)).random(v.shape).astype(np.float32)
    h = np.float32(cells * spacing(name))
    got = run_program(program, tmp_path, v, f, col, h, 1e-3, placement)
    w = S.simplify(v, f, None, col, h, placement, 1e-3)
    assert got["counts"].tolist() == [w["clusters"], 0, w["V_out"], w["F_out"], w["degenerate"], w["duplicate"]]
    assert got["origin"].tobytes() == w["origin"].tobytes() and np.array_equal(got["vlabel"], w["vlabel"])
    assert np.array_equal(got["faces"], w["faces"])
    assert got["verts"].tobytes() == w["verts"].tobytes() and got["colors"].tobytes() == w["colors"].tobytes()
    if name == "sphere" and placement == "quadric":
        moved = (w["verts"] != S.simplify(v, f, None, col, h, "mean")["verts"]).any(1).mean()
        assert moved > 0.9                                           # the quadric branch is the one taken, not the fall-back


def test_header_edge_cells_and_invalid_vertices(program, tmp_path):
    v, f, _ = R.fixtures()["sphere"]
    ext = float((v.max(0) - v.min(0)).max())
    one = run_program(program, tmp_path, v, f, None, 2 * ext, 1e-3, "quadric")
    assert one["counts"].tolist() == [1, 0, 0, 0, 716, 0] and (one["vlabel"] == 0).all()
    each = run_program(program, tmp_path, v, f, None, np.float32(ext * 2.0 ** -20), 1e-3, "weld")
    assert each["counts"].tolist() == [360, 0, 360, 716, 0, 0] and each["verts"].tobytes() == v.tobytes() and np.array_equal(each["faces"], f)
    bad = v.copy()
    bad[17, 1] = np.nan
    bad[200, 0] = np.inf
    got = run_program(program, tmp_path, bad, f, None, 0.2, 1e-3, "mean")
    assert got["counts"].tolist() == [0, 2, 0, 0, 0, 0] and S.simplify(bad, f, h=0.2) == dict(invalid=2)
    below = run_program(program, tmp_path, v, f, None, 0.2, 1e-3, "mean", origin=(0., -1., -1.))
    assert below["counts"][1] == int((v[:, 0] < 0).sum()) == S.cluster(v, 0.2, (0., -1., -1.))["invalid"]
    shifted = run_program(program, tmp_path, v, f, None, 0.2, 1e-3, "quadric", origin=(-1.03, -1.01, -1.07))
    w = S.simplify(v, f, h=0.2, placement="quadric", origin=(-1.03, -1.01, -1.07))
    assert shifted["verts"].tobytes() == w["verts"].tobytes() and np.array_equal(shifted["faces"], w["faces"])
