"""Mesh hole filling without a GPU: the header-derived exports, the workspace size, every Python refusal, the numpy replay of
tests/meshfill_ref.py checked against independent code (meshops_ref.measure: closedness, Euler characteristic, volume), and the
hole-filling part of csrc/meshops_math.h on the host - tests/meshfill_host_main.cpp, a stand-alone program that finds the boundary,
traces the loops and caps them with the header's functions over exact-size heap buffers, is built with g++ under AddressSanitizer
and UBSan (without them when the sanitizer runtime cannot be linked, as tests/test_meshops_host.py does) and must equal the replay
bit for bit: the device kernels call the same functions."""
import os
import subprocess

import numpy as np
import pytest

import meshops_ref as R
import meshfill_ref as H

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "sw-nerf_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
NAMES = ["swnerf_mesh_fill_workspace_bytes", "swnerf_mesh_boundary", "swnerf_mesh_boundary_loops", "swnerf_mesh_fill_emit"]
KEYS = ["boundary_edges", "loops", "filled_loops", "filled_edges", "skipped_loops", "unfillable_edges", "new_vertices", "new_faces"]


def meshes():
    """name -> (verts, faces): the fixtures of meshops_ref plus the cut and pinched meshes of meshfill_ref"""
    out = {k: (v, f) for k, (v, f, _) in R.fixtures().items()}
    out["cut_sphere"] = H.cut_sphere()[:2]
    out["corner_sphere"] = H.corner_sphere()[:2]
    out["cut_torus"] = H.cut_torus()[:2]
    out["open_noise"] = H.open_noise()[:2]
    out["pinched"] = H.pinched()
    out["bow_tie"] = (np.arange(15, dtype=np.float32).reshape(5, 3) ** 2 % 7, np.array([[0, 1, 2], [0, 3, 4]], np.int32))
    out["three_on_an_edge"] = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, -1, 0]], np.float32),
                               np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]], np.int32))
    return out


MESHES = meshes()


def test_exports_come_from_the_header():
    from swnerf import _lib, mesh
    for n in NAMES:
        assert n in _lib.EXPORTS, n
    L = _lib.lib()
    assert all(hasattr(L, n) for n in NAMES)
    assert _lib.DEFINES["VERSION"] == 112
    for n in ("boundary_loops", "fill_holes", "fill_holes_arrays"):
        assert callable(getattr(mesh, n))


def test_workspace_bytes():
    from swnerf import _lib
    ws = _lib.lib().swnerf_mesh_fill_workspace_bytes
    assert _lib.lib().swnerf_mesh_workspace_bytes(360, 716) == 3 * 1536 + 3072 + 256 + 512 + 10240       # the two older size functions
    assert _lib.lib().swnerf_mesh_simplify_workspace_bytes(360, 716) == 12 * 1024 + 5 * 1536 + 2 * 8704 + 3072 + 256 + 512     # keep their values
    for V, F in ((-1, 0), (0, -1), (2 ** 31, 1), (1, (2 ** 31 + 2) // 3), (2 ** 40, 2 ** 40)):
        assert ws(V, F) == 0, (V, F)
    sizes = [0, 1, 3, 31, 32, 33, 255, 256, 257, 360, 716, 100000, 2 ** 24, 2 ** 31 - 1]
    for V in sizes:
        prev = 0
        for F in [s for s in sizes if 3 * s < 2 ** 31]:
            b = ws(V, F)
            assert b > 0 and b % 256 == 0 and b >= prev, (V, F)
            prev = b
            assert b >= 2 * 8 * 3 * F + 3 * 4 * 3 * F                # two (target, value) buffers and three int32 arrays over the half-edges
    for F in (0, 716):
        col = [ws(V, F) for V in sizes]
        assert col == sorted(col)


def test_python_refusals_need_no_gpu():
    from swnerf import mesh
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    f = np.array([[0, 1, 2], [1, 2, 3]], np.int32)
    m = mesh.Mesh(v, f, np.zeros_like(v))
    for bad in (0, 2, -1, 2.5, True, False, "x", 2 ** 31, float("nan")):
        with pytest.raises(ValueError, match="max_edges"):
            mesh.fill_holes(m, max_edges=bad)
        with pytest.raises(ValueError, match="max_edges"):
            mesh.fill_holes(v, bad, faces=f)
        with pytest.raises(ValueError, match="max_edges"):
            mesh.fill_holes_arrays(v, f, max_edges=bad)
    for bad in (0, 2, -1, 2.5, "x", 2 ** 31):
        with pytest.raises(ValueError, match="fill_holes"):
            mesh.clean(m, fill_holes=bad)
        with pytest.raises(ValueError, match="fill_holes"):
            mesh.generate_mesh(None, None, None, clean={"fill_holes": bad})
    with pytest.raises(TypeError, match="unknown clean option"):
        mesh.generate_mesh(None, None, None, clean={"fill_hole": True})
    with pytest.raises(ValueError, match="n_vertices"):
        mesh.boundary_loops(f, -1)
    from swnerf import meshops
    assert meshops.clean_options({"fill_holes": True}) == {"fill_holes": True} and meshops.clean_options({"fill_holes": 7}) == {"fill_holes": 7}
    assert meshops.clean_options({"fill_holes": None}) == {"fill_holes": None}


# ----------------------------------------------------------------------------------------- the replay against independent code
@pytest.mark.parametrize("name", ["open_sphere", "fan", "cut_sphere", "corner_sphere", "cut_torus", "triangle"])
def test_the_replay_closes_the_surface(name):
    v, f = MESHES[name]
    before = R.measure(v, f)
    o = H.fill(v, f)
    m = R.measure(o["verts"], o["faces"])
    info = o["info"]
    print(name, len(v), len(f), "->", len(o["verts"]), len(o["faces"]), info)
    assert before["boundary_edges"] > 0 and not before["closed"]
    assert m["closed"] and m["boundary_edges"] == 0 and m["nonmanifold_edges"] == 0 and m["euler"] == 2
    assert m["n_components"] == before["n_components"]
    assert info["boundary_edges"] == before["boundary_edges"] == info["filled_edges"]
    assert o["verts"][:len(v)].tobytes() == v.tobytes() and np.array_equal(o["faces"][:len(f)], f)


@pytest.mark.parametrize("name", sorted(MESHES))
@pytest.mark.parametrize("max_edges", [None, 4, 30])
def test_the_replays_counts_add_up(name, max_edges):
    v, f = MESHES[name]
    o = H.fill(v, f, max_edges=max_edges)
    info, n = o["info"], o["table"][:, 1]
    skipped = n[n > max_edges] if max_edges is not None else n[:0]
    assert info["boundary_edges"] + H.self_edges(f, len(v)) == R.measure(v, f)["boundary_edges"]
    assert H.self_edges(f, len(v)) == (1 if name == "repeated_index" else 0)       # measure() also counts the edge 0 -> 0 of that fixture
    assert info["filled_edges"] + info["unfillable_edges"] + int(skipped.sum()) == info["boundary_edges"]
    assert info["skipped_loops"] == len(skipped) and info["loops"] == len(n) and (n >= 3).all()
    assert (len(o["verts"]), len(o["faces"])) == (len(v) + info["new_vertices"], len(f) + info["new_faces"])
    assert R.measure(o["verts"], o["faces"])["n_components"] == R.measure(v, f)["n_components"]
    assert R.measure(o["verts"], o["faces"])["boundary_edges"] == info["boundary_edges"] - info["filled_edges"] + H.self_edges(f, len(v))
    lead = o["table"][:, 0]
    assert (np.diff(lead) > 0).all()                                 # ascending leaders; each is the smallest half-edge id of its loop
    tail = np.asarray(f, np.int64).reshape(-1)
    for i in range(len(n)):
        p = o["loop_vertices"][o["loop_offsets"][i]:o["loop_offsets"][i + 1]]
        assert p[0] == tail[lead[i]] and len(set(p.tolist())) == len(p)


def test_the_issues_counts():
    want = {"open_sphere": (52, [52], 0), "fan": (300, [300], 0), "triangle": (3, [3], 0), "duplicated_face": (0, [], 0), "sphere": (0, [], 0),
            "cut_torus": (80, [56, 24], 0), "pinched": (74, [52], 22), "bow_tie": (6, [], 6), "three_on_an_edge": (6, [], 6)}
    for name, (nb, lens, unf) in want.items():
        o = H.fill(*MESHES[name])
        assert (o["info"]["boundary_edges"], o["table"][:, 1].tolist(), o["info"]["unfillable_edges"]) == (nb, lens, unf), name
    o = H.fill(*MESHES["open_sphere"])
    assert (len(o["verts"]), len(o["faces"])) == (361, 410)
    o = H.fill(*MESHES["triangle"])
    assert (len(o["verts"]), len(o["faces"])) == (3, 2) and R.measure(o["verts"], o["faces"])["volume"] == 0
    assert R.measure(*MESHES["three_on_an_edge"])["nonmanifold_edges"] == 1
    n = H.fill(*MESHES["open_noise"])["table"][:, 1]
    assert len(n) == 13 and int((n == 4).sum()) == 6
    i4, i3 = H.fill(*MESHES["open_noise"], max_edges=4)["info"], H.fill(*MESHES["open_noise"], max_edges=3)["info"]
    assert (i4["filled_loops"], i4["skipped_loops"], i4["new_faces"]) == (6, 7, 24) and (i3["filled_loops"], i3["new_faces"]) == (0, 0)


def test_the_blocked_mean_is_the_mean():
    """the fixed shape of additions is within fp64 rounding of math.fsum, at every run boundary"""
    import math
    rng = np.random.default_rng(0)
    A = rng.standard_normal((5000, 3)).astype(np.float32)
    for n in (4, 63, 64, 65, 128, 129, 4097):
        idx = rng.permutation(5000)[:n]
        got = H.blocked_means(A, idx, np.array([0]), np.array([n]))[0]
        want = np.array([math.fsum(A[idx, k].astype(np.float64).tolist()) / n for k in range(3)])
        assert np.abs(got - want).max() <= 2.0 ** -23 * np.abs(A).max()


def test_the_volume_claim():
    """The r = 0.6 sphere on the 24-point grid cut by the box at z = x[13]: the cap volume is pi h^2 (3 r - h) / 3, h = x[13] + r.
    The open mesh's signed volume misses it by more than 8 %, the filled one is within 3 % (the rest is marching cubes'
    discretisation); the corner-cut sphere goes from a negative volume to a positive one."""
    v, f, _, exact = H.cut_sphere()
    o = H.fill(v, f)
    vol0, vol1 = R.measure(v, f)["volume"], R.measure(o["verts"], o["faces"])["volume"]
    print(f"cut sphere: open {vol0:.5f} ({100 * (vol0 / exact - 1):+.2f} %), filled {vol1:.5f} ({100 * (vol1 / exact - 1):+.2f} %), exact {exact:.5f}")
    assert abs(vol1 - exact) <= 0.03 * exact
    assert abs(vol0 - exact) > 0.08 * exact
    v, f, _ = H.corner_sphere()
    o = H.fill(v, f)
    vol0, vol1 = R.measure(v, f)["volume"], R.measure(o["verts"], o["faces"])["volume"]
    print(f"corner-cut sphere: open {vol0:.5f}, filled {vol1:.5f}")
    assert vol0 < 0 < vol1 and R.measure(o["verts"], o["faces"])["closed"]


# ------------------------------------------------------------------------------------------- the header's functions on the host
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("meshfill_host") / "meshfill_host_main")
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "meshfill_host_main.cpp"), "-o", exe]
    r = subprocess.run(base + SAN, capture_output=True, text=True)
    if r.returncode != 0:
        assert "sanitize" in r.stderr or "asan" in r.stderr or "ubsan" in r.stderr, r.stderr      # only a failed sanitizer link falls back
        subprocess.run(base, check=True)
    return exe


def run_program(program, tmp_path, v, f, col, max_edges):
    V, F = len(v), len(f)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([V, F, col is not None], np.int32).tobytes() + np.ascontiguousarray(v, np.float32).tobytes() +
                 np.ascontiguousarray(f, np.int32).tobytes() + (b"" if col is None else np.ascontiguousarray(col, np.float32).tobytes()))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(max_edges or 0)], capture_output=True, text=True,
                       timeout=120, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, r.stderr[-3000:]
    raw = open(tmp_path / "out.bin", "rb").read()
    counts = np.frombuffer(raw, np.int32, 8, 0)
    out = dict(info=dict(zip(KEYS, counts.tolist())))
    L, Vo, Fo = int(counts[1]), V + int(counts[6]), F + int(counts[7])
    at = 32
    out["table"] = np.frombuffer(raw, np.int32, 2 * L, at).reshape(L, 2)
    at += 8 * L
    out["loop_offsets"] = np.frombuffer(raw, np.int32, L + 1, at)
    at += 4 * (L + 1)
    M = int(out["loop_offsets"][-1])
    out["loop_vertices"] = np.frombuffer(raw, np.int32, M, at)
    at += 4 * M
    out["verts"] = np.frombuffer(raw, np.float32, 3 * Vo, at).reshape(Vo, 3)
    at += 12 * Vo
    out["faces"] = np.frombuffer(raw, np.int32, 3 * Fo, at).reshape(Fo, 3)
    at += 12 * Fo
    if col is not None:
        out["colors"] = np.frombuffer(raw, np.float32, 3 * Vo, at).reshape(Vo, 3)
        at += 12 * Vo
    assert at == len(raw)
    return out


def same(got, want, colors=True):
    assert got["info"] == want["info"]
    for k in ("table", "loop_offsets", "loop_vertices", "faces"):
        assert np.array_equal(got[k], want[k]), k
    assert got["verts"].tobytes() == want["verts"].tobytes()
    if colors:
        assert got["colors"].tobytes() == want["colors"].tobytes()


@pytest.mark.parametrize("name", sorted(MESHES))
@pytest.mark.parametrize("max_edges", [None, 4])
def test_header_functions_equal_the_replay_bit_for_bit(program, tmp_path, name, max_edges):
    v, f = MESHES[name]
    col = np.random.default_rng(len(v)).random(v.shape).astype(np.float32)
    same(run_program(program, tmp_path, v, f, col, max_edges), H.fill(v, f, col, max_edges))


@pytest.mark.parametrize("n", [3, 4, 5, 63, 64, 65, 127, 128, 129, 4096, 4097])
def test_header_functions_at_every_run_boundary(program, tmp_path, n):
    v, f = R.fan(n)
    f = H.permuted(f, n)
    v = (v * np.float32(1.37) + np.float32(0.1)).astype(np.float32)
    want = H.fill(v, f)
    assert want["table"][:, 1].tolist() == [n]
    same(run_program(program, tmp_path, v, f, None, None), want, colors=False)
