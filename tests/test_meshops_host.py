"""Mesh clean-up and measurement without a GPU: the header-derived exports, the workspace size, the Python refusals, and
csrc/meshops_math.h on the host - tests/meshops_host_main.cpp, a stand-alone program that loops the header's functions over
exact-size heap buffers, is built with g++ under AddressSanitizer and UBSan (without them when the sanitizer runtime cannot be
linked, as tests/test_markers_math_host.py does) and must equal the numpy replay of tests/meshops_ref.py bit for bit: the device
kernels call the same functions."""
import os
import subprocess

import numpy as np
import pytest

import meshops_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "sw-nerf_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
NAMES = ["swnerf_mesh_workspace_bytes", "swnerf_mesh_components", "swnerf_mesh_compact", "swnerf_mesh_incidence",
         "swnerf_mesh_smooth_step", "swnerf_mesh_vertex_normals", "swnerf_mesh_measure"]


def test_exports_come_from_the_header():
    from swnerf import _lib
    for n in NAMES:
        assert n in _lib.EXPORTS, n
    L = _lib.lib()
    assert all(hasattr(L, n) for n in NAMES)
    assert _lib.DEFINES["VERSION"] == 112


def test_workspace_bytes():
    from swnerf import _lib
    ws = _lib.lib().swnerf_mesh_workspace_bytes
    for V, F in ((-1, 0), (0, -1), (2 ** 31, 1), (1, (2 ** 31 + 2) // 3), (2 ** 40, 2 ** 40)):
        assert ws(V, F) == 0, (V, F)
    sizes = [0, 1, 3, 255, 256, 257, 360, 716, 100000, 2 ** 24, 2 ** 31 - 1]
    for V in sizes:
        prev = 0
        for F in [s for s in sizes if 3 * s < 2 ** 31]:
            b = ws(V, F)
            assert b > 0 and b % 256 == 0 and b >= prev, (V, F)
            prev = b
    for F in (0, 716):
        col = [ws(V, F) for V in sizes]
        assert col == sorted(col)
    assert ws(2 ** 31 - 1, (2 ** 31 - 1) // 3) > 0


def test_python_refusals_need_no_gpu():
    from swnerf import mesh
    v = np.zeros((4, 3), np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    with pytest.raises(ValueError, match="keep"):
        mesh.keep_components(v, f, keep=0)
    with pytest.raises(ValueError, match="keep"):
        mesh.clean((v, f), keep=-2)
    with pytest.raises(ValueError, match="min_faces"):
        mesh.keep_components(v, f, min_faces=-1)
    with pytest.raises(ValueError, match="iterations"):
        mesh.smooth(v, f, iterations=-1)
    with pytest.raises(ValueError, match="iterations"):
        mesh.clean((v, f), smooth_iterations=-3)
    with pytest.raises(ValueError, match=r"\[F,3\]"):
        mesh.components(np.zeros((2, 4), np.int32), 4)
    with pytest.raises(TypeError, match="integer"):
        mesh.vertex_faces(np.zeros((2, 3), np.float32), 4)
    with pytest.raises(ValueError, match=r"\[V,3\]"):
        mesh.smooth(np.zeros((4, 2), np.float32), f)
    with pytest.raises(TypeError, match="floating"):
        mesh.measure(np.zeros((4, 3), bool), f)
    with pytest.raises(ValueError, match="n_vertices"):
        mesh.components(f, -1)
    with pytest.raises(TypeError, match="clean"):
        mesh.generate_mesh(None, None, None, clean=3)
    with pytest.raises(TypeError, match="unknown clean option"):
        mesh.generate_mesh(None, None, None, clean={"iterations": 2})


def test_selection_rule():
    from swnerf import mesh
    table = np.array([[0, 16, 9], [3, 188, 90], [7, 16, 9], [9, 0, 1], [11, 188, 91], [20, 72, 30]])
    assert mesh.select_components(table, 1)[:, 0].tolist() == [3]                      # a tie goes to the smaller label
    assert mesh.select_components(table, 3)[:, 0].tolist() == [3, 11, 20]
    assert mesh.select_components(table, 4)[:, 0].tolist() == [0, 3, 11, 20]
    assert mesh.select_components(table, "all")[:, 0].tolist() == [0, 3, 7, 11, 20]    # min_faces=1 drops the unreferenced vertex
    assert mesh.select_components(table, "all", min_faces=0)[:, 0].tolist() == [0, 3, 7, 9, 11, 20]
    assert mesh.select_components(table, 2, min_faces=189).shape == (0, 3)
    for keep in (1, 2, 5, "all"):
        for mf in (0, 1, 17, 100):
            assert np.array_equal(mesh.select_components(table, keep, mf), R.select(table, keep, mf))


def test_reference_fixtures_are_the_documented_ones():
    fx = R.fixtures()
    shape = {k: (len(v), len(f)) for k, (v, f, _) in fx.items()}
    assert shape["two_spheres"] == (256, 504) and shape["sphere"] == (360, 716) and shape["torus"] == (600, 1200)
    assert shape["noise"] == (308, 568) and shape["floaters"] == (482, 948)
    comps = lambda k: sorted(R.component_table(fx[k][1], len(fx[k][0]))[1][:, 1].tolist(), reverse=True)
    assert comps("two_spheres") == [252, 252] and comps("sphere") == [716] and comps("floaters") == [812, 56, 40, 40]
    assert comps("noise")[:8] == [188, 132, 72, 72, 24, 16, 16, 16] and len(comps("noise")) == 12
    m = R.measure(*fx["sphere"][:2])
    assert abs(m["area"] - 4.45255) < 1e-5 and abs(m["volume"] - 0.87754) < 1e-5 and m["closed"] and m["euler"] == 2
    assert R.measure(*fx["torus"][:2])["euler"] == 0
    assert abs(R.measure(R.smooth(*fx["sphere"][:2], iterations=10), fx["sphere"][1])["volume"] - 0.88752) < 1e-5
    o = R.measure(*fx["open_sphere"][:2])
    assert not o["closed"] and o["boundary_edges"] > 0 and o["nonmanifold_edges"] == 0
    d = R.measure(*fx["duplicated_face"][:2])
    assert d["nonmanifold_edges"] == 3 and d["boundary_edges"] == 0 and not d["closed"]
    assert R.measure(*fx["unreferenced"][:2])["referenced_vertices"] == 360


# ------------------------------------------------------------------------------------------------- meshops_math.h on the host
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("meshops_host") / "meshops_host_main")
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "meshops_host_main.cpp"), "-o", exe]
    r = subprocess.run(base + SAN, capture_output=True, text=True)
    if r.returncode != 0:
        assert "sanitize" in r.stderr or "asan" in r.stderr or "ubsan" in r.stderr, r.stderr      # only a failed sanitizer link falls back
        subprocess.run(base, check=True)
    return exe


def _run(program, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program, *args], capture_output=True, text=True, timeout=120, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.parametrize("name", ["sphere", "noise", "open_sphere", "fan", "duplicated_face", "unreferenced", "repeated_index", "triangle", "empty"])
@pytest.mark.parametrize("s", [0.5, -0.53])
def test_header_functions_equal_the_replay_bit_for_bit(program, tmp_path, name, s):
    v, f, _ = R.fixtures()[name]
    V, F = len(v), len(f)
    offsets, items = R.incidence(f, V)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([V, F], np.int32).tobytes() + np.ascontiguousarray(v, np.float32).tobytes() +
                 np.ascontiguousarray(f, np.int32).tobytes() + offsets.tobytes() + items.tobytes())
    _run(program, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), repr(float(np.float32(s))))
    raw = open(tmp_path / "out.bin", "rb").read()
    sm = np.frombuffer(raw, np.float32, 3 * V, 0).reshape(V, 3)
    nr = np.frombuffer(raw, np.float32, 3 * V, 12 * V).reshape(V, 3)
    terms = np.frombuffer(raw, np.float64, 5 * F, 24 * V).reshape(F, 5)
    edges = np.frombuffer(raw, np.int64, 3, 24 * V + 40 * F)
    assert sm.tobytes() == R.smooth_step(v, f, s).tobytes()
    assert terms.tobytes() == R.face_terms(v, f).tobytes()
    assert np.array_equal(nr, R.vertex_normals(v, f).astype(np.float32))
    assert edges.tolist() == list(R.edge_counts(f))
