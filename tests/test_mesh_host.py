"""Marching cubes without a GPU: the generated case table (tools/gen_mc_tables.py), its invariants, and the numpy restatement
of the kernels' contract (tests/mc_numpy.py) on shapes with a known topology, area and volume; the OBJ writer."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mc_numpy as M

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_mc_tables as G  # noqa: E402


def test_committed_table_matches_the_generator():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_mc_tables.py"), "--check"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def test_table_invariants():
    assert M.NTRI[0] == 0 and M.NTRI[255] == 0
    assert M.TRI.shape[1] == 3 * M.NTRI.max()
    for case in range(256):
        n = M.NTRI[case]
        used = M.TRI[case, :3 * n]
        assert (M.TRI[case, 3 * n:] == -1).all()
        crossing = {e for e in range(12) if (case >> G.edge_corners(e)[0] & 1) != (case >> G.edge_corners(e)[1] & 1)}
        assert set(used.tolist()) == crossing, case                  # exactly the crossing edges, each used
        assert n <= 5


def test_face_pairing_rule():
    """On every face: 2 crossings pair with each other; 4 crossings (diagonal inside corners) pair so that each inside corner
    is cut off on its own - the two edges at that inside corner form a boundary segment of the case's triangles."""
    for case in range(256):
        tris = M.TRI[case, :3 * M.NTRI[case]].reshape(-1, 3)
        directed = {(int(t[i]), int(t[(i + 1) % 3])) for t in tris for i in range(3)}
        undirected = {tuple(sorted(e)) for e in directed}
        for ring in G.faces():
            ins = [case >> c & 1 for c in ring]
            if sum(ins) in (0, 4):
                continue
            for s in range(4):
                if ins[s] and not ins[s - 1] and not ins[(s + 1) % 4]:       # an isolated inside corner on this face
                    a, b = G.edge_between(ring[s - 1], ring[s]), G.edge_between(ring[s], ring[(s + 1) % 4])
                    assert (a, b) in directed, (case, ring, a, b)             # entry -> exit, oriented
            if sum(ins) == 2 and ins[0] == ins[2]:                            # ambiguous: inside corners never joined
                out = [s for s in range(4) if not ins[s]]
                for s in out:
                    a, b = G.edge_between(ring[s - 1], ring[s]), G.edge_between(ring[s], ring[(s + 1) % 4])
                    assert (min(a, b), max(a, b)) not in undirected, (case, "outside corner cut off on an ambiguous face")


SHAPES = {"sphere": (lambda: M.sphere(40), 0.0, 2), "torus": (lambda: M.torus(48), 0.0, 0), "two_spheres": (lambda: M.two_spheres(48), 0.0, 4)}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_closed_manifold_and_euler(name):
    make, level, chi = SHAPES[name]
    f, h = make()
    v, fa, n, _ = M.marching_cubes(f, level, (h,) * 3, (-1.,) * 3)
    assert len(fa) > 100
    assert M.is_closed_oriented_manifold(fa)
    assert M.euler_characteristic(len(v), fa) == chi
    # vertex normals agree with the winding: outward from the dense region
    tri = v[fa.astype(np.int64)].astype(np.float64)
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nv = n[fa.astype(np.int64)].sum(1)
    assert (np.einsum("ij,ij->i", fn, nv) > 0).mean() > 0.99


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("level", [-0.2, 0.0, 0.3])
def test_noise_is_a_closed_manifold(seed, level):
    f = M.noise((20, 24, 18), seed=seed, pad=True)
    v, fa, n, _ = M.marching_cubes(f, level)
    assert len(fa) > 0 and M.is_closed_oriented_manifold(fa)
    assert M.euler_characteristic(len(v), fa) % 2 == 0
    assert M.area_volume(v, fa)[1] > 0


def test_sphere_area_and_volume():
    f, h = M.sphere(64, r=0.6)
    v, fa, _, _ = M.marching_cubes(f, 0.0, (h,) * 3, (-1.,) * 3)
    area, vol = M.area_volume(v, fa)
    assert abs(area / (4 * np.pi * 0.36) - 1) < 0.01
    assert vol > 0 and abs(vol / (4 / 3 * np.pi * 0.6 ** 3) - 1) < 0.01


def test_vertex_contract_details():
    """t, clamping, non-finite t, colour pick and coordinate order on a 2 x 2 x 2 grid, by hand."""
    f = np.full((2, 2, 2), -1, np.float32)
    f[0, 0, 0] = 3.0                                     # edges from (0,0,0): t = (0 - 3) / (-1 - 3) = 0.75
    cols = np.arange(24, dtype=np.float32).reshape(2, 2, 2, 3)
    v, fa, n, c = M.marching_cubes(f, 0.0, (2., 3., 4.), (10., 20., 30.), colors=cols)
    assert len(v) == 3 and fa.tolist() == [[0, 1, 2]]
    np.testing.assert_array_equal(v[0], np.float32([(0 + 0.75) * 2 + 10, 20, 30]))
    np.testing.assert_array_equal(v[2], np.float32([10, 20, (0 + 0.75) * 4 + 30]))
    np.testing.assert_array_equal(c[0], cols[1, 0, 0])   # t > 0.5: the far end point
    assert np.allclose(np.linalg.norm(n, axis=1), 1)
    f2 = f.copy()
    f2[1, 0, 0] = np.nan                                 # NaN is outside; t NaN -> 0.5, normal non-finite -> 0
    v2, _, n2, c2 = M.marching_cubes(f2, 0.0, colors=cols)
    assert v2[0, 0] == np.float32(0.5) and (n2[0] == 0).all() and (c2[0] == cols[0, 0, 0]).all()


def test_obj_round_trip(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "sw-nerf_amd"))
    from swnerf import mesh
    f, h = M.sphere(16)
    rng = np.random.default_rng(3)
    v, fa, n, _ = M.marching_cubes(f, 0.0, (h,) * 3, (-1.,) * 3)
    cols = rng.uniform(-0.5, 1.5, (len(v), 3)).astype(np.float32)
    for c in (cols, None):
        p = mesh.Mesh(v, fa, n, c).export(str(tmp_path / "m.obj"))
        v2, f2, n2, c2 = mesh.load_obj(p)
        np.testing.assert_array_equal(v2, v)
        np.testing.assert_array_equal(f2, fa)
        np.testing.assert_array_equal(n2, n)
        if c is None:
            assert c2 is None
        else:
            np.testing.assert_array_equal(c2, np.clip(c, 0, 1))
    text = open(p).read().splitlines()
    assert text[1].startswith("v ") and len(text[1].split()) == 4
    assert any(t.startswith("f ") and "//" in t for t in text)
    empty = mesh.Mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32)).export(str(tmp_path / "e.obj"))
    assert mesh.load_obj(empty)[0].shape == (0, 3)
