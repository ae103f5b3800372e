"""swnerf.mesh hole filling on the GPU against the numpy replay of tests/meshfill_ref.py: faces, loops and every count exactly, the
bytes of positions and colours exactly, recomputed normals to one float32 ulp (2^-23, the gate of tests/test_gpu_meshsimp.py), the
first V rows and F faces the input bit for bit.  The large cases have more elements than the 1024 x 256 threads of a grid-stride
launch: one loop of 300 000 edges (19 rounds of pointer jumping) and the unpadded noise((118,118,118), seed=5) at level 0.3
(1.97 M corners, 1695 loops)."""
import math

import numpy as np
import pytest
import torch

import mc_numpy as M
import meshops_ref as R
import meshfill_ref as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURES = ["two_spheres", "sphere", "torus", "noise", "floaters", "open_sphere", "fan", "empty", "triangle", "duplicated_face", "unreferenced",
            "repeated_index"]
EXTRA = ["cut_sphere", "corner_sphere", "cut_torus", "open_noise", "pinched", "bow_tie", "three_on_an_edge"]
CLOSED = ["sphere", "noise", "torus", "two_spheres"]
KEYS = ["boundary_edges", "loops", "filled_loops", "filled_edges", "skipped_loops", "unfillable_edges", "new_vertices", "new_faces"]
_CACHE = {}


@pytest.fixture(scope="module")
def fx():
    out = {k: (v, f, n) for k, (v, f, n) in R.fixtures().items()}
    out["cut_sphere"] = H.cut_sphere()[:3]
    out["corner_sphere"] = H.corner_sphere()
    out["cut_torus"] = H.cut_torus()
    out["open_noise"] = H.open_noise()
    out["pinched"] = H.pinched() + (None,)
    out["bow_tie"] = (np.arange(15, dtype=np.float32).reshape(5, 3) ** 2 % 7, np.array([[0, 1, 2], [0, 3, 4]], np.int32), None)
    out["three_on_an_edge"] = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, -1, 0]], np.float32),
                               np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]], np.int32), None)
    return out


def attrs(v, n):
    """normals (the fixture's, or made up) and colours for a fixture"""
    rng = np.random.default_rng(len(v) + 1)
    return (rng.standard_normal(v.shape).astype(np.float32) if n is None else n), rng.random(v.shape).astype(np.float32)


def ref(key, make):
    """reference results, computed once and never modified"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def same_fill(got, w, v, f, with_normals=True):
    """(verts, faces, normals, colors, info) of fill_holes_arrays against the replay `w` of the input (v, f)"""
    gv, gf, gn, gc, info = got
    print({k: info[k] for k in KEYS})
    assert [info[k] for k in KEYS] == [w["info"][k] for k in KEYS]
    assert gf.dtype == torch.int32 and np.array_equal(gf.cpu().numpy(), w["faces"])
    assert gv.dtype == torch.float32 and gv.cpu().numpy().tobytes() == w["verts"].tobytes()
    assert gv.cpu().numpy()[:len(v)].tobytes() == v.tobytes() and np.array_equal(gf.cpu().numpy()[:len(f)], f)
    if w["colors"] is not None:
        assert gc.cpu().numpy().tobytes() == w["colors"].tobytes()
    if with_normals and gn is not None and info["new_faces"]:
        err = float(np.abs(gn.cpu().numpy().astype(np.float64) - R.vertex_normals(w["verts"], w["faces"])).max())
        assert gn.dtype == torch.float32 and err <= 2.0 ** -23, err


def same_loops(got, w):
    table, off, lv, info = got
    assert table.dtype == np.int64 and np.array_equal(table, w["table"])
    assert off.dtype == torch.int32 and np.array_equal(off.cpu().numpy(), w["loop_offsets"])
    assert lv.dtype == torch.int32 and np.array_equal(lv.cpu().numpy(), w["loop_vertices"])
    assert (info["boundary_edges"], info["loops"], info["unfillable_edges"]) == (w["info"]["boundary_edges"], w["info"]["loops"], w["info"]["unfillable_edges"])


# ------------------------------------------------------------------------------------------------------------ against the replay
@pytest.mark.parametrize("name", FIXTURES + EXTRA)
def test_fill_equals_the_replay(fx, name):
    from swnerf import mesh
    v, f, n = fx[name]
    n, col = attrs(v, n)
    w = ref((name, None), lambda: H.fill(v, f, col))
    dv, df, dn, dc = dev(v), dev(f), dev(n), dev(col)
    keep = [t.clone() for t in (dv, df, dn, dc)]
    got = mesh.fill_holes_arrays(dv, df, dn, dc)
    same_fill(got, w, v, f)
    for a, b in zip(keep, (dv, df, dn, dc)):
        assert torch.equal(a, b)                                     # the inputs are never written
    again = mesh.fill_holes_arrays(dv, df, dn, dc)
    for a, b in zip(got[:4], again[:4]):
        assert torch.equal(a, b)                                     # two runs: the same bits
    if w["info"]["new_faces"] == 0:
        assert got[0] is dv and got[1] is df and got[2] is dn and got[3] is dc       # nothing added: the input tensors themselves
    same_loops(mesh.boundary_loops(df, len(v)), w)
    bare = mesh.fill_holes_arrays(dv, df)
    assert bare[2] is None and bare[3] is None and torch.equal(bare[0], got[0]) and torch.equal(bare[1], got[1])


def test_the_issues_sizes(fx):
    from swnerf import mesh
    v, f, _ = fx["open_sphere"]
    assert (len(v), len(f)) == (360, 358)
    gv, gf, _, _, info = mesh.fill_holes_arrays(dev(v), dev(f))
    assert (gv.shape[0], gf.shape[0], info["loops"], info["filled_edges"]) == (361, 410, 1, 52)
    v, f, _ = fx["triangle"]
    m = mesh.fill_holes(v, faces=f)
    assert (len(m.vertices), len(m.faces)) == (3, 2) and m.fill_info["new_vertices"] == 0
    r = m.measure()
    assert r.closed and r.volume == 0
    v, f, _ = fx["duplicated_face"]
    m = mesh.fill_holes(v, faces=f)
    assert m.fill_info["boundary_edges"] == 0 and len(m.faces) == len(f) and not m.measure().closed
    table, _, _, info = mesh.boundary_loops(fx["cut_torus"][1], len(fx["cut_torus"][0]))
    assert table[:, 1].tolist() == [56, 24]
    table, _, _, info = mesh.boundary_loops(fx["open_noise"][1], len(fx["open_noise"][0]))
    assert len(table) == 13 and int((table[:, 1] == 4).sum()) == 6
    for name in CLOSED:
        v, f, _ = fx[name]
        assert mesh.fill_holes(v, faces=f).fill_info == dict(zip(KEYS, [0] * 8))


@pytest.mark.parametrize("n", [3, 4, 5, 63, 64, 65, 127, 128, 129, 4096, 4097])
def test_loop_lengths_around_every_boundary(n):
    """the n == 3 branch, the 64-rank runs and the doubling rounds; the faces in a seeded random order with rotated corners, so the
    leader is not first in memory and next jumps at random"""
    from swnerf import mesh
    v, f = R.fan(n)
    f = H.permuted(f, n)
    v = (v * np.float32(1.37) + np.float32(0.1)).astype(np.float32)
    col = attrs(v, None)[1]
    w = H.fill(v, f, col)
    assert w["table"][:, 1].tolist() == [n]
    same_fill(mesh.fill_holes_arrays(dev(v), dev(f), None, dev(col)), w, v, f)
    same_loops(mesh.boundary_loops(dev(f), len(v)), w)


@pytest.fixture(scope="module")
def large():
    v, f, n, _ = M.marching_cubes(M.noise((118, 118, 118), seed=5, pad=False), 0.3)
    assert (len(v), len(f)) == (364586, 655328)
    return v, f, n


def test_more_elements_than_one_launchs_threads_many_loops(large):
    from swnerf import mesh
    v, f, n = large
    col = attrs(v, None)[1]
    w = H.fill(v, f, col)
    assert (len(w["verts"]), len(w["faces"]), w["info"]["loops"], w["info"]["boundary_edges"]) == (366281, 667670, 1695, 12342)
    got = mesh.fill_holes_arrays(dev(v), dev(f), dev(n), dev(col))
    same_fill(got, w, v, f)
    m = mesh.measure(got[0], got[1])
    assert m.closed and m.nonmanifold_edges == 0 and m.boundary_edges == 0


def test_more_elements_than_one_launchs_threads_one_loop():
    from swnerf import mesh
    v, f = R.fan(300000)
    f = H.permuted(f, 300000)
    w = H.fill(v, f)
    assert w["table"][:, 1].tolist() == [300000] and 300000 > 1024 * 256
    same_fill(mesh.fill_holes_arrays(dev(v), dev(f)), w, v, f)


# ----------------------------------------------------------------------------------------------------- unfillable parts, max_edges
def test_unfillable_parts_are_left_alone(fx):
    from swnerf import mesh
    v, f, _ = fx["pinched"]
    m = mesh.fill_holes(v, faces=f)
    assert [m.fill_info[k] for k in KEYS] == [74, 1, 1, 52, 0, 22, 1, 52]
    assert np.array_equal(m.faces[:len(f)], f) and mesh.measure(m).boundary_edges == 22
    v, f, _ = fx["bow_tie"]
    m = mesh.fill_holes(v, faces=f)
    assert (m.fill_info["boundary_edges"], m.fill_info["loops"], m.fill_info["unfillable_edges"], len(m.faces)) == (6, 0, 6, 2)
    v, f, _ = fx["three_on_an_edge"]
    m = mesh.fill_holes(v, faces=f)
    assert (m.fill_info["boundary_edges"], m.fill_info["loops"], len(m.faces)) == (6, 0, 3) and mesh.measure(m).nonmanifold_edges == 1


def test_max_edges(fx):
    from swnerf import mesh
    v, f, n = fx["open_noise"]
    col = attrs(v, n)[1]
    for me, (nfill, nskip) in ((4, (6, 7)), (3, (0, 13)), (13, (11, 2)), (24, (13, 0))):
        w = H.fill(v, f, col, max_edges=me)
        got = mesh.fill_holes_arrays(dev(v), dev(f), dev(n), dev(col), max_edges=me)
        same_fill(got, w, v, f)
        assert (got[4]["filled_loops"], got[4]["skipped_loops"]) == (nfill, nskip)
    assert mesh.fill_holes_arrays(dev(v), dev(f), max_edges=3)[0].shape[0] == len(v)


def test_a_bad_index_raises(fx):
    from swnerf import mesh
    v, f, _ = fx["open_sphere"]
    for where, n in (([len(f) - 1], 1), ([0, 5], 2)):
        bad = f.copy()
        for i in where:
            bad[i, 2] = len(v) if i else -1
        with pytest.raises(ValueError, match=f"{n} face indices"):
            mesh.fill_holes_arrays(dev(v), dev(bad))
        with pytest.raises(ValueError, match=f"{n} face indices"):
            mesh.boundary_loops(dev(bad), len(v))


def test_c_abi_counts_a_bad_index_and_writes_nothing(fx):
    """swnerf_mesh_boundary itself: the bad index in the last face is counted, nb = 0, and bhe / bnext stay as they were"""
    from swnerf import _lib
    v, f, _ = fx["open_sphere"]
    V, F = len(v), len(f)
    bad = f.copy()
    bad[-1, 1] = V + 3
    df = dev(bad)
    ws = torch.empty(int(_lib.lib().swnerf_mesh_fill_workspace_bytes(V, F)), dtype=torch.uint8, device=DEV)
    bhe, bnext = torch.full((3 * F,), -7, dtype=torch.int32, device=DEV), torch.full((3 * F,), -7, dtype=torch.int32, device=DEV)
    counts = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().swnerf_mesh_boundary(_lib.ptr(df), V, F, _lib.ptr(ws), _lib.ptr(bhe), _lib.ptr(bnext), _lib.ptr(counts), _lib.stream_of(df)),
               "mesh_boundary")
    assert counts.tolist() == [0, 1] and bool((bhe == -7).all()) and bool((bnext == -7).all())


# ------------------------------------------------------------------------------------------------------- entry-point consistency
@pytest.mark.parametrize("name", FIXTURES + EXTRA)
def test_entry_points_agree(fx, name):
    from swnerf import mesh
    v, f, _ = fx[name]
    m0 = mesh.measure(v, f)
    table, off, lv, info = mesh.boundary_loops(f, len(v))
    assert info["boundary_edges"] + H.self_edges(f, len(v)) == m0.boundary_edges     # measure() also counts an edge x -> x
    assert H.self_edges(f, len(v)) == (1 if name == "repeated_index" else 0)
    assert int(off[-1]) == lv.shape[0] == info["boundary_edges"] - info["unfillable_edges"] and len(table) == info["loops"]
    filled = mesh.fill_holes(v, faces=f)
    m1 = filled.measure()
    assert m1.boundary_edges == m0.boundary_edges - filled.fill_info["filled_edges"] and m1.n_components == m0.n_components
    w = ref((name, "bare"), lambda: H.fill(v, f))
    wm = R.measure(w["verts"], w["faces"])
    assert (m1.closed, m1.euler, m1.nonmanifold_edges) == (wm["closed"], wm["euler"], wm["nonmanifold_edges"])
    bound = 2 * len(w["faces"]) * 2.0 ** -53 * math.fsum(np.abs(wm["terms"][:, 1]).tolist())
    print(f"{name}: volume {m0.volume:.9g} -> {m1.volume:.9g}, |d| = {abs(m1.volume - wm['volume']):.3e}, bound = {bound:.3e}")
    assert abs(m1.volume - float(wm["volume"])) <= bound
    if name in ("open_sphere", "fan", "cut_sphere", "corner_sphere", "cut_torus", "open_noise"):
        assert m1.closed and not m0.closed and m1.volume > 0
    if name in ("open_sphere", "fan", "cut_sphere", "corner_sphere", "cut_torus"):
        assert m1.euler == 2


def test_the_volume_claim_on_the_device():
    from swnerf import mesh
    v, f, _, exact = H.cut_sphere()
    vol0, vol1 = mesh.measure(v, f).volume, mesh.fill_holes(v, faces=f).measure().volume
    assert abs(vol1 - exact) <= 0.03 * exact and abs(vol0 - exact) > 0.08 * exact
    v, f, _ = H.corner_sphere()
    assert mesh.measure(v, f).volume < 0 < mesh.fill_holes(v, faces=f).measure().volume


# ------------------------------------------------------------------------------------------------------------------ the pipeline
def test_clean_fills_before_it_smooths(fx):
    from swnerf import mesh
    v, f, n = fx["cut_sphere"]
    col = attrs(v, n)[1]
    m = mesh.Mesh(v, f, n, col)
    c = mesh.clean(m, fill_holes=True)
    w = H.fill(v, f, col)
    assert c.vertices.tobytes() == w["verts"].tobytes() and np.array_equal(c.faces, w["faces"]) and c.vertex_colors.tobytes() == w["colors"].tobytes()
    assert c.measure().closed and not mesh.clean(m).measure().closed
    s = mesh.clean(m, fill_holes=True, smooth_iterations=3)
    assert s.vertices.tobytes() == R.smooth(w["verts"], w["faces"], 3).tobytes()       # the caps are smoothed with the rest
    assert np.abs(s.vertex_normals.astype(np.float64) - R.vertex_normals(s.vertices, s.faces)).max() <= 2.0 ** -23
    q = mesh.clean(m, fill_holes=8)
    assert np.array_equal(q.faces, f) and not q.measure().closed                      # the one loop has 56 edges


def test_generate_mesh_closes_a_field_that_touches_the_bounds():
    from swnerf import mesh
    field, h = M.sphere(24)
    x = np.linspace(-1., 1., 24)
    X = np.meshgrid(x, x, x[:14], indexing="ij")
    d = field[:, :, :14].astype(np.float64)
    colors = np.random.default_rng(2).random(d.shape + (3,))
    a = mesh.generate_mesh(d, colors, X, density_threshold=0., clean={"fill_holes": True})
    b = mesh.generate_mesh(d, colors, X, density_threshold=0., clean={"fill_holes": True})
    o = mesh.generate_mesh(d, colors, X, density_threshold=0.)
    assert not o.measure().closed
    r = a.measure()
    assert r.closed and r.euler == 2 and r.volume > 0
    assert len(a.vertices) == len(o.vertices) + 1 and a.vertex_colors is not None and a.vertex_colors.shape == a.vertices.shape
    assert a.vertex_colors[:len(o.vertices)].tobytes() == o.vertex_colors.tobytes()
    for k in ("vertices", "faces", "vertex_normals", "vertex_colors"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k                  # two runs: the same bits
