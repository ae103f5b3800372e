"""swnerf.mesh welding and decimation on the GPU against the numpy replay of tests/meshsimp_ref.py: labels, counts, faces and the
bytes of positions and colours exactly; recomputed normals to one float32 ulp.  The large case is the one of
tests/test_gpu_meshops.py, noise((118,118,118), seed=5) at level 0.3 (V = 369654: more than the 1024 x 256 threads of a
grid-stride launch), at a cell of 3 spacings."""
import numpy as np
import pytest
import torch

import mc_numpy as M
import meshops_ref as R
import meshsimp_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LARGE_VF = (369654, 674416)
NAMES = ["two_spheres", "sphere", "torus", "noise", "floaters", "open_sphere", "fan", "empty", "triangle", "duplicated_face", "unreferenced",
         "repeated_index"]
PLACEMENTS = ["weld", "mean", "quadric"]
_CACHE = {}


@pytest.fixture(scope="module")
def fx():
    return R.fixtures()


@pytest.fixture(scope="module")
def large():
    v, f, n, _ = M.marching_cubes(M.noise((118, 118, 118), seed=5), 0.3)
    assert (len(v), len(f)) == LARGE_VF
    return v, f, n


@pytest.fixture(scope="module")
def sphere32():
    field, h = M.sphere(32)
    v, f, n = R.mc(field, 0., h)
    assert (len(v), len(f)) == (1608, 3212)
    return v, f, n, h


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


def same_mesh(got, w, placement, with_normals=True):
    gv, gf, gn, gc = got
    assert gf.dtype == torch.int32 and np.array_equal(gf.cpu().numpy(), w["faces"])
    assert gv.dtype == torch.float32 and gv.cpu().numpy().tobytes() == w["verts"].tobytes()
    assert gc.cpu().numpy().tobytes() == w["colors"].tobytes()
    if not with_normals:
        return
    if placement == "weld":
        assert gn.cpu().numpy().tobytes() == w["normals"].tobytes()
    else:
        err = float(np.abs(gn.cpu().numpy().astype(np.float64) - w["normals"]).max()) if len(w["verts"]) else 0.
        assert gn.dtype == torch.float32 and err <= 2.0 ** -23, err


# ------------------------------------------------------------------------------------------------------------ against the replay
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("cells", [1.5, 2.5])
def test_simplify_equals_the_replay(fx, name, cells):
    from swnerf import mesh
    v, f, n = fx[name]
    n, col = attrs(v, n)
    h = float(np.float32(cells * S.spacing(name)))
    dv, df = dev(v), dev(f)
    c = ref((name, cells, "cluster"), lambda: S.cluster(v, h))
    vlabel, clusters = mesh.cluster(dv, h)
    assert vlabel.dtype == torch.int32 and np.array_equal(vlabel.cpu().numpy(), c["vlabel"]) and clusters == c["clusters"]
    for placement in PLACEMENTS:
        w = ref((name, cells, placement), lambda: S.simplify(v, f, n, col, h, placement))
        got = mesh.simplify_arrays(dv, df, dev(n), dev(col), h, placement)
        same_mesh(got, w, placement)
        assert mesh.collapse_counts(dv, df, h) == dict(vertices=w["V_out"], faces=w["F_out"], degenerate=w["degenerate"],
                                                       duplicate=w["duplicate"], clusters=w["clusters"])
        bare = mesh.simplify_arrays(dv, df, None, None, h, placement)
        assert bare[2] is None and bare[3] is None and torch.equal(bare[0], got[0]) and torch.equal(bare[1], got[1])
    assert dv.cpu().numpy().tobytes() == v.tobytes() and np.array_equal(df.cpu().numpy(), f)      # the inputs are never written


def test_a_given_origin_and_eps(fx):
    from swnerf import mesh
    v, f, n = fx["torus"]
    n, col = attrs(v, n)
    o = (-1.03, -1.01, -1.07)
    for eps in (1e-3, 0.05):
        w = S.simplify(v, f, n, col, 0.2, "quadric", eps, origin=o)
        same_mesh(mesh.simplify_arrays(dev(v), dev(f), dev(n), dev(col), 0.2, "quadric", eps, origin=o), w, "quadric")
    assert np.array_equal(mesh.cluster(dev(v), 0.2, origin=dev(np.array(o, np.float32)))[0].cpu().numpy(), S.cluster(v, 0.2, o)["vlabel"])
    with pytest.raises(ValueError, match=f"{int((v[:, 0] < 0).sum())} vertices have no cell"):
        mesh.cluster(dev(v), 0.2, origin=(0., -1., -1.))             # below the origin: no cell


# ------------------------------------------------------------------------------------------------------------------ edge cells
def test_one_cell_for_everything_and_one_cell_per_vertex(fx):
    from swnerf import mesh
    v, f, n = fx["sphere"]
    n, col = attrs(v, n)
    ext = float((v.max(0) - v.min(0)).max())
    vlabel, clusters = mesh.cluster(dev(v), 2 * ext)
    assert clusters == 1 and int(vlabel.max()) == 0
    for placement in PLACEMENTS:
        gv, gf, gn, gc = mesh.simplify_arrays(dev(v), dev(f), dev(n), dev(col), 2 * ext, placement)
        assert tuple(gv.shape) == (0, 3) and tuple(gf.shape) == (0, 3)
    assert mesh.collapse_counts(dev(v), dev(f), 2 * ext) == dict(vertices=0, faces=0, degenerate=716, duplicate=0, clusters=1)
    vlabel, clusters = mesh.cluster(dev(v), ext * 2.0 ** -20)
    assert clusters == 360 and np.array_equal(vlabel.cpu().numpy(), np.arange(360))
    gv, gf, gn, gc = mesh.weld_arrays(dev(v), dev(f), dev(n), dev(col))          # the default tolerance
    assert gv.cpu().numpy().tobytes() == v.tobytes() and np.array_equal(gf.cpu().numpy(), f)
    assert gn.cpu().numpy().tobytes() == n.tobytes() and gc.cpu().numpy().tobytes() == col.tobytes()


# ------------------------------------------------------------------------------------------------------------- exact identities
def test_a_triangle_soup_welds_back(fx):
    from swnerf import mesh
    v, f, n = fx["sphere"]
    soup_v, soup_f = v[f].reshape(-1, 3), np.arange(3 * len(f), dtype=np.int32).reshape(-1, 3)
    before = mesh.measure(soup_v, soup_f)
    assert not before.closed and before.n_components == 716
    m = mesh.weld(soup_v, faces=soup_f)
    assert (len(m.vertices), len(m.faces)) == (360, 716)
    after = m.measure()
    assert after.closed and after.euler == 2 and after.boundary_edges == 0 and after.nonmanifold_edges == 0 and after.n_components == 1
    _, wv, wf = S.first_occurrence_merge(soup_v, soup_f)
    assert m.vertices.tobytes() == wv.tobytes() and np.array_equal(m.faces, wf)
    assert abs(after.volume - 0.87754) < 1e-5
    again = mesh.weld(m)
    assert again.vertices.tobytes() == m.vertices.tobytes() and again.faces.tobytes() == m.faces.tobytes()
    assert again.vertex_normals.tobytes() == m.vertex_normals.tobytes()


# ------------------------------------------------------------------------------------------------------------------ the purpose
def test_the_quadric_keeps_the_volume_the_mean_loses(sphere32):
    from swnerf import mesh
    v, f, n, h = sphere32
    vol = mesh.measure(v, f).volume
    off = {}
    for placement in ("quadric", "mean"):
        m = mesh.decimate(mesh.Mesh(v, f, n), cell=2.5 * h, placement=placement)
        assert (len(m.vertices), len(m.faces)) == (203, 402)
        ms = m.measure()
        assert ms.closed and ms.euler == 2
        off[placement] = abs(ms.volume - vol) / vol
        w = S.simplify(v, f, n, None, 2.5 * h, placement)
        assert m.vertices.tobytes() == w["verts"].tobytes() and np.array_equal(m.faces, w["faces"])
    print(f"sphere(32) at 2.5 spacings: volume off by {100 * off['quadric']:.2f} % (quadric), {100 * off['mean']:.2f} % (mean)")
    assert off["quadric"] < off["mean"] and off["quadric"] < 0.02                  # the replay: 0.78 % against 4.58 %


# ------------------------------------------------------------------------------------------------------------------------- size
def test_the_large_mesh(large):
    from swnerf import mesh
    v, f, n = large
    col = np.random.default_rng(7).random(v.shape).astype(np.float32)
    dv, df, dn, dc = dev(v), dev(f), dev(n), dev(col)
    w = S.simplify(v, f, None, col, 3., "quadric")
    vlabel, clusters = mesh.cluster(dv, 3.)
    assert np.array_equal(vlabel.cpu().numpy(), w["vlabel"]) and clusters == w["clusters"]
    assert mesh.collapse_counts(dv, df, 3.) == dict(vertices=w["V_out"], faces=w["F_out"], degenerate=w["degenerate"], duplicate=w["duplicate"],
                                                    clusters=w["clusters"])
    a = mesh.simplify_arrays(dv, df, dn, dc, 3., "quadric")
    b = mesh.simplify_arrays(dv, df, dn, dc, 3., "quadric")
    same_mesh(a, w, "quadric", with_normals=False)
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()             # two runs: the same bits
    print(f"large: {len(v)} / {len(f)} -> {w['V_out']} / {w['F_out']} ({w['degenerate']} degenerate, {w['duplicate']} duplicate)")
    assert w["duplicate"] > 0 and w["F_out"] < len(f) // 4
    for placement in ("weld", "mean"):
        w2 = S.simplify(v, f, n, col, 3., placement)
        same_mesh(mesh.simplify_arrays(dv, df, dn, dc, 3., placement), w2, placement, with_normals=placement == "weld")


# ----------------------------------------------------------------------------------------------------------------------- extent
def raw_calls(v, f, n, col, h, placement, pad, eps=1e-3):
    """The three entry points on outputs `pad` rows too long and pre-filled with -7, and a workspace of exactly the size the size
    function returns -> dict of everything written"""
    from swnerf import _lib
    L = _lib.lib()
    V, F = len(v), len(f)
    dv, df = dev(v), dev(f)
    dn, dc = (None if n is None else dev(n)), (None if col is None else dev(col))
    st = _lib.stream_of(dv)
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=DEV)
    f32 = lambda *s: torch.full(s, -7., dtype=torch.float32, device=DEV)
    ws = torch.empty(L.swnerf_mesh_simplify_workspace_bytes(V, F), dtype=torch.uint8, device=DEV)
    ws0 = torch.empty(L.swnerf_mesh_simplify_workspace_bytes(V, 0), dtype=torch.uint8, device=DEV)
    o = dict(vlabel=i32(V + pad), origin=f32(3 + pad), ccounts=i32(3 + pad), vmap=i32(V + 1 + pad), fpos=i32(F + 1 + pad), kcounts=i32(5 + pad),
             status=i32(1 + pad))
    _lib.check(L.swnerf_mesh_cluster(_lib.ptr(dv), V, None, h, _lib.ptr(ws0), _lib.ptr(o["vlabel"]), _lib.ptr(o["origin"]), _lib.ptr(o["ccounts"]), st),
               "mesh_cluster")
    _lib.check(L.swnerf_mesh_collapse(_lib.ptr(df), _lib.ptr(o["vlabel"]), V, F, _lib.ptr(ws), _lib.ptr(o["vmap"]), _lib.ptr(o["fpos"]),
                                      _lib.ptr(o["kcounts"]), st), "mesh_collapse")
    Vo, Fo = (int(x) for x in o["kcounts"][:2].cpu())
    Vo, Fo = max(Vo, 0), max(Fo, 0)
    o.update(Vo=Vo, Fo=Fo, verts=f32(Vo + pad, 3), faces=i32(Fo + pad, 3), normals=f32(Vo + pad, 3), colors=f32(Vo + pad, 3))
    origin = o["origin"] if float(o["origin"][0]) != -7. else torch.zeros(3, device=DEV)
    _lib.check(L.swnerf_mesh_collapse_emit(_lib.ptr(dv), _lib.ptr(df), _lib.ptr(dn), _lib.ptr(dc), _lib.ptr(o["vlabel"]), _lib.ptr(o["vmap"]),
                                           _lib.ptr(o["fpos"]), _lib.ptr(origin), h, V, F, S_PLACE[placement], eps, _lib.ptr(ws), Vo, Fo,
                                           _lib.ptr(o["verts"]), _lib.ptr(o["faces"]), _lib.ptr(o["normals"]), _lib.ptr(o["colors"]),
                                           _lib.ptr(o["status"]), st), "mesh_collapse_emit")
    torch.cuda.synchronize()
    return o


S_PLACE = {"weld": 0, "mean": 1, "quadric": 2}


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_nothing_is_written_past_the_extent(fx, placement):
    v, f, n = fx["floaters"]
    n, col = attrs(v, n)
    h = float(np.float32(2.5 * S.spacing("floaters")))
    w = S.simplify(v, f, n, col, h, placement)
    V, F = len(v), len(f)
    o = raw_calls(v, f, n, col, h, placement, pad=5)
    Vo, Fo = o["Vo"], o["Fo"]
    assert (Vo, Fo) == (w["V_out"], w["F_out"])
    assert o["ccounts"].tolist() == [w["clusters"], 0, 0] + [-7] * 5 and o["kcounts"].tolist() == [Vo, Fo, w["degenerate"], w["duplicate"], 0] + [-7] * 5
    assert o["status"].tolist() == [0] + [-7] * 5 and o["origin"].cpu().numpy()[:3].tobytes() == w["origin"].tobytes()
    assert bool((o["origin"][3:] == -7).all()) and bool((o["vlabel"][V:] == -7).all())
    assert bool((o["vmap"][V + 1:] == -7).all()) and bool((o["fpos"][F + 1:] == -7).all())
    assert int(o["vmap"][V]) == Vo and int(o["fpos"][F]) == Fo
    for k in ("verts", "faces", "colors"):
        n_rows = Fo if k == "faces" else Vo
        assert bool((o[k][n_rows:] == -7).all()), k
        assert o[k][:n_rows].cpu().numpy().tobytes() == w[k].tobytes(), k
    if placement == "weld":
        assert bool((o["normals"][Vo:] == -7).all()) and o["normals"][:Vo].cpu().numpy().tobytes() == w["normals"].tobytes()
    else:
        assert bool((o["normals"] == -7).all())                      # mean and quadric write no normals
    assert int(o["faces"][:Fo].min()) == 0 and int(o["faces"][:Fo].max()) == Vo - 1


# -------------------------------------------------------------------------------------------------------- refusals on the device
def test_a_nan_vertex_is_counted_and_nothing_is_written(fx):
    from swnerf import mesh
    v, f, _ = fx["sphere"]
    bad = v.copy()
    bad[17, 1] = np.nan
    bad[200, 0] = np.inf
    for call in (lambda: mesh.cluster(dev(bad), 0.2), lambda: mesh.decimate((dev(bad), dev(f)), cell=0.2), lambda: mesh.weld(dev(bad), 0.2, faces=dev(f)),
                 lambda: mesh.clean((dev(bad), dev(f)), weld=0.2), lambda: mesh.decimation_cell((dev(bad), dev(f)), 100)):
        with pytest.raises(ValueError, match="2 vertices have no cell"):
            call()
    from swnerf import _lib
    L = _lib.lib()
    V = len(v)
    db = dev(bad)
    ws = torch.empty(L.swnerf_mesh_simplify_workspace_bytes(V, 0), dtype=torch.uint8, device=DEV)
    vlabel = torch.full((V + 5,), -7, dtype=torch.int32, device=DEV)
    origin = torch.full((3 + 5,), -7., device=DEV)
    counts = torch.full((3 + 5,), -7, dtype=torch.int32, device=DEV)
    _lib.check(L.swnerf_mesh_cluster(_lib.ptr(db), V, None, 0.2, _lib.ptr(ws), _lib.ptr(vlabel), _lib.ptr(origin), _lib.ptr(counts), _lib.stream_of(db)),
               "mesh_cluster")
    assert counts.tolist() == [0, 2, 0] + [-7] * 5 and bool((vlabel == -7).all()) and bool((origin == -7).all())


def test_a_bad_face_index_is_counted_and_nothing_is_written(fx):
    from swnerf import mesh
    v, f, n = fx["sphere"]
    V = len(v)
    bad = f.copy()
    bad[100, 1] = V
    bad[500, 2] = -1
    for call in (lambda: mesh.decimate((dev(v), dev(bad)), cell=0.3), lambda: mesh.weld(dev(v), faces=dev(bad)),
                 lambda: mesh.collapse_counts(dev(v), dev(bad), 0.3), lambda: mesh.decimate((dev(v), dev(bad)), target_faces=100),
                 lambda: mesh.clean((dev(v), dev(bad)), weld=True)):
        with pytest.raises(ValueError, match="2 face indices are outside"):
            call()
    for placement in PLACEMENTS:
        o = raw_calls(v, bad, n, v, 0.3, placement, pad=4)
        assert o["kcounts"].tolist() == [0, 0, 0, 0, 2] + [-7] * 4
        assert bool((o["vmap"] == -7).all()) and bool((o["fpos"] == -7).all())
        assert o["status"].tolist() == [0] + [-7] * 4                # V_out = 0: emit has nothing to do
    # emit on a valid clustering but bad faces: the status word stops it
    from swnerf import _lib
    L = _lib.lib()
    good = raw_calls(v, f, n, v, 0.3, "quadric", pad=0)
    Vo, Fo, F = good["Vo"], good["Fo"], len(f)
    db, dv = dev(bad), dev(v)
    ws = torch.empty(L.swnerf_mesh_simplify_workspace_bytes(V, F), dtype=torch.uint8, device=DEV)
    for place in (0, 1, 2):
        vo = torch.full((Vo + 4, 3), -7., device=DEV)
        co = torch.full((Vo + 4, 3), -7., device=DEV)
        fo = torch.full((Fo + 4, 3), -7, dtype=torch.int32, device=DEV)
        status = torch.full((1 + 4,), -7, dtype=torch.int32, device=DEV)
        _lib.check(L.swnerf_mesh_collapse_emit(_lib.ptr(dv), _lib.ptr(db), None, _lib.ptr(dv), _lib.ptr(good["vlabel"]), _lib.ptr(good["vmap"]),
                                               _lib.ptr(good["fpos"]), _lib.ptr(good["origin"]), 0.3, V, F, place, 1e-3, _lib.ptr(ws), Vo, Fo, _lib.ptr(vo),
                                               _lib.ptr(fo), None, _lib.ptr(co), _lib.ptr(status), _lib.stream_of(dv)), "mesh_collapse_emit")
        assert status.tolist() == [2, -7, -7, -7, -7] and bool((vo == -7).all()) and bool((fo == -7).all()) and bool((co == -7).all())


def test_refused_sizes_and_arguments():
    from swnerf import _lib
    L = _lib.lib()
    t = torch.zeros(64, dtype=torch.int32, device=DEV)
    p = _lib.ptr(t)
    assert L.swnerf_mesh_cluster(p, 2 ** 31, None, 1., p, p, p, p, None) == _lib.E_ARG
    assert L.swnerf_mesh_cluster(p, 4, None, 0., p, p, p, p, None) == _lib.E_ARG
    assert L.swnerf_mesh_cluster(p, 4, None, float("nan"), p, p, p, p, None) == _lib.E_ARG
    assert b"finite and positive" in L.swnerf_last_error()
    assert L.swnerf_mesh_collapse(p, p, 3, (2 ** 31 + 2) // 3, p, p, p, p, None) == _lib.E_ARG
    assert L.swnerf_mesh_collapse_emit(p, p, None, None, p, p, p, p, 1., 4, 2, 3, 1e-3, p, 1, 1, p, p, None, None, p, None) == _lib.E_ARG
    assert b"placement" in L.swnerf_last_error()
    assert L.swnerf_mesh_collapse_emit(p, p, None, None, p, p, p, p, 1., 4, 2, 0, 1e-3, p, 5, 1, p, p, None, None, p, None) == _lib.E_ARG
    assert L.swnerf_mesh_collapse_emit(p, p, None, None, p, p, p, p, float("inf"), 4, 2, 0, 1e-3, p, 1, 1, p, p, None, None, p, None) == _lib.E_ARG


# ----------------------------------------------------------------------------------------------------------------- target_faces
@pytest.mark.parametrize("N", [100, 401, 402, 1000])
def test_target_faces(sphere32, N):
    from swnerf import mesh
    v, f, n, h = sphere32
    m = mesh.Mesh(v, f, n)
    cell = mesh.decimation_cell(m, N)
    d = mesh.decimate(m, target_faces=N)
    assert len(d.faces) <= N
    e = mesh.decimate(m, cell=cell)
    for k in ("vertices", "faces", "vertex_normals"):
        assert getattr(d, k).tobytes() == getattr(e, k).tobytes(), k
    ext = float((v.max(0) - v.min(0)).max())
    assert ext * 2.0 ** -20 <= cell <= ext * (1 + 1e-6) and mesh.collapse_counts(v, f, cell)["faces"] == len(d.faces)
    w = S.simplify(v, f, n, None, cell, "quadric")
    assert d.vertices.tobytes() == w["verts"].tobytes() and np.array_equal(d.faces, w["faces"])
    print(f"sphere(32): target {N} faces -> cell {cell:.6g} ({cell / h:.3f} spacings), {len(d.vertices)} / {len(d.faces)}")


def test_target_faces_that_the_mesh_already_meets(sphere32):
    from swnerf import mesh
    v, f, n, h = sphere32
    same = mesh.decimate(mesh.Mesh(v, f, n), target_faces=len(f))
    assert same.vertices.tobytes() == v.tobytes() and same.faces.tobytes() == f.tobytes() and same.vertex_normals.tobytes() == n.tobytes()
    dv, df = dev(v), dev(f)
    out = mesh.decimate_arrays(dv, df, None, None, target_faces=len(f) + 1)
    assert out[0] is dv and out[1] is df


# ------------------------------------------------------------------------------------------------------------------------ clean
def test_clean_with_and_without_the_new_keys(fx):
    from swnerf import mesh
    v, f, n = fx["floaters"]
    n, col = attrs(v, n)
    h = S.spacing("floaters")
    raw = mesh.Mesh(v, f, n, col)
    wl, wt = R.component_table(f, len(v))
    wv, wf, wn, wc = R.compact(v, f, wl, R.select(wt, 1)[:, 0], n, col)
    for m in (mesh.clean(raw), mesh.clean(raw, weld=None, decimate=None)):
        for a, b in ((m.vertices, wv), (m.faces, wf), (m.vertex_normals, wn), (m.vertex_colors, wc)):
            assert a.tobytes() == b.tobytes()                        # the new keys at None: today's bytes
    sm = mesh.clean(raw, smooth_iterations=2, weld=None, decimate=None)
    assert sm.vertices.tobytes() == R.smooth(wv, wf, 2).tobytes()
    soup_v, soup_f = v[f].reshape(-1, 3), np.arange(3 * len(f), dtype=np.int32).reshape(-1, 3)
    opts = dict(cell=2.5 * h, placement="quadric")
    got = mesh.clean((soup_v, soup_f), weld=True, decimate=opts, smooth_iterations=2)
    step = mesh.weld_arrays(dev(soup_v), dev(soup_f))
    step = mesh.keep_components(step[0], step[1], keep=1, min_faces=1)[:4]
    step = mesh.decimate_arrays(*step, **opts)
    sv = mesh.smooth(step[0], step[1], 2)
    assert got.vertices.tobytes() == sv.cpu().numpy().tobytes() and np.array_equal(got.faces, step[1].cpu().numpy())
    assert got.vertex_normals.tobytes() == mesh.vertex_normals(sv, step[1]).cpu().numpy().tobytes()
    from swnerf.meshops import default_tolerance
    w1 = S.simplify(soup_v, soup_f, h=default_tolerance(float((soup_v.max(0) - soup_v.min(0)).max())), placement="weld")
    k = R.component_table(w1["faces"], len(w1["verts"]))
    kv, kf = R.compact(w1["verts"], w1["faces"], k[0], R.select(k[1], 1)[:, 0])
    w3 = S.simplify(kv, kf, h=2.5 * h, placement="quadric")
    assert got.vertices.tobytes() == R.smooth(w3["verts"], w3["faces"], 2).tobytes() and np.array_equal(got.faces, w3["faces"])
    via = mesh.generate_mesh(*_field(), density_threshold=0., clean={"weld": True, "decimate": opts})
    assert 0 < len(via.faces) < 812 // 4 and via.measure().n_components == 1


def _field():
    field, h = R.floater_field(20)
    (X, Y, Z), _ = M.grid(20)
    return field, None, (X, Y, Z)
