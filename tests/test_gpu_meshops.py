"""swnerf.mesh clean-up and measurement on the GPU against the numpy restatement of tests/meshops_ref.py: components, selection
and compaction, incidence and the integer results exactly; smoothing bit for bit; normals to one float32 ulp; the fp64 sums to a
bound derived from the number of additions.  The large case is noise((118,118,118), seed=5) at level 0.3: V = 369654,
F = 674416 (16398 components, valence up to 17) - more than the 1024 x 256 threads of any grid-stride launch, and 1445 scan tiles
for the 1024 threads of the tile-offset pass."""
import math

import numpy as np
import pytest
import torch

import mc_numpy as M
import meshops_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LARGE_VF = (369654, 674416)
ALL = ["two_spheres", "sphere", "torus", "noise", "floaters", "open_sphere", "fan", "empty", "triangle", "duplicated_face", "unreferenced",
       "repeated_index", "large"]
_CACHE = {}


@pytest.fixture(scope="module")
def fx():
    out = R.fixtures()
    v, f, n, _ = M.marching_cubes(M.noise((118, 118, 118), seed=5), 0.3)
    assert (len(v), len(f)) == LARGE_VF
    out["large"] = (v, f, n)
    return out


def ref(fx, name, what):
    """reference results, computed once per fixture and never modified"""
    key = (name, what)
    if key not in _CACHE:
        v, f, _ = fx[name]
        _CACHE[key] = {"table": lambda: R.component_table(f, len(v)), "incidence": lambda: R.incidence(f, len(v)),
                       "measure": lambda: R.measure(v, f)}[what]()
    return _CACHE[key]


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


# ---------------------------------------------------------------------------------------------------------------- components
@pytest.mark.parametrize("name", ALL)
def test_components_equal_the_reference(fx, name):
    from swnerf import mesh
    v, f, _ = fx[name]
    vlabel, table = mesh.components(dev(f), len(v))
    want_label, want_table = ref(fx, name, "table")
    assert vlabel.dtype == torch.int32 and np.array_equal(vlabel.cpu().numpy(), want_label)
    assert table.shape == want_table.shape and np.array_equal(table, want_table)
    assert table[:, 1].sum() == len(f) and table[:, 2].sum() == len(v)


@pytest.mark.parametrize("name", ["noise", "floaters", "two_spheres", "unreferenced", "large"])
@pytest.mark.parametrize("keep", [1, 2, "all"])
@pytest.mark.parametrize("min_faces", [1, 41])
def test_keep_components_is_exactly_the_masked_mesh(fx, name, keep, min_faces):
    from swnerf import mesh
    v, f, n = fx[name]
    rng = np.random.default_rng(len(v))
    n = rng.standard_normal(v.shape).astype(np.float32) if n is None else n
    col = rng.random(v.shape).astype(np.float32)
    want_label, want_table = ref(fx, name, "table")
    rows = R.select(want_table, keep, min_faces)
    wv, wf, wn, wc = R.compact(v, f, want_label, rows[:, 0], n, col)
    gv, gf, gn, gc, labels = mesh.keep_components(dev(v), dev(f), dev(n), dev(col), keep=keep, min_faces=min_faces)
    assert labels.tolist() == rows[:, 0].tolist()
    assert gf.dtype == torch.int32 and np.array_equal(gf.cpu().numpy(), wf)
    for g, w in ((gv, wv), (gn, wn), (gc, wc)):
        assert g.cpu().numpy().tobytes() == w.tobytes()
    if name == "two_spheres" and keep == 1:
        assert labels.tolist() == [0] and len(wf) == 252                # the tie rule: the smaller label
    gv2, gf2, gn2, gc2, _ = mesh.keep_components(dev(v), dev(f), keep=keep, min_faces=min_faces)
    assert gn2 is None and gc2 is None and torch.equal(gv2, gv) and torch.equal(gf2, gf)


def test_compact_writes_nothing_past_its_extent(fx):
    from swnerf import _lib, mesh
    v, f, _ = fx["floaters"]
    V, F = len(v), len(f)
    vlabel, table = mesh.components(dev(f), V)
    rows = mesh.select_components(table, 1)
    Vo, Fo = int(rows[0, 2]), int(rows[0, 1])
    vo = torch.full((Vo + 5, 3), -7., device=DEV)
    fo = torch.full((Fo + 5, 3), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(_lib.lib().swnerf_mesh_workspace_bytes(V, F), dtype=torch.uint8, device=DEV)
    kept = dev(rows[:, 0], torch.int32)
    dv, df = dev(v), dev(f)
    _lib.check(_lib.lib().swnerf_mesh_compact(_lib.ptr(dv), _lib.ptr(df), None, None, _lib.ptr(vlabel), V, F, _lib.ptr(kept), 1, _lib.ptr(ws),
                                              Vo, Fo, _lib.ptr(vo), _lib.ptr(fo), None, None, _lib.stream_of(dv)), "mesh_compact")
    assert bool((vo[Vo:] == -7).all()) and bool((fo[Fo:] == -7).all())
    assert int(fo[:Fo].min()) == 0 and int(fo[:Fo].max()) == Vo - 1


# ----------------------------------------------------------------------------------------------------------------- incidence
@pytest.mark.parametrize("name", ALL)
def test_incidence_equals_the_reference(fx, name):
    from swnerf import mesh
    v, f, _ = fx[name]
    offsets, items = mesh.vertex_faces(dev(f), len(v))
    wo, wi = ref(fx, name, "incidence")
    assert offsets.dtype == torch.int32 and items.dtype == torch.int32
    assert np.array_equal(offsets.cpu().numpy(), wo) and np.array_equal(items.cpu().numpy(), wi)
    if name == "fan":
        assert int(offsets[1] - offsets[0]) == 300                      # past the insertion-sort threshold: the heap sort


# ----------------------------------------------------------------------------------------------------------------- smoothing
SMOOTH = ["sphere", "open_sphere", "fan", "noise", "unreferenced", "repeated_index", "duplicated_face", "large"]


@pytest.mark.parametrize("name", SMOOTH)
def test_one_smoothing_step_equals_the_replay_bit_for_bit(fx, name):
    from swnerf import mesh
    v, f, _ = fx[name]
    dv, df = dev(v), dev(f)
    inc = mesh.vertex_faces(df, len(v))
    for s in (0.5, -0.53):
        got = mesh.smooth_step(dv, df, s, incidence=inc).cpu().numpy()
        assert got.tobytes() == R.smooth_step(v, f, s).tobytes(), (name, s)
    assert dv.cpu().numpy().tobytes() == v.tobytes()


@pytest.mark.parametrize("name", ["sphere", "open_sphere", "fan", "noise"])
@pytest.mark.parametrize("iterations", [1, 5])
def test_taubin_iterations_equal_the_replay_bit_for_bit(fx, name, iterations):
    from swnerf import mesh
    v, f, _ = fx[name]
    dv, df = dev(v), dev(f)
    a = mesh.smooth(dv, df, iterations=iterations)
    b = mesh.smooth(dv, df, iterations=iterations, incidence=mesh.vertex_faces(df, len(v)))
    assert a.cpu().numpy().tobytes() == R.smooth(v, f, iterations).tobytes()
    assert torch.equal(a, b) and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()         # two runs: the same bits
    assert dv.cpu().numpy().tobytes() == v.tobytes()                                              # the input is never written
    zero = mesh.smooth(dv, df, iterations=0)
    assert zero.data_ptr() != dv.data_ptr() and zero.cpu().numpy().tobytes() == v.tobytes()


def test_smoothing_keeps_the_volume(fx):
    from swnerf import mesh
    v, f, _ = fx["sphere"]
    sm = mesh.smooth(dev(v), dev(f), iterations=10)
    before, after = mesh.measure(dev(v), dev(f)).volume, mesh.measure(sm, dev(f)).volume
    print(f"sphere(16): volume {before:.5f} -> {after:.5f} after 10 Taubin iterations")
    assert abs(before - 0.87754) < 1e-5 and abs(after - 0.87754) <= 0.02 * 0.87754             # the replay gives 0.88752: 1.1 %


# ------------------------------------------------------------------------------------------------------------------- normals
@pytest.mark.parametrize("name", ["two_spheres", "sphere", "torus", "noise", "floaters", "open_sphere", "fan", "unreferenced",
                                  "repeated_index", "large"])
def test_vertex_normals(fx, name):
    from swnerf import mesh
    v, f, mcn = fx[name]
    got = mesh.vertex_normals(dev(v), dev(f)).cpu().numpy()
    want = R.vertex_normals(v, f)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{name}: normals max |d| = {err:.3e}")
    assert got.dtype == np.float32 and err <= 2.0 ** -23
    unref = np.diff(ref(fx, name, "incidence")[0]) == 0
    assert (got[unref] == 0).all()
    if mcn is not None:
        assert float((got * mcn).sum(1).mean()) > 0                     # toward lower density, like the marching-cubes normals


# ------------------------------------------------------------------------------------------------------------------- measure
@pytest.mark.parametrize("name", ALL)
def test_measure(fx, name):
    from swnerf import mesh
    v, f, _ = fx[name]
    dv, df = dev(v), dev(f)
    values, counts = mesh.measure_raw(dv, df)
    again = mesh.measure_raw(dv, df, incidence=mesh.vertex_faces(df, len(v)))
    assert values.tobytes() == again[0].tobytes() and counts.tobytes() == again[1].tobytes()     # two runs: the same bits
    w = ref(fx, name, "measure")
    F = len(f)
    for q, what in enumerate(("area", "volume", "moment x", "moment y", "moment z")):
        bound = 2 * F * 2.0 ** -53 * math.fsum(np.abs(w["terms"][:, q]).tolist())
        err = abs(float(values[q]) - float(w["sums"][q]))
        print(f"{name}: {what} = {values[q]:.17g}, |d| = {err:.3e}, bound = {bound:.3e}")
        assert err <= bound, (name, what)
    assert (values[11:] == 0).all()
    m = mesh.measure(dv, df)
    if w["referenced_vertices"]:
        assert np.array_equal(m.bbox_min, w["bbox_min"]) and np.array_equal(m.bbox_max, w["bbox_max"])
        assert np.array_equal(m.extents, w["bbox_max"] - w["bbox_min"])
    else:
        assert m.bbox_min is None and m.bbox_max is None and m.extents is None
    for k in ("referenced_vertices", "edges", "boundary_edges", "nonmanifold_edges", "n_components", "euler", "closed"):
        assert m[k] == w[k], (name, k, m[k], w[k])
    assert m.area == float(values[0]) and m.volume == float(values[1])
    if name != "repeated_index":                                        # the helper has no notion of an edge (a, a)
        assert m.closed == M.is_closed_oriented_manifold(f)
    if w["referenced_vertices"] == len(v) and len(f):
        assert m.euler == M.euler_characteristic(len(v), f)
    if m.volume != 0:
        assert np.array_equal(m.centroid, values[2:5] / values[1])
    else:
        assert m.centroid is None


def test_measure_known_values_and_input_forms(fx, tmp_path):
    from swnerf import mesh
    v, f, n = fx["sphere"]
    m = mesh.Mesh(v, f, n).measure()
    assert abs(m.area - 4.45255) < 1e-5 and abs(m.volume - 0.87754) < 1e-5 and m.closed and m.euler == 2 and m.n_components == 1
    w = R.measure(v, f)["sums"]
    assert np.abs(m.centroid - w[2:5] / w[1]).max() < 1e-12 and np.abs(m.centroid).max() < 1e-4   # a centred sphere
    t = mesh.measure(fx["torus"][0], fx["torus"][1])
    assert t.euler == 0 and t.closed
    path = mesh.Mesh(v, f, n).export(str(tmp_path / "s.obj"))
    from_obj = mesh.measure(path)                                       # %.9g keeps every float32 exact
    assert all(np.array_equal(from_obj[k], m[k]) for k in m)
    assert mesh.measure((dev(v), dev(f), dev(n), None)).area == m.area


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_generate_mesh_with_clean(fx):
    from swnerf import mesh
    field, h = R.floater_field(20)
    (X, Y, Z), _ = M.grid(20)
    rng = np.random.default_rng(2)
    col = rng.random(field.shape + (3,)).astype(np.float32)
    raw = mesh.generate_mesh(field, col, (X, Y, Z), density_threshold=0.)
    none = mesh.generate_mesh(field, col, (X, Y, Z), density_threshold=0., clean=None)
    spacing, origin = mesh._grid_geometry((X, Y, Z))
    direct = mesh.marching_cubes(dev(field), 0., spacing, origin, dev(col))
    for a, b, c in zip((raw.vertices, raw.faces, raw.vertex_normals, raw.vertex_colors),
                       (none.vertices, none.faces, none.vertex_normals, none.vertex_colors), direct):
        assert a.tobytes() == b.tobytes() == c.cpu().numpy().tobytes()  # clean=None: exactly what the call returned before
    assert (len(raw.vertices), len(raw.faces)) == (482, 948)
    before = raw.measure()
    assert before.n_components == 4 and before.extents.max() > 1.5
    m = mesh.generate_mesh(field, col, (X, Y, Z), density_threshold=0., clean=True)
    after = m.measure()
    assert len(m.faces) == 812 and after.n_components == 1 and after.closed
    assert after.extents.max() <= 1.0 + 2 * h
    wl, wt = R.component_table(raw.faces, len(raw.vertices))
    wv, wf, wn, wc = R.compact(raw.vertices, raw.faces, wl, R.select(wt, 1)[:, 0], raw.vertex_normals, raw.vertex_colors)
    for a, b in ((m.vertices, wv), (m.faces, wf), (m.vertex_normals, wn), (m.vertex_colors, wc)):
        assert a.tobytes() == b.tobytes()                               # not smoothed: the marching-cubes normals are carried along
    s = mesh.generate_mesh(field, col, (X, Y, Z), density_threshold=0., clean={"smooth_iterations": 3, "keep": 2, "min_faces": 41})
    assert len(s.faces) == 812 + 56
    sv = R.smooth(*R.compact(raw.vertices, raw.faces, wl, R.select(wt, 2, 41)[:, 0])[:2], iterations=3)
    assert s.vertices.tobytes() == sv.tobytes()
    assert np.abs(s.vertex_normals.astype(np.float64) - R.vertex_normals(sv, s.faces)).max() <= 2.0 ** -23
    c = mesh.clean(raw, smooth_iterations=3, keep=2, min_faces=41)
    assert c.vertices.tobytes() == s.vertices.tobytes() and c.faces.tobytes() == s.faces.tobytes()


# --------------------------------------------------------------------------------------------------------------- bad indices
def test_bad_face_indices_raise_and_write_nothing_out_of_range(fx):
    from swnerf import _lib, mesh
    v, f, _ = fx["sphere"]
    V, F = len(v), len(f)
    bad = f.copy()
    bad[100, 1] = V
    bad[500, 2] = -1
    dv, db = dev(v), dev(bad)
    for call in (lambda: mesh.components(db, V), lambda: mesh.vertex_faces(db, V), lambda: mesh.keep_components(dv, db),
                 lambda: mesh.smooth(dv, db), lambda: mesh.vertex_normals(dv, db), lambda: mesh.measure(dv, db), lambda: mesh.clean((dv, db))):
        with pytest.raises(ValueError, match="2 face indices are outside"):
            call()
    L = _lib.lib()
    ws = torch.empty(L.swnerf_mesh_workspace_bytes(V, F), dtype=torch.uint8, device=DEV)
    st = _lib.stream_of(dv)
    vlabel = torch.full((V + 4,), -7, dtype=torch.int32, device=DEV)
    table = torch.full((V + 4, 3), -7, dtype=torch.int32, device=DEV)
    counts = torch.full((2 + 4,), -7, dtype=torch.int32, device=DEV)
    _lib.check(L.swnerf_mesh_components(_lib.ptr(db), V, F, _lib.ptr(ws), _lib.ptr(vlabel), _lib.ptr(table), _lib.ptr(counts), st), "mesh_components")
    assert counts.tolist() == [0, 2, -7, -7, -7, -7] and bool((vlabel[V:] == -7).all()) and bool((table == -7).all())
    offsets = torch.full((V + 1 + 4,), -7, dtype=torch.int32, device=DEV)
    items = torch.full((3 * F + 4,), -7, dtype=torch.int32, device=DEV)
    status = torch.full((1 + 4,), -7, dtype=torch.int32, device=DEV)
    _lib.check(L.swnerf_mesh_incidence(_lib.ptr(db), V, F, _lib.ptr(ws), _lib.ptr(offsets), _lib.ptr(items), _lib.ptr(status), st), "mesh_incidence")
    assert status.tolist() == [2, -7, -7, -7, -7] and bool((offsets[V + 1:] == -7).all()) and bool((items == -7).all())
    # measure on a valid incidence but bad faces: the status word stops it
    good = mesh.vertex_faces(dev(f), V)
    values = torch.full((16 + 4,), -7., dtype=torch.float64, device=DEV)
    cnt = torch.full((8 + 4,), -7, dtype=torch.int64, device=DEV)
    _lib.check(L.swnerf_mesh_measure(_lib.ptr(dv), _lib.ptr(db), _lib.ptr(good[0]), _lib.ptr(good[1]), V, F, _lib.ptr(ws), _lib.ptr(values),
                                     _lib.ptr(cnt), st), "mesh_measure")
    assert int(cnt[7]) == 2 and float(values[0]) == 0. and bool((values[16:] == -7).all()) and bool((cnt[8:] == -7).all())


def test_refused_sizes_and_arguments():
    from swnerf import _lib
    L = _lib.lib()
    t = torch.zeros(64, dtype=torch.int32, device=DEV)
    p = _lib.ptr(t)
    assert L.swnerf_mesh_components(p, 2 ** 31, 1, p, p, p, p, None) == _lib.E_ARG
    assert L.swnerf_mesh_incidence(p, 3, (2 ** 31 + 2) // 3, p, p, p, p, None) == _lib.E_ARG
    assert L.swnerf_mesh_smooth_step(p, p, p, p, 2, 1, 0.5, p, None) == _lib.E_ARG             # out == verts
    assert b"out must not be verts" in L.swnerf_last_error()
    assert L.swnerf_mesh_compact(p, p, None, None, p, 4, 2, p, 1, p, 5, 2, p, p, None, None, None) == _lib.E_ARG
