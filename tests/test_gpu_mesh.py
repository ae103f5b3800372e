"""Marching cubes on the MI355X (swnerf_mc_count / swnerf_mc_emit, swnerf.mesh.marching_cubes / generate_mesh / nerf_to_mesh)
against the numpy restatement of the contract (tests/mc_numpy.py): faces and colours bit-identical, vertices within 2 ulp,
normals within 1e-5; geometric invariants on larger grids; the reference's nearest-sample colour rule; the example."""
import os
import sys

import numpy as np
import pytest
import torch

import cases
import mc_numpy as M

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def mesh():
    import swnerf.mesh as mesh
    return mesh


def run_gpu(mesh, dev, f, level, spacing=(1., 1., 1.), origin=(0., 0., 0.), colors=None, ld=1):
    f = np.asarray(f, np.float32)
    if ld == 1:
        d = torch.from_numpy(f).to(dev)
        c = torch.from_numpy(np.asarray(colors, np.float32)).to(dev) if colors is not None else None
    else:
        q = torch.zeros(f.shape + (4,), dtype=torch.float32)
        q[..., 3] = torch.from_numpy(f)
        if colors is not None:
            q[..., :3] = torch.from_numpy(np.asarray(colors, np.float32))
        q = q.to(dev)
        d, c = q[..., 3], (q[..., :3] if colors is not None else None)
    out = mesh.marching_cubes(d, level, spacing, origin, c)
    torch.cuda.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in out)


def within_ulp(a, b, n=2):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    tol = n * np.spacing(np.maximum(np.abs(a), np.abs(b)))
    return bool((np.abs(a.astype(np.float64) - b.astype(np.float64)) <= tol).all())


def compare(mesh, dev, f, level, spacing=(1., 1., 1.), origin=(0., 0., 0.), with_colors=True, ld=1, seed=5):
    cols = np.random.default_rng(seed).uniform(-1, 2, f.shape + (3,)).astype(np.float32) if with_colors else None
    g = run_gpu(mesh, dev, f, level, spacing, origin, cols, ld)
    r = M.marching_cubes(f, level, spacing, origin, cols)
    assert g[0].shape == r[0].shape and g[1].shape == r[1].shape, (g[0].shape, r[0].shape, g[1].shape, r[1].shape)
    assert g[1].dtype == np.int32
    np.testing.assert_array_equal(g[1], r[1])
    assert within_ulp(g[0], r[0]), np.abs(g[0] - r[0]).max()
    np.testing.assert_allclose(g[2], r[2], atol=1e-5, rtol=0)
    if with_colors:
        np.testing.assert_array_equal(g[3], r[3])
    else:
        assert g[3] is None
    return g


FIELDS = {
    "sphere": lambda: (M.sphere(40), 0.0),
    "torus": lambda: (M.torus(48), 0.0),
    "two_spheres": lambda: (M.two_spheres(48), 0.0),
    "noise_padded": lambda: ((M.noise((20, 24, 18), 0), 1.0), 0.1),
    "noise_open": lambda: ((M.noise((30, 30, 32), 1, pad=False), 1.0), 0.0),
    "noise_17x33x9": lambda: ((M.noise((17, 33, 9), 2, pad=False), 1.0), -0.1),
}


@pytest.mark.parametrize("ld", [1, 4])
@pytest.mark.parametrize("name", sorted(FIELDS))
def test_matches_numpy_restatement(mesh, dev, name, ld):
    (f, h), level = FIELDS[name]()
    g = compare(mesh, dev, f, level, (h, h * 1.5, h * 0.75), (-1., 0.25, 3.), ld=ld)
    assert len(g[1]) > 0
    if name != "noise_open" and name != "noise_17x33x9":
        assert M.is_closed_oriented_manifold(g[1])


@pytest.mark.parametrize("ld", [1, 4])
def test_without_colours(mesh, dev, ld):
    f, h = M.sphere(24)
    compare(mesh, dev, f, 0.0, (h,) * 3, (-1.,) * 3, with_colors=False, ld=ld)


@pytest.mark.parametrize("ld", [1, 4])
def test_integer_field_ties(mesh, dev, ld):
    """f == level is outside: corners exactly at the level, t in {0, 1}, zero-area triangles kept"""
    f = np.random.default_rng(7).integers(0, 4, (13, 16, 11)).astype(np.float32)
    compare(mesh, dev, f, 2.0, ld=ld)
    compare(mesh, dev, f, 1.0, (0.5, 2., 1.), ld=ld)


@pytest.mark.parametrize("ld", [1, 4])
def test_non_finite_entries(mesh, dev, ld):
    f = M.noise((16, 12, 20), 3, pad=False)
    rng = np.random.default_rng(4)
    flat = f.ravel()
    for v in (np.nan, np.inf, -np.inf):
        flat[rng.choice(flat.size, 40, replace=False)] = v
    compare(mesh, dev, f, 0.0, ld=ld)


@pytest.mark.parametrize("ld", [1, 4])
def test_empty_surfaces(mesh, dev, ld):
    for f, level in ((np.zeros((9, 8, 7), np.float32), 1.0), (np.ones((9, 8, 7), np.float32), 0.0),
                     (np.zeros((2, 2, 2), np.float32), 0.0)):
        g = run_gpu(mesh, dev, f, level, colors=np.zeros(f.shape + (3,), np.float32), ld=ld)
        assert g[0].shape == (0, 3) and g[1].shape == (0, 3) and g[2].shape == (0, 3) and g[3].shape == (0, 3)


@pytest.mark.parametrize("pct", [10, 50, 90])
def test_reference_density_field(mesh, dev, golden, pct):
    """G10: the density field the reference's sample_grid made (6^3, seeded fine net) at its percentiles"""
    ref = golden("g10_mesh_query")
    dens = ref["density"]
    level = float(np.float32(np.percentile(dens, pct)))
    ax = [np.linspace(b[0], b[1], cases.G10_RES) for b in cases.G10_BOUNDS]
    spacing = tuple(float(a[1] - a[0]) for a in ax)
    origin = tuple(float(a[0]) for a in ax)
    for ld in (1, 4):
        g = run_gpu(mesh, dev, dens, level, spacing, origin, ref["color"], ld)
        r = M.marching_cubes(dens.astype(np.float32), level, spacing, origin, ref["color"].astype(np.float32))
        np.testing.assert_array_equal(g[1], r[1])
        assert len(g[1]) > 0 and within_ulp(g[0], r[0])
        np.testing.assert_allclose(g[2], r[2], atol=1e-5)
        np.testing.assert_array_equal(g[3], r[3])
    xyz = np.meshgrid(*ax, indexing="ij")
    assert np.array_equal(xyz[0], ref["X"])
    m = mesh.generate_mesh(dens, ref["color"], xyz, density_threshold=level)
    np.testing.assert_array_equal(m.faces, r[1])
    np.testing.assert_array_equal(m.vertex_colors, r[3])


def test_large_noise_is_closed_and_deterministic(mesh, dev):
    f = M.noise((126, 126, 126), 11)                     # padded: 128^3, the vectorised path
    level = 0.05
    a = run_gpu(mesh, dev, f, level)
    b = run_gpu(mesh, dev, f, level)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y, equal_nan=True)
    assert len(a[1]) > 100000 and M.is_closed_oriented_manifold(a[1])
    chi = M.euler_characteristic(len(a[0]), a[1])
    assert chi % 2 == 0
    r = M.marching_cubes(f, level)
    np.testing.assert_array_equal(a[1], r[1])
    assert within_ulp(a[0], r[0])


def test_sphere_geometry_on_gpu(mesh, dev):
    f, h = M.sphere(64, r=0.6)
    v, fa, n, _ = run_gpu(mesh, dev, f, 0.0, (h,) * 3, (-1.,) * 3)
    area, vol = M.area_volume(v, fa)
    assert abs(area / (4 * np.pi * 0.36) - 1) < 0.01 and vol > 0 and abs(vol / (4 / 3 * np.pi * 0.216) - 1) < 0.01
    assert M.is_closed_oriented_manifold(fa) and M.euler_characteristic(len(v), fa) == 2


def test_bad_arguments_raise(mesh, dev):
    for shape in ((1, 5, 5), (5, 1, 5), (5, 5, 1)):
        with pytest.raises(ValueError):
            mesh.marching_cubes(torch.zeros(shape, device=dev), 0.0)
    from swnerf import _lib
    L = _lib.lib()
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
    tot = torch.zeros(2, dtype=torch.int64, device=dev)
    x = torch.zeros(64, device=dev)
    st = _lib.stream_of(x)
    assert L.swnerf_mc_count(_lib.ptr(x), 4, 4, 1, 1, 0.0, _lib.ptr(ws), _lib.ptr(tot), st) != 0
    assert b">= 2" in L.swnerf_last_error()
    assert L.swnerf_mc_count(_lib.ptr(x), 4, 4, 4, 0, 0.0, _lib.ptr(ws), _lib.ptr(tot), st) != 0
    assert L.swnerf_mc_workspace_bytes(1, 4, 4) == 0
    import ctypes
    f3 = (ctypes.c_float * 3)(1, 1, 1)
    p = _lib.ptr(x)
    assert L.swnerf_mc_emit(p, None, 4, 4, 4, 1, 0, 0.0, f3, f3, _lib.ptr(ws), 1 << 31, 0, p, p, p, None, st) != 0
    assert b"int32" in L.swnerf_last_error()


@pytest.fixture(scope="module")
def fine_net(dev):
    from swnerf import synth, model
    m = model.vallina_NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.nerf_state_dict(*synth.NET_FINE[:1], alpha_bias=synth.NET_FINE[1]).items()})
    return m.to(dev).eval()


def reference_colours(verts, color_field, xyz):
    """extract_mesh.py:116-121, vectorised: per axis the argmin of |coordinate - vertex| (ties to the lower index)"""
    X, Y, Z = xyz
    ax = [X[:, 0, 0], Y[0, :, 0], Z[0, 0, :]]
    v = np.asarray(verts, np.float64)
    idx = [np.argmin(np.abs(ax[b][None, :] - v[:, b:b + 1]), axis=1) for b in range(3)]
    return color_field[idx[0], idx[1], idx[2]]


def test_nerf_to_mesh_and_reference_colours(mesh, dev, fine_net):
    R, level = 48, 0.5
    with torch.no_grad():
        m = mesh.nerf_to_mesh(fine_net, cases.G10_BOUNDS, resolution=R, density_threshold=level, num_views=8)
        dens, col, xyz = mesh.sample_grid(cases.G10_BOUNDS, R, fine_net, num_views=8)
    g = mesh.generate_mesh(dens, col, xyz, density_threshold=level)
    assert len(m.faces) > 1000
    for a, b in ((m.vertices, g.vertices), (m.faces, g.faces), (m.vertex_normals, g.vertex_normals), (m.vertex_colors, g.vertex_colors)):
        np.testing.assert_array_equal(a, b)
    q = mesh.sample_grid(cases.G10_BOUNDS, R, fine_net, num_views=8, on_device=True)
    assert q.shape == (R, R, R, 4) and q.dtype == torch.float32 and q.is_cuda
    np.testing.assert_array_equal(q[..., 3].cpu().numpy().astype(np.float64), dens)
    # the reference's nearest-sample colours; only vertices with t within 1e-6 of 0.5 may differ
    spacing, origin = mesh._grid_geometry(xyz)
    _, _, _, _, t = M.marching_cubes(dens.astype(np.float32), level, spacing, origin, col.astype(np.float32), return_t=True)
    refc = reference_colours(g.vertices, col, xyz).astype(np.float32)
    diff = (refc != g.vertex_colors).any(1)
    assert not (diff & (np.abs(t - 0.5) >= 1e-6)).any(), int((diff & (np.abs(t - 0.5) >= 1e-6)).sum())
    assert diff.sum() <= max(3, len(t) // 1000)


def test_example_writes_a_manifold_obj(mesh, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import extract_mesh_lego_like as ex
    path = ex.main(str(tmp_path), resolution=40, num_views=8)
    v, f, n, c = mesh.load_obj(path)
    assert len(f) > 1000 and c is not None and c.min() >= 0 and c.max() <= 1
    e = M.directed_edges(f)
    key = e[:, 0].astype(np.int64) * len(v) + e[:, 1]
    assert np.unique(key).size == key.size                 # oriented 2-manifold (with boundary where it meets the grid)
    assert np.unique(f).size == len(v)
