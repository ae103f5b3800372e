"""The fused grid query of the time-conditioned nets at one frame time (swnerf_query_points_time, swnerf.mesh.query_points /
sample_grid / nerf_to_mesh / mesh_sequence with frame_time) on the MI355X: against float64, against the reference's outputs
(g17_dynamic_query.npz), against the op path, chunking, the zero_canonical branch, mesh_sequence and the example.

Tolerances.  D-NeRF (test_gpu_parity.py's): dx atol 1e-6; raw at t = 0.5 atol 1e-3, rtol 1e-4 (gamma(x + dx) amplifies a 2e-7
rounding of dx by 2^9); raw at t = 0 with zero_canonical atol 1e-4, rtol 1e-4.  T-NeRF (test_gpu_tnerf.py's raw bound):
|diff| - 1e-4 |ref| < 2e-4."""
import os
import sys

import numpy as np
import pytest
import torch

import cases
import cases_tnerf
import tnerf_ref
from oracle import nerf_oracle as O

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZES = (1, 31, 32, 33, 127, 128, 129, 161)          # the tile (32), wave and workgroup (128) edges
MMAX, VMAX = max(SIZES), 3
TIMES = (0.0, 0.5)


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module")
def mesh():
    import swnerf.mesh as mesh
    return mesh


@pytest.fixture(scope="module")
def dn():
    from swnerf import model, embedder
    e10, _ = embedder.get_embedder(10, 3, 0)
    m = model.NeRF.get_by_name("direct_temporal", D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27,
                               input_ch_time=21, use_viewdirs=True, embed_fn=e10, zero_canonical=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in cases.weights_dnerf().items()})
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def tn():
    from swnerf.model import TNeRF
    m = TNeRF(**cases_tnerf.NET)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in cases_tnerf.weights().items()}, strict=True)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def inputs(mesh):
    """MMAX seeded points inside the G10 bounds and VMAX spiral directions; every smaller case takes their leading rows"""
    rng = np.random.default_rng(171)
    lo, hi = np.array([b[0] for b in cases.G10_BOUNDS]), np.array([b[1] for b in cases.G10_BOUNDS])
    pts = rng.uniform(lo, hi, (MMAX, 3)).astype(np.float32)
    dirs = mesh.generate_viewdirs(VMAX).astype(np.float32)
    return torch.from_numpy(pts), torch.from_numpy(dirs)


def _embed64(x, L):
    """gamma(x) in float64 of the float32 values x (x * 2^k is exact in float32, so this is what the kernels approximate)"""
    x = x.double()
    out = [x]
    for k in range(L):
        out += [torch.sin(x * float(2 ** k)), torch.cos(x * float(2 ** k))]
    return torch.cat(out, -1)


@pytest.fixture(scope="module")
def ref64(inputs):
    """{(net, t): (raw [VMAX, MMAX, 4] float64, dx [MMAX, 3] or None)} - computed once on the CPU, never modified"""
    pts, dirs = inputs
    with torch.no_grad():
        sd_d = {k: torch.from_numpy(v).double() for k, v in cases.weights_dnerf().items()}
        sd_t = {k: torch.from_numpy(v).double() for k, v in cases_tnerf.weights().items()}
        out = {}
        for t in TIMES:
            te = _embed64(torch.full((MMAX, 1), t), 10)
            raws, traws, dx = [], [], None
            for v in range(VMAX):
                ed = _embed64(dirs[v][None].expand(MMAX, 3), 4)
                o, dx = O.dnerf_mlp(sd_d, torch.cat([_embed64(pts, 10), ed], -1), te)
                raws.append(o)
                traws.append(tnerf_ref.forward(sd_t, torch.cat([_embed64(pts, 10), ed], -1), ed, te))
            out[("dnerf", t)] = (torch.stack(raws), dx)
            out[("tnerf", t)] = (torch.stack(traws), None)
    return out


def _dnerf_close(got, ref, t, what):
    atol = 1e-3 if t else 1e-4
    d = (got.double().cpu() - ref).abs()
    print(f"{what}: max |diff| {float(d.max()):.3e} (atol {atol}, rtol 1e-4)")
    assert bool((d <= atol + 1e-4 * ref.abs()).all()), (what, float((d - 1e-4 * ref.abs()).max()))


def _tnerf_close(got, ref, what):
    d = (got.double().cpu() - ref).abs() - 1e-4 * ref.abs()
    print(f"{what}: max(|diff| - 1e-4 |ref|) {float(d.max()):.3e} (< 2e-4)")
    assert float(d.max()) < 2e-4, what


def _expected(raw, V):
    """[M,4] = [mean over the first V directions of rgb, sigma] from raw [VMAX, M, 4]"""
    return torch.cat([raw[:V, :, :3].mean(0), raw[0, :, 3:]], -1)


# ---- 1. against float64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TIMES)
@pytest.mark.parametrize("V", (1, 3))
def test_dnerf_query_against_float64(mesh, dn, inputs, ref64, V, t):
    pts, dirs = (a.to(DEV) for a in inputs)
    raw, dx = ref64[("dnerf", t)]
    for M in SIZES:
        out, gdx = mesh.query_points(dn, pts[:M], dirs[:V], shared_dirs=True, frame_time=t, return_dx=True)
        assert out.shape == (M, 4) and gdx.shape == (M, 3)
        ddx = float((gdx.double().cpu() - dx[:M]).abs().max())
        print(f"dnerf M={M} V={V} t={t}: max |d dx| {ddx:.3e} (atol 1e-6)")
        assert ddx <= 1e-6
        _dnerf_close(out, _expected(raw[:, :M], V), t, f"dnerf M={M} V={V} t={t} out")
    if t == 0:
        assert float(gdx.abs().max()) == 0.0


@pytest.mark.parametrize("t", TIMES)
@pytest.mark.parametrize("V", (1, 3))
def test_tnerf_query_against_float64(mesh, tn, inputs, ref64, V, t):
    pts, dirs = (a.to(DEV) for a in inputs)
    raw, _ = ref64[("tnerf", t)]
    for M in SIZES:
        out = mesh.query_points(tn, pts[:M], dirs[:V], shared_dirs=True, frame_time=t)
        assert out.shape == (M, 4)
        _tnerf_close(out, _expected(raw[:, :M], V), f"tnerf M={M} V={V} t={t} out")


# ---- 2. against the reference's own outputs, through sample_grid ------------------------------------------------------------------
@pytest.mark.parametrize("tag,t", (("t0", 0.0), ("t5", 0.5)))
def test_sample_grid_against_g17(mesh, dn, tn, golden, tag, t):
    ref = golden("g17_dynamic_query")
    R = cases.G10_RES
    dens, col, _ = mesh.sample_grid(cases.G10_BOUNDS, R, dn, num_views=cases.G10_VIEWS, frame_time=t)
    assert dens.shape == (R, R, R) and col.shape == (R, R, R, 3) and dens.dtype == np.float64
    got = torch.from_numpy(np.concatenate([col.reshape(-1, 3), dens.reshape(-1, 1)], -1))
    want = torch.from_numpy(np.concatenate([ref[f"dnerf_{tag}_mean"], ref[f"dnerf_{tag}_sigma"][:, None].astype(np.float64)], -1))
    _dnerf_close(got, want, t, f"dnerf sample_grid {tag}")
    ax = [np.linspace(b[0], b[1], R) for b in cases.G10_BOUNDS]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    pts = torch.tensor(np.stack([X.ravel(), Y.ravel(), Z.ravel()], -1), dtype=torch.float32, device=DEV)
    dirs = torch.tensor(mesh.generate_viewdirs(cases.G10_VIEWS), dtype=torch.float32, device=DEV)
    _, dx = mesh.query_points(dn, pts, dirs, frame_time=t, return_dx=True)
    ddx = float(np.abs(dx.cpu().numpy() - ref[f"dnerf_{tag}_dx"]).max())
    print(f"dnerf {tag}: max |d dx| {ddx:.3e} (atol 1e-6)")
    assert ddx <= 1e-6
    dens, col, _ = mesh.sample_grid(cases.G10_BOUNDS, R, tn, num_views=cases.G10_VIEWS, frame_time=t)
    got = torch.from_numpy(np.concatenate([col.reshape(-1, 3), dens.reshape(-1, 1)], -1))
    want = torch.from_numpy(np.concatenate([ref[f"tnerf_{tag}_mean"], ref[f"tnerf_{tag}_sigma"][:, None].astype(np.float64)], -1))
    _tnerf_close(got, want, f"tnerf sample_grid {tag}")


# ---- 3. fused against the op path --------------------------------------------------------------------------------------------------
def _op_path_dnerf(dn, pts, dirs_rows, t):
    """render_dnerf.run_network on host-embedded rows, one direction per point: swnerf_embed + swnerf_mlp_forward"""
    from swnerf import render_dnerf, embedder
    e10, e4, et = embedder.get_embedder(10, 3, 0)[0], embedder.get_embedder(4, 3, 0)[0], embedder.get_embedder(10, 1, 0)[0]
    M = pts.shape[0]
    out, dx = render_dnerf.run_network(pts[:, None], dirs_rows, torch.full((M, 1), t, device=pts.device), dn, e10, e4, et)
    return out[:, 0], dx[:, 0]


@pytest.mark.parametrize("t", TIMES)
def test_dnerf_fused_against_the_op_path(mesh, dn, inputs, t):
    pts, dirs = (a.to(DEV) for a in inputs)
    M = 129
    per, per_dx = [], []
    for v in range(VMAX):
        rows = dirs[v:v + 1].expand(M, 3).contiguous()
        o_op, dx_op = _op_path_dnerf(dn, pts[:M], rows, t)
        o_f, dx_f = mesh.query_points(dn, pts[:M], rows, shared_dirs=False, frame_time=t, return_dx=True)
        # the TIME tile (once per wave) and the in-line TIME segment add in the same order: the same bits
        assert torch.equal(dx_f, dx_op), float((dx_f - dx_op).abs().max())
        assert torch.equal(o_f[:, 3], o_op[:, 3]), float((o_f[:, 3] - o_op[:, 3]).abs().max())
        _dnerf_close(o_f, o_op.double().cpu(), t, f"dnerf per-point rgb vs op path, direction {v}")
        per.append(o_f)
        per_dx.append(dx_f)
    shared, sdx = mesh.query_points(dn, pts[:M], dirs, shared_dirs=True, frame_time=t, return_dx=True)
    assert torch.equal(shared[:, 3], per[0][:, 3]) and torch.equal(sdx, per_dx[0])
    d = float((shared[:, :3] - torch.stack(per)[..., :3].mean(0)).abs().max())
    print(f"dnerf t={t}: shared rgb vs mean of per-point calls {d:.3e} (1e-5)")
    assert d <= 1e-5
    with pytest.raises(RuntimeError, match="one per point"):
        mesh.query_points(dn, pts[:10], dirs, shared_dirs=False, frame_time=t)
    assert mesh.query_points(dn, pts[:0], dirs, shared_dirs=True, frame_time=t).shape == (0, 4)


@pytest.mark.parametrize("t", TIMES)
def test_tnerf_fused_against_the_op_path(mesh, tn, inputs, t):
    """per-point directions take the op path (embedders, TNeRF.forward on the generic GEMMs): the fused shared-direction launch
    agrees with it within the T-NeRF bound, and with the mean of V such calls"""
    pts, dirs = (a.to(DEV) for a in inputs)
    M = 129
    per = torch.stack([mesh.query_points(tn, pts[:M], dirs[v:v + 1].expand(M, 3).contiguous(), shared_dirs=False, frame_time=t)
                       for v in range(VMAX)])
    assert per.shape == (VMAX, M, 4)
    one = mesh.query_points(tn, pts[:M], dirs[:1], shared_dirs=True, frame_time=t)
    _tnerf_close(one, per[0].double().cpu(), f"tnerf t={t} fused V=1 vs op path")
    shared = mesh.query_points(tn, pts[:M], dirs, shared_dirs=True, frame_time=t)
    _tnerf_close(shared, _expected(per.double().cpu(), VMAX), f"tnerf t={t} fused V=3 vs mean of op-path calls")
    assert torch.equal(shared[:, 3], one[:, 3])                    # the density does not depend on the directions
    assert mesh.query_points(tn, pts[:0], dirs, shared_dirs=True, frame_time=t).shape == (0, 4)
    assert mesh.query_points(tn, pts[:M], dirs, shared_dirs=True, frame_time=torch.full((M, 1), t, device=DEV)).equal(shared)


# ---- 4. chunked calls --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("dnerf", "tnerf"))
def test_chunks_give_the_bits_of_one_launch(mesh, dn, tn, inputs, kind):
    pts, dirs = (a.to(DEV) for a in inputs)
    net = dn if kind == "dnerf" else tn
    for t in TIMES:
        whole = mesh.query_points(net, pts, dirs, shared_dirs=True, frame_time=t)
        parts = torch.cat([mesh.query_points(net, pts[i:i + 64], dirs, shared_dirs=True, frame_time=t) for i in range(0, MMAX, 64)])
        assert torch.equal(parts, whole), (kind, t)
    if kind == "dnerf":
        dx = mesh.query_points(dn, pts, dirs, frame_time=0.5, return_dx=True)[1]
        dxp = torch.cat([mesh.query_points(dn, pts[i:i + 64], dirs, frame_time=0.5, return_dx=True)[1] for i in range(0, MMAX, 64)])
        assert torch.equal(dx, dxp)


# ---- 5. zero_canonical -------------------------------------------------------------------------------------------------------------
def test_zero_canonical_at_time_zero_is_the_static_query(mesh, dn, inputs):
    pts, dirs = (a.to(DEV) for a in inputs)
    out, dx = mesh.query_points(dn, pts, dirs, shared_dirs=True, frame_time=0.0, return_dx=True)
    assert float(dx.abs().max()) == 0.0 and dx.shape == (MMAX, 3)
    assert torch.equal(out, mesh.query_points(dn._occ, pts, dirs, shared_dirs=True))
    rows = dirs[1:2].expand(MMAX, 3).contiguous()
    assert torch.equal(mesh.query_points(dn, pts, rows, shared_dirs=False, frame_time=0.0), mesh.query_points(dn._occ, pts, rows, shared_dirs=False))
    # a net that deforms at t = 0 too (zero_canonical off) does not take that branch
    dn.zero_canonical = False
    try:
        out2, dx2 = mesh.query_points(dn, pts, dirs, shared_dirs=True, frame_time=0.0, return_dx=True)
    finally:
        dn.zero_canonical = True
    assert float(dx2.abs().max()) > 1e-3 and not torch.equal(out2, out)


# ---- 6. mesh_sequence --------------------------------------------------------------------------------------------------------------
def test_mesh_sequence(mesh, dn, tmp_path):
    R, V, times = 24, 8, (0.0, 0.5)
    dens0, _, _ = mesh.sample_grid(cases.G10_BOUNDS, R, dn, num_views=V, frame_time=0.0)
    level = float(np.percentile(dens0, 70))
    seq = mesh.mesh_sequence(dn, cases.G10_BOUNDS, times, resolution=R, density_threshold=level, num_views=V, out_dir=str(tmp_path / "seq"))
    assert len(seq) == 2
    for i, (t, m) in enumerate(zip(times, seq)):
        assert len(m.faces) > 0
        dens, col, xyz = mesh.sample_grid(cases.G10_BOUNDS, R, dn, num_views=V, frame_time=t)
        g = mesh.generate_mesh(dens, col, xyz, density_threshold=level)
        for a, b in ((m.vertices, g.vertices), (m.faces, g.faces), (m.vertex_normals, g.vertex_normals), (m.vertex_colors, g.vertex_colors)):
            np.testing.assert_array_equal(a, b)
        n2m = mesh.nerf_to_mesh(dn, cases.G10_BOUNDS, resolution=R, density_threshold=level, num_views=V, frame_time=t)
        np.testing.assert_array_equal(n2m.vertices, m.vertices)
        np.testing.assert_array_equal(n2m.faces, m.faces)
        v, f, n, c = mesh.load_obj(str(tmp_path / "seq" / f"mesh_{i:03d}.obj"))
        np.testing.assert_array_equal(v, m.vertices)
        np.testing.assert_array_equal(f, m.faces)
        np.testing.assert_array_equal(n, m.vertex_normals)
        np.testing.assert_array_equal(c, np.clip(m.vertex_colors, 0, 1))
    assert not np.array_equal(seq[0].vertices, seq[1].vertices)    # the surface moved
    assert mesh.mesh_sequence(dn, cases.G10_BOUNDS, (), resolution=R) == []


# ---- 7. the example ----------------------------------------------------------------------------------------------------------------
def test_example_writes_three_objs(mesh, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import extract_mesh_dnerf_like as ex
    paths = ex.main(str(tmp_path), resolution=24, num_views=8)
    assert len(paths) == 3 and len(set(paths)) == 3
    for p in paths:
        v, f, n, c = mesh.load_obj(p)
        assert len(f) > 0 and len(v) > 0 and n.shape == v.shape and c is not None and c.min() >= 0 and c.max() <= 1
        assert f.min() >= 0 and f.max() < len(v)
