"""The grid query of the time-conditioned nets at one frame time, without a GPU: the CPU restatements (oracle run_network_dnerf,
tests/tnerf_ref.forward) against the reference's own outputs (g17_dynamic_query.npz, tests/golden/make_golden_dynamic_query.py), the
export and every refusal of swnerf_query_points_time (argument checks run before any device call), and the refusals of
swnerf.mesh.query_points."""
import numpy as np
import pytest
import torch

import cases
import cases_tnerf
import tnerf_ref
from oracle import nerf_oracle as O

E_ARG, E_UNSUPP = -1, -2
DNERF, TNERF = 1, 3
TIMES = {"t0": 0.0, "t5": 0.5}
ATOL, RTOL = 2e-6, 1e-5                      # test_oracle_golden.py's G10 rows


@pytest.fixture(scope="module")
def grid():
    from swnerf import mesh
    ax = [np.linspace(b[0], b[1], cases.G10_RES) for b in cases.G10_BOUNDS]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    pts = np.stack([X.ravel(), Y.ravel(), Z.ravel()], -1).astype(np.float32)
    vd = mesh.generate_viewdirs(cases.G10_VIEWS).astype(np.float32)
    return pts, vd


def test_g17_inputs_are_the_seeded_ones(golden, grid):
    ref = golden("g17_dynamic_query")
    sd_d, sd_t = cases.weights_dnerf(), cases_tnerf.weights()
    crc = cases.checksum(grid[0], grid[1], np.array(list(TIMES.values())), *[sd_d[k] for k in sorted(sd_d)], *[sd_t[k] for k in sorted(sd_t)])
    assert int(ref["crc"][0]) == int(crc[0])
    M, V = len(grid[0]), len(grid[1])
    for tag in TIMES:
        assert ref[f"dnerf_{tag}_raw"].shape == (V, M, 4) and ref[f"tnerf_{tag}_raw"].shape == (V, M, 4) == ref[f"tnerf_{tag}_raw_f32"].shape
        assert ref[f"dnerf_{tag}_dx"].shape == (M, 3)
    assert not ref["dnerf_t0_dx"].any() and np.abs(ref["dnerf_t5_dx"]).max() > 0.01          # zero_canonical at t = 0; a real deformation at 0.5


@pytest.mark.parametrize("tag", sorted(TIMES))
def test_oracle_dnerf_query_reproduces_g17(golden, grid, tag):
    ref = golden("g17_dynamic_query")
    pts, vd = (torch.from_numpy(a) for a in grid)
    sd = O.to_torch_sd(cases.weights_dnerf())
    M = pts.shape[0]
    ft = torch.full((M, 1), TIMES[tag])
    with torch.no_grad():
        for v in range(vd.shape[0]):
            out, dx = O.run_network_dnerf(sd, pts[:, None], vd[v][None].expand(M, 3), ft)
            np.testing.assert_allclose(out[:, 0].numpy(), ref[f"dnerf_{tag}_raw"][v], atol=ATOL, rtol=RTOL)
            np.testing.assert_allclose(dx[:, 0].numpy(), ref[f"dnerf_{tag}_dx"], atol=ATOL, rtol=RTOL)
    np.testing.assert_allclose(ref[f"dnerf_{tag}_raw"][..., :3].astype(np.float64).mean(0), ref[f"dnerf_{tag}_mean"], atol=0, rtol=0)
    np.testing.assert_array_equal(ref[f"dnerf_{tag}_raw"][0][:, 3], ref[f"dnerf_{tag}_sigma"])


@pytest.mark.parametrize("tag", sorted(TIMES))
def test_tnerf_ref_query_reproduces_g17(golden, grid, tag):
    """g17 records the reference's TNeRF twice (make_golden_dynamic_query.py): with float64 parameters on the runner's float32
    encodings - exactly what tnerf_ref.forward restates, compared at the G10 rows' tolerance - and in the runner's own float32,
    which lies within test_tnerf_host.py's bound for that pair (atol 1e-5: 8 layers of float32 rounding, measured 6.6e-6)."""
    ref = golden("g17_dynamic_query")
    pts, vd = (torch.from_numpy(a) for a in grid)
    sd = {k: torch.from_numpy(v).double() for k, v in cases_tnerf.weights().items()}
    M = pts.shape[0]
    ep, et = tnerf_ref.embed(pts, 10), tnerf_ref.embed(torch.full((M, 1), TIMES[tag]), 10)
    outs = []
    with torch.no_grad():
        for v in range(vd.shape[0]):
            ed = tnerf_ref.embed(vd[v][None].expand(M, 3), 4)
            outs.append(tnerf_ref.forward(sd, torch.cat([ep, ed], -1), ed, et).numpy())
            print(f"tnerf {tag} direction {v}: max |tnerf_ref - reference (float64)| = {np.abs(outs[-1] - ref[f'tnerf_{tag}_raw'][v]).max():.3e}")
    assert ref[f"tnerf_{tag}_raw"].dtype == np.float64 and ref[f"tnerf_{tag}_raw_f32"].dtype == np.float32
    np.testing.assert_allclose(np.stack(outs), ref[f"tnerf_{tag}_raw"], atol=ATOL, rtol=RTOL)
    np.testing.assert_allclose(ref[f"tnerf_{tag}_raw_f32"], ref[f"tnerf_{tag}_raw"], atol=1e-5, rtol=0)
    np.testing.assert_array_equal(ref[f"tnerf_{tag}_raw"][..., :3].mean(0), ref[f"tnerf_{tag}_mean"])
    np.testing.assert_array_equal(ref[f"tnerf_{tag}_raw"][0][:, 3], ref[f"tnerf_{tag}_sigma"])


# ---- the C ABI: export and refusals (pointers are never dereferenced: every call below is rejected, or has nothing to do, first)
@pytest.fixture(scope="module")
def L():
    from swnerf import _lib
    assert "swnerf_query_points_time" in _lib.EXPORTS
    return _lib.lib()


def _call(L, **change):
    a = dict(kind=DNERF, packed=8, pts=8, M=4, dirs=8, n_dirs=3, shared=1, t=0.5, run_deform=1, Lp=10, Ld=4, Lt=10, out=8, dx=None)
    a.update(change)
    rc = L.swnerf_query_points_time(a["kind"], a["packed"], a["pts"], a["M"], a["dirs"], a["n_dirs"], a["shared"], a["t"], a["run_deform"],
                                    a["Lp"], a["Ld"], a["Lt"], a["out"], a["dx"], None)
    return rc, L.swnerf_last_error()


REFUSALS = [
    (dict(kind=0), E_ARG, b"net kind 0 has no frame time"), (dict(kind=2), E_ARG, b"net kind 2"), (dict(kind=7), E_ARG, b"net kind 7"),
    (dict(packed=None), E_ARG, b"NULL pointer or negative M"), (dict(pts=None), E_ARG, b"NULL pointer or negative M"),
    (dict(dirs=None), E_ARG, b"NULL pointer or negative M"), (dict(out=None), E_ARG, b"NULL pointer or negative M"),
    (dict(M=-1), E_ARG, b"NULL pointer or negative M"), (dict(M=0, packed=None), E_ARG, b"NULL pointer or negative M"),
    (dict(Lp=11), E_UNSUPP, b"embedder bands (11,4,10) exceed (10,4,10)"), (dict(Ld=5), E_UNSUPP, b"exceed (10,4,10)"),
    (dict(Lt=11), E_UNSUPP, b"exceed (10,4,10)"), (dict(Lp=-1), E_UNSUPP, b"exceed (10,4,10)"),
    (dict(n_dirs=0), E_ARG, b"need >= 1 shared directions, got 0 for 4 points"),
    (dict(shared=0, n_dirs=3), E_ARG, b"need one per point directions, got 3 for 4 points"),
    (dict(kind=TNERF, shared=0, n_dirs=4), E_UNSUPP, b"shared directions only"),
    (dict(kind=TNERF, dx=8), E_ARG, b"T-NeRF has no position_delta output"),
    (dict(kind=TNERF, Ld=0), E_UNSUPP, b"T-NeRF needs view directions"),
    (dict(kind=TNERF, n_dirs=0), E_ARG, b"need >= 1 shared directions"),
    (dict(kind=TNERF, packed=None), E_ARG, b"NULL pointer or negative M"),
]


@pytest.mark.parametrize("change,code,text", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _, _ in REFUSALS])
def test_query_points_time_refusals_without_gpu(L, change, code, text):
    rc, msg = _call(L, **change)
    assert rc == code and text in msg and msg.startswith(b"query_points_time: "), (rc, msg)


@pytest.mark.parametrize("kind", [DNERF, TNERF])
def test_query_points_time_of_no_points_is_a_no_op(L, kind):
    assert _call(L, kind=kind, M=0)[0] == 0
    assert _call(L, kind=kind, M=0, pts=None, dirs=None, out=None)[0] == 0          # empty tensors have NULL data pointers


# ---- swnerf.mesh.query_points: refusals that need neither the GPU nor a packed blob
@pytest.fixture(scope="module")
def nets():
    from swnerf import model
    static = model.vallina_NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
    dn = model.DirectTemporalNeRF(D=8, W=256, input_ch=63, input_ch_views=27, input_ch_time=21, output_ch=5, skips=[4], use_viewdirs=True)
    tn = model.TNeRF(**cases_tnerf.NET)
    return static, dn, tn


def test_query_points_python_refusals(nets):
    from swnerf import mesh
    static, dn, tn = nets
    pts, dirs = torch.zeros(4, 3), torch.tensor([[0., 0., 1.]])
    with pytest.raises(ValueError, match="static net takes no frame_time"):
        mesh.query_points(static, pts, dirs, frame_time=0.5)
    for net in (dn, tn):
        with pytest.raises(NotImplementedError, match="frame_time"):
            mesh.query_points(net, pts, dirs)
        with pytest.raises(ValueError, match="Only accepts all points from same time"):
            mesh.query_points(net, pts, dirs, frame_time=torch.tensor([0.5, 0.5, 0.25, 0.5]))
    with pytest.raises(ValueError, match="return_dx"):
        mesh.query_points(tn, pts, dirs, frame_time=0.5, return_dx=True)
    with pytest.raises(ValueError, match="return_dx"):
        mesh.query_points(static, pts, dirs, return_dx=True)
    assert mesh._single_time(torch.full((7, 1), 0.25)) == 0.25 and mesh._single_time(0.5) == 0.5
    assert mesh._single_time(0.1) == float(np.float32(0.1))                         # as the kernels read it


def test_mesh_sequence_and_frame_time_signatures():
    import inspect
    from swnerf import mesh
    assert list(inspect.signature(mesh.mesh_sequence).parameters) == ["net", "bounds", "times", "resolution", "density_threshold", "num_views",
                                                                      "out_dir", "basename"]
    assert inspect.signature(mesh.mesh_sequence).parameters["basename"].default == "mesh_{:03d}.obj"
    for fn in (mesh.query_points, mesh.sample_grid, mesh.nerf_to_mesh):
        assert inspect.signature(fn).parameters["frame_time"].default is None
    # an injected two-argument query never sees the time
    seen = []
    q = lambda p, d: (seen.append((p.shape, d.shape)), torch.zeros(p.shape[0], 4))[1]
    dens, col, _ = mesh.sample_grid(cases.G10_BOUNDS, 3, None, num_views=2, query=q, frame_time=0.5, sharded=False)
    assert dens.shape == (3, 3, 3) and col.shape == (3, 3, 3, 3) and seen == [((27, 3), (2, 3))]
