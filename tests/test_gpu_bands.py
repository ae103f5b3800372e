"""The fused passes at embedder band counts other than (10, 4, 10).

Every fused entry point takes (L_pos, L_dir, L_time) at run time and accepts 0..10 / 0..4 (T-NeRF 1..4) / 0..10; the packers
place the input-layer, skip-layer, view-layer and `_time.0` columns through the slot maps of csrc/swnerf_common.h, which turn
slots into zero pad when k >= L.  Here each net kind (CANON, NOVIEW, DNERF, TNERF) runs at the covering set of triples of
tests/golden/cases_bands.py - (10, 4, 10) included as the control row, through the same code and the same gates:

  1. the per-row MLP kernels and the point queries against float64 on the fp32 encodings;
  2. the fused inference pass, with and without resampling, every output against the oracle at the matching multires;
  3. the bf16x3 pass against the fp32 pass (CANON, DNERF: the kinds it is built for), at test_gpu_x3.py's gates;
  4. training through render_rays under autograd, fused and op path: every parameter gradient against float64 autograd with
     exact ReLU-flip accounting, and the gradient shapes;
  5. with no tolerance at all: the narrow net against the (10, 4, 10) net whose extra input columns are zero
     (cases_bands.widen) - the same function, and for the kernels the same MFMA sequence with exact zeros in place of the
     dropped products, so every output of the inference passes is the same BITS; gradients of the shared columns at the
     fused-vs-op gate of test_gpu_backward.py (2e-6 of the tensor's max: the split-K atomics reorder sums);
  6. the refusals: bands beyond the limits at the C ABI, and nets beyond them in Python (generic / op path, to the oracle).

The gates are the ones the same quantity has at (10, 4, 10) elsewhere in the suite (bands_ref.GATES); tests/test_bands_host.py
shows on the CPU that the fp32 oracle alone stays inside them against float64 at every triple, that `widen` builds the
same function, and that the gradient cases have no ReLU unit near its kink.

Measured on MI355X: in each test's docstring (worst over the triples; the control row beside it).  The whole module takes 7 s."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bands_ref as BR
import cases_bands as CB
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
DEV = torch.device("cuda:0")
CASES = [(k, b) for k in CB.KINDS for b in CB.triples(k)]
GRAD_CASES = [(k, b) for k in CB.KINDS for b in CB.triples(k, CB.GRAD_TRIPLES)]
X3_CASES = [(k, b) for k, b in CASES if k in ("canon", "dnerf")]
ids = lambda cases: [f"{c[0]}-{c[1][0]}.{c[1][1]}.{c[1][2]}" for c in cases]
S, NI = CB.N_SAMPLES, CB.N_IMPORTANCE


def _net(kind, sd_np, bands, train=False):
    import swnerf.model as model
    from swnerf.embedder import get_embedder
    Cp, Cd, Ct = CB.widths(CB.applicable(kind, bands))
    if kind == "canon":
        m = model.vallina_NeRF(D=8, W=256, input_ch=Cp, input_ch_views=Cd, output_ch=5, skips=[4], use_viewdirs=True)
    elif kind == "noview":
        m = model.vallina_NeRF(D=8, W=256, input_ch=Cp, input_ch_views=0, output_ch=5, skips=[4], use_viewdirs=False)
    elif kind == "dnerf":
        m = model.DirectTemporalNeRF(D=8, W=256, input_ch=Cp, input_ch_views=Cd, input_ch_time=Ct, output_ch=5, skips=[4],
                                     use_viewdirs=True, embed_fn=get_embedder(bands[0], 3, 0)[0], zero_canonical=True)
    else:
        m = model.TNeRF(8, Cp, Cd, Ct, 128, 4)
    m.load_state_dict({k: T(v) for k, v in sd_np.items()}, strict=True)
    m = m.to(DEV)
    return m.train() if train else m.eval()


def _query(kind, bands, netchunk=1024 * 64):
    """The lambda the runners' create_* build for these encoders (nerf/run.py:248-251, run_dnerf.py:281-286, run_tnerf.py:270-276)"""
    import swnerf.render as render, swnerf.render_dnerf as rd, swnerf.render_tnerf as rt
    from swnerf.embedder import get_embedder
    Lp, Ld, Lt = CB.applicable(kind, bands)
    embed_fn, _ = get_embedder(Lp, 3, 0)
    embeddirs_fn = None if kind == "noview" else get_embedder(Ld, 3, 0)[0]
    embedtime_fn, _ = get_embedder(Lt, 1, 0)
    if kind in ("canon", "noview"):
        return lambda inputs, viewdirs, network_fn: render.run_network(inputs, viewdirs, network_fn, embed_fn=embed_fn,
                                                                       embeddirs_fn=embeddirs_fn, netchunk=netchunk)
    mod = rd if kind == "dnerf" else rt
    return lambda inputs, viewdirs, ts, network_fn: mod.run_network(inputs, viewdirs, ts, network_fn, embed_fn=embed_fn,
                                                                    embeddirs_fn=embeddirs_fn, embedtime_fn=embedtime_fn, netchunk=netchunk)


def _pass(kind, net, rb, n_samples, precision=None, **kw):
    """One launch of the fused inference pass with every output the kind has"""
    import swnerf.render as render, swnerf.render_dnerf as rd, swnerf.render_tnerf as rt
    want = ["rgb_map", "disp_map", "acc_map", "depth_map", "weights", "raw"] + ([] if "z_vals" in kw else ["z_out"])
    if kind == "tnerf":
        assert precision is None
        return rt.render_pass_tnerf(rb, net, n_samples, want=want, **kw)
    if kind == "dnerf":
        kw["run_deform"] = rd.runs_deform(net, float(rb[0, 8]))
        want.append("dx")
    return render.render_pass(rb, net, n_samples, want=want, precision=precision or "fp32", **kw)


def _ref_dtype(kind):
    # the references the other GPU tests use: the fp32 oracle (O.render_rays / render_rays_dnerf) for the reference's nets, float64 (tnerf_ref) for T-NeRF
    return torch.float64 if kind == "tnerf" else torch.float32


@functools.lru_cache(maxsize=None)
def _case(kind, bands, t=CB.FRAME_TIME):
    """Computed once per case and shared: weights, rays, the reference's coarse pass and its resampled depths"""
    sd = CB.weights(kind, bands)
    rb = T(CB.ray_batch(kind, t=t))
    z = BR.coarse_z(rb, S)
    ref = BR.pass_ref(kind, sd, rb, z, bands, True, _ref_dtype(kind))
    ref["z_out"] = z
    zf, zstd = BR.resample_ref(z, ref["weights"], NI)
    return sd, rb, ref, zf, zstd


def _same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


# ---- 2. the fused inference pass -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,bands", CASES, ids=ids(CASES))
def test_render_pass_vs_oracle(kind, bands):
    """swnerf_render_pass at n = 37, S = 40 (+ 24 drawn: a ragged last tile, a workgroup with dead waves) with the in-LDS
    resampling, the fine pass on OUR depths (the policy of test_gpu_parity.py: the comparison is not about sample_pdf's
    conditioning), n = 3 / S = 2, and D-NeRF's `t == 0` canonical-only branch.
    Measured max |delta|, worst triple (control row): CANON rgb 2.9e-6 (7.8e-7), acc 3.0e-6, disp 1.6e-6, depth 1.4e-5, raw 7.4e-6
    (5.0e-6), z_std 1.2e-4; NOVIEW rgb 1.9e-6 (4.5e-7), raw 6.9e-6 (3.8e-6); DNERF rgb 1.1e-5 (3.5e-6), acc 1.2e-5, raw 7.2e-5
    (1.1e-4), dx 1.9e-7 (1.3e-7), z_std 1.8e-4 (6.3e-4); TNERF rgb 1.2e-6 (2.1e-7), raw 1.1e-5 (6.8e-6); coarse depths equal to the
    oracle's bit for bit.  Resampled depths off by > 2e-5, of 2368: CANON <= 14, NOVIEW <= 15 (23 allowed); DNERF at t = 0.5
    <= 31, at the control row (236 allowed)."""
    sd, rb, ref, zf_ref, zstd_ref = _case(kind, bands)
    net = _net(kind, sd, bands)
    with torch.no_grad():
        g = rb.to(DEV)
        c = _pass(kind, net, g, S, white_bkgd=True, **({} if kind == "tnerf" else dict(n_importance=NI)))
        worst = {"coarse": BR.check_pass(c, ref, kind, f"{kind} {bands} coarse")}
        assert 0.05 < float(c["acc_map"].mean()) < 0.95
        if kind == "tnerf":                                  # one net, no resampling (run_tnerf.py:395-500): given depths instead
            z_in = zf_ref.to(DEV)
        else:
            nfl = BR.check_depths(c["z_fine"], zf_ref, S, f"{kind} {bands} z_fine", 0.9 if kind == "dnerf" else 0.99)
            worst["z_std"] = BR.check_pass(c, dict(z_std=zstd_ref), kind, f"{kind} {bands}", keys=["z_std"])
            worst["z_std"]["depths off by > 2e-5"] = nfl
            z_in = c["z_fine"]
            assert bool((z_in[:, 1:] >= z_in[:, :-1]).all())
        f = _pass(kind, net, g, S + NI, white_bkgd=True, z_vals=z_in)
        worst["fine"] = BR.check_pass(f, BR.pass_ref(kind, sd, rb, z_in.cpu(), bands, True, _ref_dtype(kind)), kind, f"{kind} {bands} fine")
        s = _pass(kind, net, g[:3], 2, white_bkgd=False)
        z2 = BR.coarse_z(rb[:3], 2)
        r2 = dict(BR.pass_ref(kind, sd, rb[:3], z2, bands, False, _ref_dtype(kind)), z_out=z2)
        worst["n=3 S=2"] = BR.check_pass(s, r2, kind, f"{kind} {bands} n=3 S=2")
        if kind == "dnerf":
            sd0, rb0, ref0, _, _ = _case(kind, bands, 0.0)
            c0 = _pass(kind, net, rb0.to(DEV), S, white_bkgd=True)
            assert float(c0["dx"].abs().max()) == 0.0
            worst["t=0"] = BR.check_pass(c0, ref0, kind, f"{kind} {bands} t=0")
    for k, w in worst.items():
        print(f"\n[parity] render_pass {kind} {bands} {k}: {BR.fmt(w)}")


# ---- 5. the narrow net == the (10, 4, 10) net with zero columns, bit for bit ------------------------------------------------------------
def _all_passes(kind, net, rb, precision, z_fine=None):
    """z_fine: the depths of the fine pass (None: the ones this coarse pass draws; T-NeRF has no resampling and is always given them)"""
    out = {}
    c = _pass(kind, net, rb, S, precision, white_bkgd=True, **({} if kind == "tnerf" else dict(n_importance=NI)))
    out.update({"c." + k: v for k, v in c.items()})
    z_in = z_fine if z_fine is not None else c["z_fine"]
    out.update({"f." + k: v for k, v in _pass(kind, net, rb, S + NI, precision, white_bkgd=True, z_vals=z_in).items()})
    out.update({"s." + k: v for k, v in _pass(kind, net, rb[:3], 2, precision, white_bkgd=False).items()})
    if kind == "dnerf":
        rb0 = rb.clone()
        rb0[:, 8] = 0.0
        out.update({"t0." + k: v for k, v in _pass(kind, net, rb0, S, precision, white_bkgd=True).items()})
    return out, z_in


WIDE_CASES = [(k, b, "fp32") for k, b in CASES] + [(k, b, "bf16x3") for k, b in X3_CASES]


@pytest.mark.parametrize("kind,bands,precision", WIDE_CASES, ids=[f"{i}-{c[2]}" for i, c in zip(ids(WIDE_CASES), WIDE_CASES)])
def test_narrow_net_equals_widened_net_bit_for_bit(kind, bands, precision):
    """Every output of the inference passes of the net at `bands` is torch.equal (NaN disparity: same pattern) to the pass at
    (10, 4, 10) on the widened net, fed the same depths.  The kernels evaluate all ten / four / ten bands whatever L is and
    the packers write zero into the slots with k >= L, so both launches run the same instructions on the same operands except
    for exact zeros multiplied by a sine instead of by nothing: no k-tile count depends on L (csrc/mlp_core.h), and bit equality
    holds for all four kinds.  bf16x3 is built for CANON and DNERF (the other two kinds have no such pass).
    Measured: equal in all 41 cases."""
    sd, rb, _, zf_ref, _ = _case(kind, bands)
    prec = None if kind == "tnerf" else precision
    with torch.no_grad():
        a, z_fine = _all_passes(kind, _net(kind, sd, bands), rb.to(DEV), prec, zf_ref.to(DEV) if kind == "tnerf" else None)
        b, _ = _all_passes(kind, _net(kind, CB.widen(kind, sd, bands), CB.wide_bands(kind)), rb.to(DEV), prec, z_fine)
    assert list(a) == list(b)
    bad = [k for k in a if not _same(a[k], b[k])]
    assert not bad, f"{kind} {bands} {precision}: differ from the widened net: " + ", ".join(f"{k} {float((a[k] - b[k]).nan_to_num().abs().max()):.2e}" for k in bad)


# ---- 3. bf16x3 against fp32 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,bands", X3_CASES, ids=ids(X3_CASES))
def test_x3_pass_tracks_fp32_pass(kind, bands):
    """swnerf_render_pass_x3 against the fp32 pass of the same triple at the gates test_gpu_x3.py states for (10, 4, 10):
    static raw 1e-4 max(|raw|, 1) + 2e-4, maps and weights 1e-4, depth 5e-4, disparity rtol 1e-3 / atol 1e-4 with equal NaN
    pattern; D-NeRF at t = 0.5 dx 5e-5, raw 1e-3 max|raw|, maps 5e-4, PSNR > 80 dB (t = 0: the static figures, > 95 dB).
    Measured, worst triple (control row): CANON raw 1.7e-4 (7.3e-5), rgb 2.1e-5 (9.2e-6), depth 1.2e-4, PSNR >= 104 dB (114);
    DNERF raw 1.3e-3 on |raw| up to 10 (8.9e-4), rgb 5.9e-5 (1.0e-4), PSNR >= 97.8 dB (94.0)."""
    sd, rb, _, _, _ = _case(kind, bands)
    net = _net(kind, sd, bands)
    g = rb.to(DEV)
    psnr = lambda x, y: float(-10.0 * torch.log10(torch.mean((x.double() - y.double()) ** 2).clamp_min(1e-30)))
    runs = [(g, True)]
    if kind == "dnerf":
        g0 = g.clone()
        g0[:, 8] = 0.0
        runs.append((g0, False))
    for rays, deform in runs:
        with torch.no_grad():
            a = _pass(kind, net, rays, S, "fp32", white_bkgd=True, n_importance=NI)
            b = _pass(kind, net, rays, S, "bf16x3", white_bkgd=True, n_importance=NI)
            fa = _pass(kind, net, rays, S + NI, "fp32", white_bkgd=True, z_vals=a["z_fine"])
            fb = _pass(kind, net, rays, S + NI, "bf16x3", white_bkgd=True, z_vals=a["z_fine"])
        assert torch.equal(a["z_out"], b["z_out"]) and bool((b["z_fine"][:, 1:] >= b["z_fine"][:, :-1]).all())
        for x, y, which in ((a, b, "coarse"), (fa, fb, "fine")):
            scale = max(float(x["raw"].abs().max()), 1.0)
            m = {k: float((x[k] - y[k]).abs().max()) for k in ("raw", "rgb_map", "acc_map", "weights", "depth_map")}
            m["psnr"] = psnr(x["rgb_map"], y["rgb_map"])
            print(f"\n[parity] bf16x3 vs fp32 {kind} {bands} t={float(rays[0, 8]) if kind == 'dnerf' else '-'} {which}: "
                  + ", ".join(f"{k} {v:.3g}" for k, v in m.items()))
            if kind == "canon":
                assert m["raw"] < 1e-4 * scale + 2e-4, m
                assert max(m["rgb_map"], m["acc_map"], m["weights"]) < 1e-4 and m["depth_map"] < 5e-4, m
            else:
                m["dx"] = float((x["dx"] - y["dx"]).abs().max())
                assert m["dx"] < 5e-5 and (deform or float(y["dx"].abs().max()) == 0.0), m
                assert m["raw"] < (1e-3 if deform else 1e-4) * scale, m
                assert max(m["rgb_map"], m["acc_map"], m["weights"]) < (5e-4 if deform else 1e-4), m
                assert m["psnr"] > (80.0 if deform else 95.0), m
            if kind == "canon":                              # (test_gpu_x3.py gates disparity for the static net only)
                nan = torch.isnan(x["disp_map"])
                assert torch.equal(nan, torch.isnan(y["disp_map"]))
                assert torch.allclose(x["disp_map"][~nan], y["disp_map"][~nan], rtol=1e-3, atol=1e-4)


# ---- 1. per-row kernels -----------------------------------------------------------------------------------------------------------------
def _rows(kind, rb):
    """74 sample points of the test rays (two row tiles of 32 and a ragged one), one direction each"""
    z = BR.coarse_z(rb, S)
    pts = (rb[:, None, 0:3] + rb[:, None, 3:6] * z[..., None])[:, ::20].reshape(-1, 3)
    dirs = rb[:, None, -3:].expand(rb.shape[0], 2, 3).reshape(-1, 3) if kind != "noview" else torch.zeros_like(pts)
    return pts.contiguous(), dirs.contiguous()


def _row_gate(got, ref, gate, what):
    d, ex = BR.excess(got, ref, *gate, what)
    assert ex <= 1.0, f"{what}: max |delta| {d:.3e} is {ex:.2f} x the gate ({gate[0]:g} + {gate[1]:g} |ref|)"
    return d


@pytest.mark.parametrize("kind,bands", CASES, ids=ids(CASES))
def test_per_row_kernels_vs_float64(kind, bands):
    """Module.forward on rows of encodings (swnerf_mlp_forward CANON / DNERF with run_deform 1 and 0 and dx_out,
    swnerf_mlp_forward_noview) and the point queries (swnerf_query_points per point and with shared directions,
    swnerf_query_points_time DNERF per point with position_delta, DNERF and TNERF with shared directions; T-NeRF with one
    direction per point runs the encoders and TNeRF.forward, the fused stream has no per-row direction columns) against the
    float64 net on the fp32 encodings.
    Measured max |delta|, worst triple (control row): CANON 4.6e-6 (3.4e-6); NOVIEW 3.8e-6 (2.0e-6); DNERF t = 0.5 raw 3.7e-5
    (5.1e-5), dx 1.2e-7 (7.7e-8), t = 0 raw 4.1e-6; TNERF 8.3e-6 (7.3e-6)."""
    import swnerf.mesh as mesh
    from swnerf.embedder import get_embedder
    Lp, Ld, Lt = CB.applicable(kind, bands)
    sd = CB.weights(kind, bands)
    net = _net(kind, sd, bands)
    rb = T(CB.ray_batch(kind))
    pts, dirs = _rows(kind, rb)
    M = pts.shape[0]
    assert M == 74
    ex, ed = O.embed(pts, Lp), O.embed(dirs, Ld)
    gate = BR.ROW_GATES[kind]
    out = []
    with torch.no_grad():
        if kind == "canon":
            ref, _ = BR.rows_ref(kind, sd, pts, dirs, None, bands)
            out.append(("mlp_forward", _row_gate(net(torch.cat([ex, ed], -1).to(DEV)), ref, gate, "mlp_forward")))
            out.append(("query_points", _row_gate(mesh.query_points(net, pts.to(DEV), dirs.to(DEV)), ref, gate, "query_points")))
        elif kind == "noview":
            ref, _ = BR.rows_ref(kind, sd, pts, dirs, None, bands)
            got = net(ex.to(DEV))
            assert got.shape == (M, 5)
            out.append(("mlp_forward_noview", _row_gate(got, ref, gate, "mlp_forward_noview")))
        elif kind == "dnerf":
            for t in (CB.FRAME_TIME, 0.0):
                ref, dx_ref = BR.rows_ref(kind, sd, pts, dirs, t, bands)
                te = O.embed(torch.full((M, 1), t), Lt).to(DEV)
                g_out, g_dx = net(torch.cat([ex, ed], -1).to(DEV), [te, te])
                gt = gate if t else BR.ROW_GATES["dnerf_t0"]
                out.append((f"mlp_forward t={t}", _row_gate(g_out, ref, gt, f"mlp_forward t={t}")))
                out.append((f"dx t={t}", _row_gate(g_dx, dx_ref, BR.GATES["dx"], f"mlp_forward dx t={t}")))
                q_out, q_dx = mesh.query_points(net, pts.to(DEV), dirs.to(DEV), frame_time=t, return_dx=True)
                out.append((f"query_points_time t={t}", _row_gate(q_out, ref, gt, f"query_points_time t={t}")))
                out.append((f"query dx t={t}", _row_gate(q_dx, dx_ref, BR.GATES["dx"], f"query_points_time dx t={t}")))
                if not t:
                    assert float(g_dx.abs().max()) == 0.0 and float(q_dx.abs().max()) == 0.0
        elif kind == "tnerf":                                # one direction per point: the encoders + TNeRF.forward (mesh._query_tnerf_rows)
            ref, _ = BR.rows_ref(kind, sd, pts, dirs, CB.FRAME_TIME, bands)
            got = mesh.query_points(net, pts.to(DEV), dirs.to(DEV), frame_time=CB.FRAME_TIME)
            out.append(("query_points per point", _row_gate(got, ref, gate, "query_points, one direction per point")))
        if kind in ("canon", "dnerf", "tnerf"):
            # shared directions: [mean over the views of rgb, sigma] (nerf/extract_mesh.py:61-79)
            V = 3
            vd = dirs[::25][:V]
            t = None if kind == "canon" else CB.FRAME_TIME
            per_view = torch.stack([BR.rows_ref(kind, sd, pts, vd[v][None].expand(M, 3), t, bands)[0] for v in range(V)])
            ref = torch.cat([per_view[..., :3].mean(0), per_view[0, :, 3:4]], -1)
            got = mesh.query_points(net, pts.to(DEV), vd.to(DEV), shared_dirs=True, **({} if t is None else dict(frame_time=t)))
            out.append(("query_points shared dirs", _row_gate(got, ref, gate, "query_points, shared directions")))
    print(f"\n[parity] per-row kernels {kind} {bands}: " + ", ".join(f"{k} {v:.2e}" for k, v in out))


# ---- 4. training -------------------------------------------------------------------------------------------------------------------------
FIRST_LAYERS = {"canon": ["pts_linears.0.weight", "pts_linears.5.weight", "views_linears.0.weight"],
                "noview": ["pts_linears.0.weight", "pts_linears.5.weight"],
                "dnerf": ["_occ.pts_linears.0.weight", "_occ.pts_linears.5.weight", "_occ.views_linears.0.weight", "_time.0.weight", "_time.5.weight"],
                "tnerf": ["layers.0.0.weight", "layers.5.0.weight", "layer_9.0.weight"]}


# the band-taking exports a training step must reach (the spy below counts them): fused kernels / op path
FUSED_ENTRIES = {"canon": ["swnerf_render_pass_train", "swnerf_render_pass_backward", "swnerf_pack_net_bwd_kind", "swnerf_unslot_grad"],
                 "noview": ["swnerf_render_pass_train", "swnerf_render_pass_backward_noview", "swnerf_pack_net_bwd_noview", "swnerf_unslot_grad"],
                 "dnerf": ["swnerf_render_pass_train_dnerf", "swnerf_render_pass_backward_dnerf", "swnerf_pack_net_bwd_kind", "swnerf_unslot_grad",
                           "swnerf_unslot_grad_time"],
                 "tnerf": ["swnerf_render_pass_train_tnerf", "swnerf_render_pass_backward_tnerf", "swnerf_pack_net_bwd_tnerf", "swnerf_unslot_grad",
                           "swnerf_unslot_grad_time"]}
OP_ENTRIES = {"canon": ["swnerf_embed", "swnerf_mlp_forward_train", "swnerf_mlp_backward_dx", "swnerf_pack_net_bwd_kind"],
              "noview": ["swnerf_embed"],                                   # then the generic GEMMs, which take no bands
              "dnerf": ["swnerf_embed", "swnerf_deform_forward_train", "swnerf_mlp_forward_train", "swnerf_mlp_backward_dx_pts",
                        "swnerf_deform_backward_dx", "swnerf_pack_net_bwd_kind"],
              "tnerf": ["swnerf_embed"]}


def _train_step(kind, sd_np, bands, rb, loss_of, fused, monkeypatch):
    """loss.backward() through the runner's render_rays on the fused training kernels or on the op path -> (ret, grads)"""
    import swnerf.render as render, swnerf.render_dnerf as rd, swnerf.render_tnerf as rt
    from swnerf import _lib
    net = _net(kind, sd_np, bands, train=True)
    q = _query(kind, bands)
    calls = {}
    real = _lib.lib()

    class Spy:
        def __getattr__(self, name):
            f = getattr(real, name)
            if not name.startswith("swnerf_"):
                return f

            def wrapped(*a, **k):
                calls[name] = calls.get(name, 0) + 1
                return f(*a, **k)
            return wrapped
    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    if fused:
        monkeypatch.delenv("SWNERF_TRAIN_OP_PATH", raising=False)
    else:
        monkeypatch.setenv("SWNERF_TRAIN_OP_PATH", "1")
    kw = dict(N_importance=0, white_bkgd=True, perturb=0., raw_noise_std=0.)
    with torch.enable_grad():
        if kind in ("canon", "noview"):
            ret = render.render_rays(rb.to(DEV), net, q, CB.GRAD_S, **kw)
        elif kind == "dnerf":
            ret = rd.render_rays(rb.to(DEV), net, q, CB.GRAD_S, **kw)
        else:
            with rt.fused_train(fused):
                ret = rt.render_rays(rb.to(DEV), net, q, CB.GRAD_S, **kw)
        loss_of(ret, torch.arange(rb.shape[0])).backward()
    monkeypatch.setattr(_lib, "lib", lambda: real)
    monkeypatch.delenv("SWNERF_TRAIN_OP_PATH", raising=False)
    ran_fused = any(k.startswith("swnerf_render_pass_train") for k in calls)
    assert ran_fused == fused, (kind, fused, sorted(calls))
    missing = [k for k in (FUSED_ENTRIES if fused else OP_ENTRIES)[kind] if k not in calls]
    assert not missing, (kind, fused, missing, sorted(calls))
    return ret, {k: p.grad for k, p in net.named_parameters()}


def _float64_check(kind, sd_np, bands, rb, z, ray_loss, grads, what, dx):
    import dnerf_ref, flipcheck, tnerf_train_ref
    Lp, Ld, Lt = bands
    stats = {}
    if kind in ("canon", "noview"):
        used = {k: g for k, g in grads.items() if kind == "canon" or k.startswith(("pts_linears", "output_linear"))}
        fl = flipcheck.flip_aware_check(sd_np, rb, z, True, ray_loss, used, what, bands=(Lp, Ld), stats=stats)
    elif kind == "dnerf":
        fl = dnerf_ref.flip_aware_check(sd_np, rb, z, True, ray_loss, grads, what, dx.detach().cpu(), bands=bands, stats=stats)
    else:
        fl = tnerf_train_ref.flip_aware_check({k: T(v) for k, v in sd_np.items()}, rb, z, True, ray_loss, grads, what, bands=bands, stats=stats)
    return fl, stats["worst"]


@pytest.mark.parametrize("kind,bands", GRAD_CASES, ids=ids(GRAD_CASES))
def test_training_gradients_vs_float64(kind, bands, monkeypatch):
    """One training step through render_rays at n = 5, S = 33 (a ragged tile, n no multiple of 4) with a loss on rgb_map, acc_map
    and (NaN-guarded) disp_map, so that every seed of the compositing backward is live - on the fused training kernels
    (render_pass_train / _backward and their NOVIEW, D-NeRF and T-NeRF forms) and on the op path (mlp_forward_train,
    mlp_backward_dx, deform_*, the generic GEMMs).  Every parameter gradient against float64 autograd with exact ReLU-flip
    accounting (thr 5e-6, rtol 2e-5: the checkers' defaults); the gradient of every first-layer / skip-layer / view-layer /
    `_time.0` weight has the reference's shape and no NaN.  Fused against op path where both run the same arithmetic per element:
    CANON 2e-6, DNERF 5e-6 of each tensor's max (test_gpu_backward.py's gates; NOVIEW's op path is the generic GEMMs and T-NeRF's
    fused pass folds `feature` into `layer_9`, so there the figure is printed and float64 is the judge).  Then the same step on
    the widened (10, 4, 10) net: its gradients on the shared columns within 2e-6, its forward outputs the same bits.
    (`reproducible_wgrad`, under which these would be the same bits, only acts in the generic GEMMs of swnerf/generic.py; the
    weight gradients of the fused-architecture nets always go through the split-K atomics, so no case here can set it.)
    Measured: worst residual against float64 1.9e-6 of a tensor's max (control rows 9.9e-7 .. 1.9e-6), no risky unit, no flip;
    fused vs op path CANON <= 7.3e-7, DNERF <= 1.3e-6 (NOVIEW 1.5e-6, TNERF 1.8e-6); narrow vs widened <= 2.0e-7."""
    sd_np = CB.weights(kind, bands)
    rb = T(CB.grad_rays(kind, bands))
    n = rb.shape[0]
    z = BR.coarse_z(rb, CB.GRAD_S)
    rng = np.random.default_rng(11)
    tgt, wd, wa = (T(rng.uniform(0, 1, s).astype(np.float32)) for s in ((n, 3), (n,), (n,)))

    def ray_loss(ret, idx):
        c = lambda t: t[idx.to(t.device)].to(ret["rgb_map"])
        ok = ~torch.isnan(ret["disp_map"])
        return (((ret["rgb_map"] - c(tgt)) ** 2).sum() / (3 * n) + 0.1 * (ret["acc_map"] * c(wa)).sum() / n
                + 0.01 * (torch.where(ok, ret["disp_map"], torch.zeros_like(ret["disp_map"])) * c(wd)).sum() / n)

    Cp, Cd, Ct = CB.widths(bands)
    W = 128 if kind == "tnerf" else 256
    shapes = {"pts_linears.0.weight": (W, Cp), "pts_linears.5.weight": (W, Cp + W), "views_linears.0.weight": (W // 2, W + Cd),
              "_time.0.weight": (W, Cp + Ct), "_time.5.weight": (W, Cp + W), "layers.0.0.weight": (W, Cp + Ct),
              "layers.5.0.weight": (W, Cp + Ct + W), "layer_9.0.weight": (W // 2, W + Cd)}
    res = {}
    for fused in (True, False):
        ret, grads = _train_step(kind, sd_np, bands, rb, ray_loss, fused, monkeypatch)
        for name in FIRST_LAYERS[kind]:
            g = grads[name]
            assert g is not None and tuple(g.shape) == shapes[name.replace("_occ.", "")] and bool(torch.isfinite(g).all()), name
        dx = ret.get("position_delta")
        if "z_vals" in ret:                                  # the time-conditioned runners return their depths
            assert float((ret["z_vals"].detach().cpu() - z).abs().max()) <= BR.GATES["z_out"][0]
        fl, worst = _float64_check(kind, sd_np, bands, rb, ret["z_vals"].detach().cpu() if "z_vals" in ret else z, ray_loss, grads, f"{kind} {bands} {'fused' if fused else 'op path'}", dx)
        res[fused] = (ret, grads)
        print(f"\n[parity] training {kind} {bands} {'fused' if fused else 'op path'}: every gradient within 2e-5 of float64, worst {worst:.2e}; "
              f"(flips, risky units) {fl}")
    worst = 0.0
    gate = {"canon": 2e-6, "dnerf": 5e-6}.get(kind)
    for k, gf in res[True][1].items():
        go = res[False][1][k]
        if gf is None or go is None:
            assert kind == "noview" and k.startswith("views_linears"), k          # the module owns it, no pass reads it
            continue
        d, scale = float((gf - go).abs().max()), max(float(go.abs().max()), 1e-12)
        worst = max(worst, d / scale)
        assert gate is None or d <= gate * scale, f"{kind} {bands} {k}: fused vs op path {d:.3e} of {scale:.3e}"
    print(f"\n[parity] training {kind} {bands}: fused vs op path, worst gradient difference {worst:.2e} of its max")
    if bands == CB.wide_bands(kind):
        return
    wide_sd = CB.widen(kind, sd_np, bands)
    ret_w, grads_w = _train_step(kind, wide_sd, CB.wide_bands(kind), rb, ray_loss, True, monkeypatch)
    worst = 0.0
    for k, gn in res[True][1].items():
        gw = grads_w[k]
        if gn is None:
            continue
        cols = CB.shared_columns(kind, k, bands)
        if cols is not None:
            gw = gw[:, torch.from_numpy(cols).to(gw.device)]
        d, scale = float((gn - gw).abs().max()), max(float(gn.abs().max()), 1e-12)
        worst = max(worst, d / scale)
        assert d <= 2e-6 * scale, f"{kind} {bands} {k}: narrow vs widened net {d:.3e} of {scale:.3e}"
    for k in ("rgb_map", "acc_map", "disp_map"):
        assert _same(res[True][0][k].detach(), ret_w[k].detach()), k
    print(f"\n[parity] training {kind} {bands}: narrow vs widened net, worst gradient difference on shared columns {worst:.2e} of its max")


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
BAD = [(11, 4, 10), (10, 5, 10), (10, 4, 11)]


def _refusal(L, _lib):
    def refused(rc, *names, code=None):
        msg = L.swnerf_last_error().decode()
        assert rc == (_lib.E_UNSUPP if code is None else code), (rc, msg)
        assert all(str(v) in msg for v in names), msg
    return refused


def test_c_abi_refuses_bands_beyond_the_limits():
    """Each band-taking entry point returns SWNERF_E_UNSUPP for (11,4,10), (10,5,10), (10,4,11) where it has that member, and
    the T-NeRF packs for L_dir = 0; swnerf_last_error names the bands.  Two entry points that take a single band check it with
    their other arguments and answer SWNERF_E_ARG, naming it (include/swnerf.h says so): swnerf_render_pass_backward_dnerf
    (L_pos) and swnerf_unslot_grad_time (L_time).  Every call returns from its argument check; the pointers are one 16 MiB
    device buffer of zeros and M = 1, so that a check that moved behind a launch would show as a failed assertion here, not
    as a launch on memory the kernel does not own."""
    from swnerf import _lib
    L = _lib.lib()
    refused = _refusal(L, _lib)
    big = torch.zeros(1 << 22, device=DEV)
    p = ctypes.c_void_p(big.data_ptr())
    params = (ctypes.c_void_p * 64)(*([p.value] * 64))
    st = _lib.stream_of(big)

    for Lp, Ld, Lt in BAD:
        three = (Lp, Ld, Lt)
        for kind in (_lib.NET_CANON, _lib.NET_DNERF, _lib.NET_TNERF):
            refused(L.swnerf_pack_net(kind, params, Lp, Ld, Lt, p, st), *three)
        refused(L.swnerf_pack_net_bwd_tnerf(params, Lp, Ld, Lt, p, st), *three)
        refused(L.swnerf_pack_net_x3_kind(_lib.NET_DNERF, params, Lp, Ld, Lt, p, p, st), *three)
        refused(L.swnerf_mlp_forward(_lib.NET_DNERF, p, p, 1, Lp, Ld, p, Lt, 1, p, p, st), *three)
        refused(L.swnerf_deform_forward_train(p, p, p, 1, Lp, Ld, Lt, p, p, p, st), *three)
        for kind in (_lib.NET_DNERF, _lib.NET_TNERF):
            refused(L.swnerf_query_points_time(kind, p, p, 1, p, 1, 0, 0.5, 1, Lp, Ld, Lt, p, None, st), *three)
        if Lt <= 10:
            refused(L.swnerf_query_points(p, p, 1, p, 1, 0, Lp, Ld, p, st), Lp, Ld)
            refused(L.swnerf_mlp_forward_train(p, p, 1, Lp, Ld, p, p, p, st), Lp, Ld)
            refused(L.swnerf_pack_net_bwd(params, Lp, Ld, p, st), Lp, Ld)
            refused(L.swnerf_pack_net_x3(params, Lp, Ld, p, p, st), Lp, Ld)
            for bk in (_lib.BWD_CANON, _lib.BWD_CANON_INPUT_GRAD, _lib.BWD_DEFORM, _lib.BWD_DNERF_FUSED):
                refused(L.swnerf_pack_net_bwd_kind(bk, params, Lp, Ld, p, st), Lp, Ld)
            refused(L.swnerf_unslot_grad(p, 96, 1, 0, 32, Lp, Ld, p, 96, 0, st), Lp, Ld)
        if Lp > 10:
            refused(L.swnerf_pack_net_noview(params, Lp, 5, p, st), Lp)
            refused(L.swnerf_pack_net_bwd_noview(params, Lp, 5, p, st), Lp)
            refused(L.swnerf_mlp_forward_noview(p, p, 1, 3 * (1 + 2 * Lp), Lp, 5, p, st), Lp)
            refused(L.swnerf_mlp_backward_dx_pts(p, p, p, p, 1, Lp, p, p, st), Lp)
            # (packed, bits, bits_d, raw, z, rays, cols, noise, dx, g_pd, n_rays, S, white, L_pos, g_rgb, g_disp, g_acc, g_raw, grad, grad_d, d_raw, g_dx)
            refused(L.swnerf_render_pass_backward_dnerf(p, p, p, p, p, p, 12, None, p, None, 1, 2, 1, Lp, p, None, None, None, p, p, p, p, st),
                    f"L_pos {Lp}", code=_lib.E_ARG)
        if Lt > 10:
            refused(L.swnerf_unslot_grad_time(p, 32, 1, 32, Lt, p, 96, 0, st), f"L_time={Lt}", code=_lib.E_ARG)
    refused(L.swnerf_pack_net(_lib.NET_TNERF, params, 10, 0, 10, p, st), 10, 0)
    refused(L.swnerf_pack_net_bwd_tnerf(params, 10, 0, 10, p, st), 10, 0)
    torch.cuda.synchronize()
    assert float(big.abs().max()) == 0.0                      # nothing was written


def test_fused_passes_refuse_bands_beyond_the_limits():
    """swnerf_render_pass / _x3 and the training passes (swnerf_render_pass_train, _train_dnerf, _train_tnerf) with the
    well-formed arguments and buffers of a real launch and only the bands out of range: SWNERF_E_UNSUPP naming them, nothing
    launched.  (The static training pass has no time band: it is given the two triples it can tell.)"""
    from swnerf import _lib
    import swnerf.render as render
    L = _lib.lib()
    refused = _refusal(L, _lib)
    new = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=DEV)
    n, Sg = 4, CB.GRAD_S
    rows = L.swnerf_train_rows(n, Sg)
    nact, nxs, nbits = L.swnerf_act_floats_per_row(), L.swnerf_xs_floats_per_row(), L.swnerf_mask_floats(rows)
    train_out = ["rgb_map", "disp_map", "acc_map", "raw", "z_out"]

    sd, rb, _, _, _ = _case("dnerf", CB.CONTROL)
    net = _net("dnerf", sd, CB.CONTROL)
    kind, packed, _, _, _ = net.packed()
    g = rb.to(DEV)
    for three in BAD:
        a, out, keep = render.pass_args(g, kind, packed, three, S, 4, 1, {}, ["rgb_map", "disp_map", "acc_map"])
        refused(L.swnerf_render_pass(a, _lib.stream_of(g)), *three)
        a, out, keep = render.pass_args(g, kind, net.packed_x3()[0], three, S, 4, 1, {}, ["rgb_map", "disp_map", "acc_map"])
        refused(L.swnerf_render_pass_x3(a, 3, _lib.stream_of(g)), *three)
        a, out, keep = render.pass_args(g[:n].contiguous(), kind, packed, three, Sg, 4, 1, {}, train_out + ["dx"])
        bufs = [new(rows, nact), new(nbits), new(rows, nxs), new(rows, nact), new(nbits), new(rows, nxs)]
        refused(L.swnerf_render_pass_train_dnerf(a, *[_lib.ptr(b) for b in bufs], _lib.stream_of(g)), *three)
    sdc, rbc, _, _, _ = _case("canon", CB.wide_bands("canon"))
    netc = _net("canon", sdc, CB.wide_bands("canon"))
    kc, pc, _, _, _ = netc.packed()
    gc = rbc.to(DEV)[:n].contiguous()
    for three in BAD[:2]:
        a, out, keep = render.pass_args(gc, kc, pc, three, Sg, 4, 0, {}, train_out)
        bufs = [new(rows, nact), new(nbits), new(rows, nxs)]
        refused(L.swnerf_render_pass_train(a, *[_lib.ptr(b) for b in bufs], _lib.stream_of(gc)), *three[:2])
    sdt, rbt, _, _, _ = _case("tnerf", CB.CONTROL)
    nett = _net("tnerf", sdt, CB.CONTROL)
    kt, pt, _, _, _ = nett.packed()
    gt = rbt.to(DEV)[:n].contiguous()
    for three in BAD:
        a, out, keep = render.pass_args(gt, kt, pt, three, Sg, 4, 0, {}, train_out)
        bufs = [new(rows, L.swnerf_tnerf_act_floats_per_row()), new(rows, L.swnerf_tnerf_xs_floats_per_row())]
        refused(L.swnerf_render_pass_train_tnerf(a, *[_lib.ptr(b) for b in bufs], _lib.stream_of(gt)), *three)
    torch.cuda.synchronize()


def test_nets_beyond_the_limits_take_the_generic_path():
    """A D=8 / W=256 net with input_ch = 69 (L_pos = 11) and a T-NeRF with dir_feat = 3 (L_dir = 0) get no fused plan; they
    render layer by layer on the generic GEMMs / the op path, to the oracle's values."""
    import swnerf.model as model, swnerf.render as render, swnerf.render_tnerf as rt
    from swnerf import synth
    from swnerf.embedder import get_embedder
    rb = T(CB.ray_batch("canon"))
    sd = synth.nerf_state_dict(20251900, 69, 27, alpha_bias=-1.0)
    net = model.vallina_NeRF(D=8, W=256, input_ch=69, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
    net.load_state_dict({k: T(v) for k, v in sd.items()})
    net = net.to(DEV).eval()
    embed_fn, embeddirs_fn = get_embedder(11, 3, 0)[0], get_embedder(4, 3, 0)[0]
    q = lambda inputs, viewdirs, network_fn: render.run_network(inputs, viewdirs, network_fn, embed_fn=embed_fn,
                                                                embeddirs_fn=embeddirs_fn, netchunk=1024 * 64)
    with torch.no_grad():
        assert not net._is_fused_arch() and render.fused_plan(q, [net, None]) is None
        with pytest.raises(NotImplementedError):
            net.packed()
        r = render.render_rays(rb.to(DEV), net, q, S, retraw=True, N_importance=0, white_bkgd=True)
        ref = O.render_rays(rb, O.to_torch_sd(sd), None, S, 0, white_bkgd=True, retraw=True, multires=11, multires_views=4)
        w = BR.check_pass(r, ref, "canon", "L_pos = 11 on the generic path", keys=["rgb_map", "disp_map", "acc_map", "raw"])
        print(f"\n[parity] vallina_NeRF input_ch = 69 (generic path) vs oracle: {BR.fmt(w)}")
        # T-NeRF without direction bands
        bands = (6, 0, 9)
        Cp, Cd, Ct = CB.widths(bands)
        sdt = synth.tnerf_state_dict(20251901, Cp, Cd, Ct, density_bias=0.5)
        tn = model.TNeRF(8, Cp, Cd, Ct, 128, 4)
        tn.load_state_dict({k: T(v) for k, v in sdt.items()})
        tn = tn.to(DEV).eval()
        rbt = T(CB.ray_batch("tnerf"))
        embed_fn, embeddirs_fn, embedtime_fn = get_embedder(6, 3, 0)[0], get_embedder(0, 3, 0)[0], get_embedder(9, 1, 0)[0]
        qt = lambda inputs, viewdirs, ts, network_fn: rt.run_network(inputs, viewdirs, ts, network_fn, embed_fn=embed_fn,
                                                                    embeddirs_fn=embeddirs_fn, embedtime_fn=embedtime_fn, netchunk=1024 * 64)
        assert tn.fused_bands() is None and rt.tnerf_plan(qt, tn) is None
        with pytest.raises(NotImplementedError):
            tn.packed()
        r = rt.render_rays(rbt.to(DEV), tn, qt, S, retraw=True, white_bkgd=True)
        z = r["z_vals"].cpu()
        assert float((z - BR.coarse_z(rbt, S)).abs().max()) <= BR.GATES["z_out"][0]
        # (bands_ref takes the kind's own L_dir >= 1 through `applicable`; here the reference is evaluated at L_dir = 0 directly)
        n = rbt.shape[0]
        pts = (rbt[:, None, 0:3] + rbt[:, None, 3:6] * z[..., None]).reshape(-1, 3)
        sd64 = BR.sd_of(sdt, torch.float64)
        ex, ed = O.embed(pts, 6).double(), O.embed(rbt[:, None, -3:].expand(n, S, 3).reshape(-1, 3), 0).double()
        et = O.embed(torch.full((n * S, 1), CB.FRAME_TIME), 9).double()
        raw = BR.tnerf_mlp(sd64, ex, et, ed).reshape(n, S, 4)
        rgb, disp, acc, _, _ = O.raw2outputs(raw, z.double(), rbt[:, 3:6].double(), 0., True)
        assert 0.05 < float(acc.mean()) < 0.95
        w = BR.check_pass(r, dict(rgb_map=rgb, disp_map=disp, acc_map=acc, raw=raw), "tnerf", "T-NeRF L_dir = 0 on the op path",
                          keys=["rgb_map", "disp_map", "acc_map", "raw"])
        print(f"\n[parity] TNeRF dir_feat = 3 (op path) vs float64: {BR.fmt(w)}")
