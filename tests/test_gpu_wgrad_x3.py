"""swnerf_gemm_tn_group_x3 (csrc/wgrad_x3_kernels.hip) through the C ABI against float64, and a fused training step in both
weight-gradient modes.

Operands are 256-column windows of [M, 2432] buffers like `grad` / `act`; every output is a window inside a larger buffer of non-zero
floats and everything outside the window must come back bit for bit.  The main C of an item on the bf16x3 kernel gets the gate AND the
1/16 condition of tests/wgrad_x3_ref.py.  What the entry keeps in fp32 gets the fp32 gate of tests/test_gpu_wgrad_units.py,
    |got - ref64| <= n u (|A|^T |B| + |C0|),  n = M + 514,  u = 2^-24:
the bias column sums, the B2 rider (its own swnerf_gemm_tn launch) and the main C of an item on the fallback (M < 4096, an operand off
16-byte alignment, the 17th item).  Row counts: 4096 = one slab per workgroup, 4100 = 129 workgroups, the last with 4 rows, 24 581 =
several slabs per workgroup and a partial one."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(os.path.dirname(HERE), "sw-nerf_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import cases                    # noqa: E402
import wgrad_units_ref as WR    # noqa: E402
import wgrad_x3_ref as XR       # noqa: E402
from oracle import nerf_oracle as O    # noqa: E402
from swnerf import _lib, wgrad  # noqa: E402

pytestmark = pytest.mark.gpu
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
_BUFFERS, _PRODUCTS = {}, {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    yield torch.device("cuda:0")
    _BUFFERS.clear()
    _PRODUCTS.clear()


def _buffers(dev, M, zeros):
    """GA, GB [M, 2432] and enc [M, 90] for one case, made once: device randn around the seeded operand columns of wgrad_x3_ref"""
    if (M, zeros) not in _BUFFERS:
        g = torch.Generator(device=dev).manual_seed(31 * M + int(zeros))
        GA, GB = (torch.randn((M, XR.LD), generator=g, device=dev) for _ in range(2))
        A, B = XR.operands(M, zeros)
        GA[:, XR.A_COL:XR.A_COL + A.shape[1]] = A.to(dev)
        GB[:, XR.B_COL:XR.B_COL + B.shape[1]] = B.to(dev)
        _BUFFERS[(M, zeros)] = GA, GB, torch.randn((M, 90), generator=g, device=dev)
    return _BUFFERS[(M, zeros)]


def _at(t, floats):
    return ctypes.c_void_p(t.data_ptr() + 4 * floats)


def _fp32_gate(what, got, ref, mag, M):
    r = WR.ratio(got, ref, mag, M + 514)
    print(f"{what}: |got - ref64| / fp32 gate = {r:.3e}")
    assert r <= 1.0, f"{what}: {r:.3e} of the fp32 gate"


def _run_group(dev, M, zeros, items):
    """items: dicts(aw, bw: window 0 / 1 of the seeded A / B columns; bias, rider: bool; a_off: floats the A window is shifted by).
    One swnerf_gemm_tn_group_x3 call; then every output of every item against float64."""
    L = _lib.lib()
    GA, GB, enc = _buffers(dev, M, zeros)
    g = torch.Generator(device=dev).manual_seed(1009 * M + len(items))
    out, arr = [], []
    for q in items:
        Cb, bb, C2b = (torch.randn(s, generator=g, device=dev) for s in ((258, 265), (263,), (258, 70)))
        out.append((Cb, bb, C2b, Cb.clone(), bb.clone(), C2b.clone()))
        a_col, b_col = XR.A_COL + 256 * q["aw"] + q.get("a_off", 0), XR.B_COL + 256 * q["bw"]
        arr.append(_lib.GemmItem(_at(GA, a_col), XR.LD, _at(GB, b_col), XR.LD, _at(Cb, 265 + 5), 265, _at(bb, 3) if q.get("bias") else None,
                                 _at(enc, 0) if q.get("rider") else None, 90, 63 if q.get("rider") else 0,
                                 _at(C2b, 70 + 4) if q.get("rider") else None, 70, None, 0, 0, None, 0, None))
    _lib.check(L.swnerf_gemm_tn_group_x3((_lib.GemmItem * len(arr))(*arr), len(arr), M, _lib.stream_of(GA)), "gemm_tn_group_x3")
    torch.cuda.synchronize()
    n_x3 = 0
    for k, (q, (Cb, bb, C2b, C0, b0, C20)) in enumerate(zip(items, out)):
        a_col, b_col = XR.A_COL + 256 * q["aw"] + q.get("a_off", 0), XR.B_COL + 256 * q["bw"]
        A, B = GA[:, a_col:a_col + 256], GB[:, b_col:b_col + 256]
        what = f"M={M} zeros={zeros} item {k}/{len(items)}"
        on_x3 = M >= 4096 and a_col % 4 == 0 and n_x3 < 16
        c0 = C0[1:257, 5:261]
        key = (M, zeros, a_col, b_col)
        if key not in _PRODUCTS:                              # float64, once per operand pair
            _PRODUCTS[key] = XR.reference(A, B)
        if on_x3:
            n_x3 += 1
            XR.check(what + " C", Cb[1:257, 5:261], M, _PRODUCTS[key], c0)
        else:
            ref, mag, _ = _PRODUCTS[key]
            _fp32_gate(what + " C (fp32 route)", Cb[1:257, 5:261], c0.double() + ref, mag + c0.double().abs(), M)
        outside = torch.ones_like(Cb, dtype=torch.bool)
        outside[1:257, 5:261] = False
        assert torch.equal(Cb[outside], C0[outside]), what + ": C was written outside its window"
        if q.get("bias"):
            a64 = A.double()
            _fp32_gate(what + " bias", bb[3:259], b0[3:259].double() + a64.sum(0), a64.abs().sum(0) + b0[3:259].double().abs(), M)
            assert torch.equal(bb[:3], b0[:3]) and torch.equal(bb[259:], b0[259:]), what + ": bias was written outside its window"
        else:
            assert torch.equal(bb, b0), what + ": bias written without a bias pointer"
        if q.get("rider"):
            a64, e64, c20 = A.double(), enc[:, :63].double(), C20[1:257, 4:67].double()
            _fp32_gate(what + " C2", C2b[1:257, 4:67], c20 + a64.T @ e64, a64.abs().T @ e64.abs() + c20.abs(), M)
            outside = torch.ones_like(C2b, dtype=torch.bool)
            outside[1:257, 4:67] = False
            assert torch.equal(C2b[outside], C20[outside]), what + ": C2 was written outside its window"
        else:
            assert torch.equal(C2b, C20)


@pytest.mark.parametrize("M,zeros", XR.CASES, ids=lambda v: str(v))
def test_one_item_with_bias(dev, M, zeros):
    _run_group(dev, M, zeros, [dict(aw=0, bw=0, bias=True)])


@pytest.mark.parametrize("M", [4096, 4100, 24581])
def test_one_item_without_bias_and_with_rider(dev, M):
    """no bias pointer: the bias buffer stays untouched; the rider (Ni2 = 63 of ld 90) into its own window"""
    _run_group(dev, M, False, [dict(aw=1, bw=0)])
    _run_group(dev, M, False, [dict(aw=0, bw=1, bias=True, rider=True)])


@pytest.mark.parametrize("M,zeros", [(4100, False), (24581, True)], ids=lambda v: str(v))
def test_group_of_three(dev, M, zeros):
    """three items of one launch, each on its own workgroup range and row split (85 workgroups per item), the middle one with a rider"""
    _run_group(dev, M, zeros, [dict(aw=0, bw=0, bias=True), dict(aw=1, bw=1, bias=True, rider=True), dict(aw=1, bw=0)])


def test_group_of_seventeen(dev):
    """16 items in the grouped launch (16 workgroups each, 256 rows per workgroup), the 17th alone on the fp32 kernel"""
    _run_group(dev, 4096, False, [dict(aw=k & 1, bw=(k >> 1) & 1, bias=k % 3 == 0) for k in range(17)])


def test_fallbacks_are_fp32(dev):
    """M = 4095 (below the LDS-DMA kernels' threshold) and an A window one float off 16-byte alignment: today's fp32 route"""
    _BUFFERS.setdefault((4095, False), tuple(b[:4095] for b in _buffers(dev, 4096, False)))
    _run_group(dev, 4095, False, [dict(aw=0, bw=0, bias=True), dict(aw=1, bw=1, bias=True, rider=True)])
    _run_group(dev, 4096, False, [dict(aw=0, bw=0, bias=True, a_off=1), dict(aw=0, bw=1, bias=True)])


# ---- a fused training step in both modes ------------------------------------------------------------------------------------------
def _both_modes(step):
    """step() -> {name: gradient}.  Runs it with the fp32 and with the bf16x3 weight-gradient GEMMs; every tensor of the latter within
    2e-5 of the former's max |g| (the project's standing gradient gate; the float64 emulation puts bf16x3 at 4.2-4.7e-6 on random operands)."""
    prev = wgrad.set_precision("fp32")
    try:
        n0 = wgrad.X3_LAUNCHES
        g32 = step()
        assert wgrad.X3_LAUNCHES == n0, "the fp32 mode launched the bf16x3 kernel"
        wgrad.set_precision("bf16x3")
        gx3 = step()
        assert wgrad.X3_LAUNCHES > n0, "the bf16x3 mode never reached swnerf_gemm_tn_group_x3"
    finally:
        wgrad.set_precision(prev)
    assert list(g32) == list(gx3) and all(v is not None for v in g32.values())
    bad = []
    for k in g32:
        scale = max(float(g32[k].abs().max()), 1e-30)
        r = float((gx3[k].double() - g32[k].double()).abs().max()) / scale
        print(f"  {k:40s} max |g_x3 - g_fp32| / max |g_fp32| = {r:.3e}")
        if r > 2e-5:
            bad.append((k, r))
    assert not bad, bad


def test_static_training_step_in_both_modes(dev):
    """64 rays x (64 + 64) samples, two nets with view directions, perturb = 0: the coarse pass has 4096 rows, the fine pass 8192"""
    import swnerf.embedder as embedder, swnerf.model as model, swnerf.render as render
    sd_c, sd_f = cases.weights_static()
    embed_fn, _ = embedder.get_embedder(10, 3, 0)
    embeddirs_fn, _ = embedder.get_embedder(4, 3, 0)
    q = lambda inputs, viewdirs, network_fn: render.run_network(inputs, viewdirs, network_fn, embed_fn=embed_fn,
                                                                embeddirs_fn=embeddirs_fn, netchunk=1024 * 64)
    g = cases.g7_inputs(n=64, seed=41)
    rb = O.make_ray_batch(T(g["rays_o"]), T(g["rays_d"]), 2., 6.).to(dev)
    tgt = T(np.random.default_rng(6).uniform(0, 1, (64, 3)).astype(np.float32)).to(dev)

    def net(sd):
        m = model.vallina_NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
        m.load_state_dict({k: T(v) for k, v in sd.items()})
        return m.to(dev)

    def step():
        nc, nf = net(sd_c), net(sd_f)
        with torch.enable_grad():
            ret = render.render_rays(rb, nc, q, 64, N_importance=64, network_fine=nf, white_bkgd=True, perturb=0., raw_noise_std=0.)
            (torch.mean((ret["rgb_map"] - tgt) ** 2) + torch.mean((ret["rgb0"] - tgt) ** 2)).backward()
        torch.cuda.synchronize()
        return {"c." + k: p.grad for k, p in nc.named_parameters()} | {"f." + k: p.grad for k, p in nf.named_parameters()}

    print("\n[wgrad x3] static step, 64 x (64 + 64):")
    _both_modes(step)


def test_dnerf_training_step_in_both_modes(dev):
    """DirectTemporalNeRF at one frame time (t = 0.5), 64 rays x (64 + 64): the deformation net's and the canonical net's GEMMs"""
    import swnerf.embedder as embedder, swnerf.model as model, swnerf.render_dnerf as rd
    sd = cases.weights_dnerf()
    embed_fn, _ = embedder.get_embedder(10, 3, 0)
    embeddirs_fn, _ = embedder.get_embedder(4, 3, 0)
    embedtime_fn, _ = embedder.get_embedder(10, 1, 0)
    q = lambda inputs, viewdirs, ts, network_fn: rd.run_network(inputs, viewdirs, ts, network_fn, embed_fn=embed_fn,
                                                                embeddirs_fn=embeddirs_fn, embedtime_fn=embedtime_fn, netchunk=1024 * 64)
    g = cases.g8_inputs(n=64)
    rb = O.make_ray_batch(T(g["rays_o"]), T(g["rays_d"]), 2., 6., frame_time=0.5).to(dev)
    tgt = T(np.random.default_rng(7).uniform(0, 1, (64, 3)).astype(np.float32)).to(dev)

    def step():
        m = model.DirectTemporalNeRF(D=8, W=256, input_ch=63, input_ch_views=27, input_ch_time=21, output_ch=5, skips=[4],
                                     use_viewdirs=True, embed_fn=embed_fn, zero_canonical=True)
        m.load_state_dict({k: T(v) for k, v in sd.items()})
        m = m.to(dev)
        with torch.enable_grad():
            ret = rd.render_rays(rb, m, q, 64, N_importance=64, white_bkgd=True, perturb=0., raw_noise_std=0.)
            loss = torch.mean((ret["rgb_map"] - tgt) ** 2)
            if "rgb0" in ret:
                loss = loss + torch.mean((ret["rgb0"] - tgt) ** 2)
            loss.backward()
        torch.cuda.synchronize()
        return {k: p.grad for k, p in m.named_parameters()}

    print("\n[wgrad x3] D-NeRF step at t = 0.5, 64 x (64 + 64):")
    _both_modes(step)
