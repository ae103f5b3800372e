"""LPIPS on the GPU against the float64 restatement tests/lpips_ref.py: the implicit-GEMM convolution, the pooling kernel,
the per-tap kernel, and metrics.LPIPS end to end for both trunks.

The tolerance is not a fixed number.  The yardstick is the package's own arithmetic: lpips_ref(fp32=True) (the same graph in
float32 on the CPU) deviates from float64 by at most e_ref over a test set; the kernels may deviate by at most 4 x e_ref over
the same set - both are fp32 accumulations over the same K in different summation orders.  Every set has at least 8 cases.
Each test prints its figures before it asserts (pytest -s shows them)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R

pytestmark = pytest.mark.gpu
GATE = 4.0


def _dev():
    return torch.device("cuda:0")


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


# ---- 1. conv2d_nhwc -------------------------------------------------------------------------------------------------------
# (name, N, Cin, Cout, H, W, kernel, stride, pad)
CONV_CASES = [
    ("a_alex_conv1", 2, 3, 64, 35, 47, 11, 4, 2),        # K = 363, tiles straddle the image boundary
    ("b_alex_conv2", 1, 64, 192, 7, 5, 5, 1, 2),
    ("c_vgg_conv1", 2, 3, 64, 18, 21, 3, 1, 1),          # K = 27
    ("d_vgg_conv5", 1, 512, 512, 3, 2, 3, 1, 1),         # K = 4608, the window is mostly padding
    ("e_ragged_1x1", 3, 5, 37, 9, 9, 1, 1, 0),           # ragged Cin and Cout
    ("e_ragged_3x3s2", 3, 5, 37, 9, 9, 3, 2, 0),
    ("f_one_pixel_1x1", 1, 5, 37, 1, 1, 1, 1, 0),        # a single output pixel
    ("f_one_pixel_3x3s2", 1, 5, 37, 3, 3, 3, 2, 0),
    ("g_cout70_scalar_weights", 2, 8, 70, 6, 7, 3, 1, 1),   # the 128-wide tile with 4-byte weight loads, K = 72 (a ragged chunk)
    ("h_s3_p5_k7", 1, 4, 132, 10, 13, 7, 3, 5),          # stride 3, the widest padding, two column tiles
]


@pytest.fixture(scope="module")
def conv_refs():
    out = {}
    for idx, (name, n, ci, co, h, w, k, s, p) in enumerate(CONV_CASES):
        g = torch.Generator().manual_seed(100 + idx)
        x = torch.randn(n, ci, h, w, generator=g)
        wt = torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
        b = 0.1 + 0.02 * torch.randn(co, generator=g)
        r64 = F.conv2d(x.double(), wt.double(), b.double(), stride=s, padding=p)
        r32 = F.conv2d(x, wt, b, stride=s, padding=p)
        out[name] = (x, wt, b, r64, r32)
    return out


def test_conv2d_nhwc_against_float64(conv_refs):
    from swnerf import lpips
    dev, cache = _dev(), {}
    worst_ref, rows = 0.0, []
    for idx, (name, n, ci, co, h, w, k, s, p) in enumerate(CONV_CASES):
        x, wt, b, r64, r32 = conv_refs[name]
        packed = lpips.pack_conv_weight(cache, idx, wt.to(dev))
        assert torch.equal(packed.cpu().view(k, k, ci, co), wt.permute(2, 3, 1, 0))
        for relu in (False, True):
            want = torch.relu(r64) if relu else r64
            got = lpips.conv2d_nhwc(_nhwc(x).to(dev), packed, b.to(dev), co, k, s, p, relu=relu).cpu()
            assert got.shape == _nhwc(want).shape, name
            scale = float(want.abs().max())
            e_k = float((got.double() - _nhwc(want)).abs().max()) / scale           # every output, borders included
            e_r = float(((torch.relu(r32) if relu else r32).double() - want).abs().max()) / scale
            worst_ref = max(worst_ref, e_r)
            rows.append((name, relu, e_k, e_r))
            if relu:
                assert bool((got >= 0).all())
    for name, relu, e_k, e_r in rows:
        print(f"conv {name:26s} relu={int(relu)} kernel {e_k:.3e} fp32-ref {e_r:.3e} ratio to e_ref {e_k / worst_ref:.2f}")
    print(f"conv e_ref = {worst_ref:.3e}, worst kernel / e_ref = {max(r[2] for r in rows) / worst_ref:.2f}")
    assert len(rows) >= 8 and worst_ref > 0
    for name, relu, e_k, _ in rows:
        assert e_k <= GATE * worst_ref, (name, relu, e_k, worst_ref)


def test_conv2d_nhwc_without_bias_and_twice_the_same_bits(conv_refs):
    from swnerf import lpips
    dev = _dev()
    name, n, ci, co, h, w, k, s, p = CONV_CASES[1]
    x, wt, b, r64, _ = conv_refs[name]
    packed = lpips.pack_conv_weight({}, 0, wt.to(dev))
    xs = _nhwc(x).to(dev)
    a = lpips.conv2d_nhwc(xs, packed, None, co, k, s, p)
    assert torch.equal(a, lpips.conv2d_nhwc(xs, packed, None, co, k, s, p))
    assert torch.equal(a, lpips.conv2d_nhwc(xs, packed, torch.zeros(co, device=dev), co, k, s, p))     # no bias = a zero bias
    assert not torch.equal(a, lpips.conv2d_nhwc(xs, packed, b.to(dev), co, k, s, p))
    nan = xs.clone()
    nan[0, 3, 2, 5] = float("nan")                                                  # a NaN stays a NaN through the ReLU
    out = lpips.conv2d_nhwc(nan, packed, b.to(dev), co, k, s, p, relu=True)
    assert bool(torch.isnan(out[0, 3, 2]).all()) and not bool(torch.isnan(out[0, 0, 0]).any())


# ---- 2. maxpool2d_nhwc ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("special", [None, float("nan"), float("-inf")])
def test_maxpool2d_nhwc_equals_torch(special):
    from swnerf import lpips
    dev = _dev()
    g = torch.Generator().manual_seed(7)
    for h, w in ((7, 7), (8, 9)):
        for c in (64, 5):
            x = torch.randn(3, c, h, w, generator=g)
            if special is not None:
                x[0, 1, 2, 2] = special                                               # inside several windows
                x[1, :, :3, :3] = special                                             # a whole 3 x 3 window
                x[2, c - 1, h - 2, w - 2] = special
            for win in (3, 2):
                want = _nhwc(F.max_pool2d(x, kernel_size=win, stride=2))
                got = lpips.maxpool2d_nhwc(_nhwc(x).to(dev), win).cpu()
                np.testing.assert_array_equal(got.numpy(), want.numpy(), err_msg=f"{h}x{w} c={c} window {win}")


# ---- 3. lpips_layer -------------------------------------------------------------------------------------------------------
LAYER_CASES = [(c, h, w) for c in (64, 512, 5) for h, w in ((1, 1), (3, 2), (7, 10))]


@pytest.fixture(scope="module")
def layer_refs():
    out = []
    for idx, (c, h, w) in enumerate(LAYER_CASES):
        g = torch.Generator().manual_seed(200 + idx)
        f0 = torch.relu(torch.randn(2, c, h, w, generator=g))
        f1 = torch.relu(f0 + 0.3 * torch.randn(2, c, h, w, generator=g))
        f1[0, :, 0, 0] = 0                                                            # the eps path: an all-zero pixel in one image
        lin = torch.rand(c, generator=g)
        out.append((f0, f1, lin, R.layer(f0.double(), f1.double(), lin.double()), R.layer(f0, f1, lin).double()))
    return out


def test_lpips_layer_against_float64(layer_refs):
    from swnerf import lpips
    dev = _dev()
    e_ref = max(float((r32 - r64).abs().max()) for _, _, _, r64, r32 in layer_refs)
    rows = []
    for (c, h, w), (f0, f1, lin, r64, _) in zip(LAYER_CASES, layer_refs):
        a, b, l = _nhwc(f0).to(dev), _nhwc(f1).to(dev), lin.to(dev)
        got, mp = lpips.lpips_layer(a, b, l, want_map=True)
        again = lpips.lpips_layer(a, b, l)
        assert got.dtype == torch.float64 and torch.equal(got, again)                 # two runs, the same bits
        assert torch.equal(lpips.lpips_layer(b, a, l), got)                           # (x - y)^2 = (y - x)^2 in every bit
        assert torch.equal(lpips.lpips_layer(a, a, l), torch.zeros(2, dtype=torch.float64, device=dev))
        assert torch.allclose(mp.double().mean(dim=(1, 2)), got, rtol=1e-12, atol=0)  # the map is what the mean is taken of
        acc = lpips.lpips_layer(a, b, l, out=got.clone(), accumulate=True)
        assert torch.equal(acc, got + got)
        rows.append(((c, h, w), float((got.cpu() - r64).abs().max())))
    for case, e_k in rows:
        print(f"layer C,h,w={case} kernel {e_k:.3e} ratio to e_ref {e_k / e_ref:.2f}")
    print(f"layer e_ref = {e_ref:.3e}")
    assert len(rows) >= 8 and e_ref > 0
    for case, e_k in rows:
        assert e_k <= GATE * e_ref, (case, e_k, e_ref)


# ---- 4. end to end --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e():
    """the models and, per (net, size, normalize, uint8), the inputs and both references; e_ref over all final values"""
    from swnerf import metrics
    weights = {net: R.seeded_weights(net) for net in ("alex", "vgg")}
    models = {net: metrics.LPIPS(net, weights=weights[net], device=_dev()) for net in weights}
    entries = []
    for net in ("alex", "vgg"):
        for si, (h, w) in enumerate(R.E2E_SIZES[net]):
            gt, pred = R.seeded_images(3, h, w, R.IMG_SEED)
            for normalize in (False, True):
                for u8 in ((False, True) if si == 0 else (False,)):
                    a, b = ((pred * 255).round().to(torch.uint8), (gt * 255).round().to(torch.uint8)) if u8 else (pred, gt)
                    fa, fb = (a.float() / 255., b.float() / 255.) if u8 else (a, b)
                    r64 = R.lpips_ref(net, *weights[net], fa, fb, normalize=normalize)
                    r32 = R.lpips_ref(net, *weights[net], fa, fb, normalize=normalize, fp32=True)
                    entries.append(dict(net=net, hw=(h, w), normalize=normalize, u8=u8, a=a, b=b, r64=r64, r32=r32))
    e_ref = max(float((e["r32"] - e["r64"]).abs().max()) for e in entries)
    assert sum(e["r64"].numel() for e in entries) >= 8 and e_ref > 0
    return models, entries, e_ref


def _pick(entries, net, size_index=0, normalize=False, u8=False):
    return next(e for e in entries if e["net"] == net and e["hw"] == R.E2E_SIZES[net][size_index] and e["normalize"] == normalize and e["u8"] == u8)


def test_lpips_end_to_end_against_float64(e2e):
    models, entries, e_ref = e2e
    rows = []
    for e in entries:
        got = models[e["net"]](e["a"], e["b"], normalize=e["normalize"])
        assert got.shape == (3, 1, 1, 1) and got.dtype == torch.float32 and got.is_cuda
        rows.append((e, float((got.reshape(-1).cpu().double() - e["r64"]).abs().max())))
    for e, e_k in rows:
        print(f"lpips {e['net']:4s} {e['hw']} normalize={int(e['normalize'])} uint8={int(e['u8'])} values {[round(v, 5) for v in e['r64'].tolist()]} "
              f"kernel {e_k:.3e} ratio to e_ref {e_k / e_ref:.2f}")
    print(f"lpips e_ref = {e_ref:.3e}")
    for e, e_k in rows:
        assert e_k <= GATE * e_ref, (e["net"], e["hw"], e["normalize"], e["u8"], e_k, e_ref)


@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_lpips_layouts_chunks_identity_and_symmetry(e2e, net):
    models, entries, e_ref = e2e
    m, e = models[net], _pick(entries, net, normalize=True)
    a, b = e["a"], e["b"]
    base = m(a, b, normalize=True)
    assert torch.equal(m(_nhwc(a), _nhwc(b), normalize=True, layout="nhwc"), base)
    assert torch.equal(m(a.numpy(), b.to(_dev()), normalize=True), base)              # numpy, CPU and GPU tensors alike
    assert torch.equal(m(a, b, normalize=True, chunk_frames=1), base)                 # chunked = unchunked, bit for bit
    assert torch.equal(m(a, b, normalize=True, chunk_frames=2), base)
    assert torch.equal(m(a[0], b[0], normalize=True), base[:1])                       # one 3-d frame
    assert torch.equal(m(a, a, normalize=True), torch.zeros(3, 1, 1, 1, device=_dev()))
    swapped = m(b, a, normalize=True)
    assert float((swapped - base).abs().max()) <= GATE * e_ref
    assert float((swapped.reshape(-1).cpu().double() - e["r64"]).abs().max()) <= GATE * e_ref


def test_calculate_metrics_and_the_notebook_class_with_a_model(e2e):
    from swnerf import metrics
    models, entries, e_ref = e2e
    e = _pick(entries, "alex", normalize=False)
    pred, gt = _nhwc(e["a"]).numpy(), _nhwc(e["b"]).numpy()                          # [0, 1] HWC frames, pred already clipped
    want = R.lpips_ref("alex", *R.seeded_weights("alex"), e["b"], e["a"], normalize=False)       # the reference's order: (gt, pred)
    plain = metrics.calculate_metrics(gt[0], pred[0])
    assert plain[2] is None
    for i in range(3):
        psnr, ssim, lp = metrics.calculate_metrics(gt[i], pred[i], lpips_model=models["alex"])
        assert lp.shape == (1, 1, 1, 1) and abs(float(lp) - float(want[i])) <= GATE * e_ref
        assert (psnr, ssim) == metrics.calculate_metrics(gt[i], pred[i])[:2]
    ps, ss, lps = metrics.batch_metrics(gt, pred, lpips_model=models["alex"])
    assert (ps, ss) == metrics.batch_metrics(gt, pred) and len(lps) == 3
    assert max(abs(l - float(v)) for l, v in zip(lps, want)) <= GATE * e_ref
    # an unclipped prediction is clipped before the network sees it, as nerf/run.py:55 does
    wild = pred + np.where(pred >= 1.0, 0.5, 0.0).astype(np.float32) - np.where(pred <= 0.0, 0.5, 0.0).astype(np.float32)
    assert metrics.batch_metrics(gt, wild, lpips_model=models["alex"])[2] == lps
    # the notebook: VGG, [0, 1] -> [-1, 1], the mean over the batch
    v = _pick(entries, "vgg", normalize=True)
    nb = metrics.LPIPS_notebook.__new__(metrics.LPIPS_notebook)
    nb.model = models["vgg"]
    got = nb(v["a"], v["b"])
    assert got.ndim == 0 and abs(float(got) - float(v["r64"].mean())) <= GATE * e_ref
    err = metrics.estim_error(v["a"].numpy(), v["b"].numpy(), lpips_model=nb)
    assert set(err) == {"mse", "psnr", "ssim", "lpips"} and err["lpips"] == float(got)
    assert metrics.estim_error(v["a"].numpy(), v["b"].numpy(), lpips_model=models["vgg"])["lpips"] == float(got)
    assert set(metrics.estim_error(v["a"].numpy(), v["b"].numpy())) == {"mse", "psnr", "ssim"}


def test_the_weight_pack_cache_is_the_one_of_packing(e2e):
    models, entries, _ = e2e
    m = models["alex"]
    packs = {k: v[1].data_ptr() for k, v in m._packs.items()}
    assert sorted(packs) == [0, 1, 2, 3, 4]
    e = _pick(entries, "alex")
    before = m(e["a"], e["b"])
    assert {k: v[1].data_ptr() for k, v in m._packs.items()} == packs                # a second call packs nothing again
    w0 = m._dev[0][0][0]
    w0.mul_(2.0)                                                                      # an in-place change is seen: a NEW packed tensor
    changed = m(e["a"], e["b"])
    w0.mul_(0.5)
    assert not torch.equal(changed, before) and torch.equal(m(e["a"], e["b"]), before)
