"""GPU image metrics (swnerf_image_metrics through swnerf.metrics) against the float64 restatement in
tests/metrics_ref.py, and the two evaluators built on them (runner.render_test, runner.evaluate_dir).
Gates: window sums, S and the reductions are fp64 from fp32 inputs, so the results differ from the restatement only by
summation order, and the map by its fp32 rounding.  Measured on MI355X: per-image SSIM 1.8e-15 on the
synthetic frames and 1.4e-13 on a nearly constant render (R = 3.7e-4, so C2 = 1.3e-10 and var = E[x^2] - mu^2 cancels),
PSNR 7.1e-15 dB, map 2.98e-8 (half an fp32 ulp below 1); each gate is a small multiple of the worst case."""
import ast
import json
import os

import numpy as np
import pytest
import torch

import metrics_ref as M

pytestmark = pytest.mark.gpu

SSIM_TOL = 1e-12         # per-image SSIM, absolute (measured 1.4e-13 at worst)
MAP_TOL = 6e-8           # per-pixel S, absolute (measured 2.98e-8)
PSNR_TOL = 1e-13         # dB (measured 7.1e-15)
MSE_RTOL = 1e-12
MODES = {"skimage": M.SKIMAGE, "gauss11": M.GAUSS11}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sw():
    import swnerf.metrics, swnerf.runner, swnerf.render, swnerf.render_dnerf, swnerf.synth  # noqa
    import swnerf
    return swnerf


def frames(n, h, w, seed=0, noise=0.1):
    r = np.random.default_rng(seed)
    gt = r.random((n, h, w, 3), dtype=np.float32)
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    gt = (0.5 * gt + 0.5 * (0.5 + 0.5 * np.sin(6 * xx + 4 * yy))[None, :, :, None]).astype(np.float32)
    pred = (gt + noise * r.standard_normal(gt.shape)).astype(np.float32)
    return pred, gt


def check(got, ref, what):
    g = {k: got[k].cpu().numpy() for k in ("mse", "psnr", "range", "ssim")}
    for k in ("mse", "psnr", "range", "ssim"):
        assert np.array_equal(np.isnan(g[k]), np.isnan(ref[k])), (what, k, g[k], ref[k])
    np.testing.assert_array_equal(g["range"], ref["range"], err_msg=what)
    np.testing.assert_allclose(g["mse"], ref["mse"], rtol=MSE_RTOL, atol=0, equal_nan=True, err_msg=what)
    np.testing.assert_allclose(g["psnr"], ref["psnr"], rtol=0, atol=PSNR_TOL, equal_nan=True, err_msg=what)
    np.testing.assert_allclose(g["ssim"], ref["ssim"], rtol=0, atol=SSIM_TOL, equal_nan=True, err_msg=what)
    return {k: float(np.nanmax(np.abs(g[k] - ref[k]), initial=0.0)) for k in ("psnr", "ssim")
            if np.isfinite(ref[k]).any()}


SIZES = [(11, 11), (13, 101), (61, 67), (800, 800)]
CASES = [("skimage", (7, 7))] + [(m, hw) for hw in SIZES for m in ("skimage", "gauss11")]   # 7x7 is below the 11x11 window


@pytest.mark.parametrize("mode,hw", CASES)
def test_modes_match_float64_restatement(sw, dev, mode, hw):
    h, w = hw
    n = 1 if h * w > 10000 else 3
    pred, gt = frames(n, h, w, seed=h * 1000 + w)
    got = sw.metrics.image_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), mode=mode)
    err = check(got, M.batch(pred, gt, MODES[mode]), f"{mode} {hw}")
    print(f"[metrics] {mode} {h}x{w}: max |d ssim| {err['ssim']:.3e}, max |d psnr| {err['psnr']:.3e} dB")


def test_frames_with_different_ranges_in_one_batch(sw, dev):
    pred, gt = frames(4, 29, 45, seed=3)
    scale = np.array([1.0, 0.5, 3.0, 255.0], np.float32)[:, None, None, None]
    off = np.array([0.0, 0.25, -1.0, 0.0], np.float32)[:, None, None, None]
    pred, gt = pred * scale + off, gt * scale + off
    for mode in MODES:
        got = sw.metrics.image_metrics(pred, gt, mode=mode)                         # host numpy path
        ref = M.batch(pred, gt, MODES[mode])
        assert len(set(ref["range"].tolist())) == 4
        check(got, ref, mode)


@pytest.mark.parametrize("data_range", [1.0, "gt", "pred_rule"])
@pytest.mark.parametrize("clip", [False, True])
def test_clip_and_range_sources(sw, dev, data_range, clip):
    pred, gt = frames(3, 37, 41, seed=5, noise=0.4)                                 # pred well outside [0, 1]
    if data_range == "pred_rule" and not clip:
        pred = pred * 200.0                                                         # max > 128 and min < -0.5: L = 256
    for mode in MODES:
        got = sw.metrics.image_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), mode=mode,
                                       data_range=data_range, clip_pred=clip)
        ref = M.batch(pred, gt, MODES[mode], data_range=data_range, clip_pred=clip)
        check(got, ref, f"{mode} {data_range} clip={clip}")
    if data_range == "pred_rule":
        assert float(got["range"][0]) == (1.0 if clip else 256.0)


def test_pred_rule_is_over_the_whole_batch_across_chunks(sw, dev):
    pred, gt = frames(5, 16, 20, seed=6)
    pred[3] = np.abs(pred[3]) * 200.0                                               # one frame of one chunk decides L
    got = sw.metrics.image_metrics(pred, gt, mode="gauss11", data_range="pred_rule", chunk_frames=2)
    ref = M.batch(pred, gt, M.GAUSS11, data_range="pred_rule")
    assert set(ref["range"].tolist()) == {255.0}
    check(got, ref, "chunks")


@pytest.mark.parametrize("mode", ["skimage", "gauss11"])
def test_map_matches_restatement(sw, dev, mode):
    for (h, w) in ((61, 67), (13, 101)):
        pred, gt = frames(2, h, w, seed=7)
        got = sw.metrics.image_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), mode=mode,
                                       want_map=True)
        mp = got["map"].cpu().numpy()
        k = 7 if mode == "skimage" else 11
        assert mp.shape == (2, h - k + 1, w - k + 1, 3)
        for i in range(2):
            ref = M.ssim_map(pred[i], gt[i], MODES[mode], M.gt_range(gt[i]))
            d = np.abs(mp[i] - ref)
            assert d.max() <= MAP_TOL, (mode, h, w, i, np.unravel_index(d.argmax(), d.shape), d.max())
            print(f"[metrics] map {mode} {h}x{w}: max |d S| {d.max():.3e}")
        # the per-image SSIM is the mean of its map
        np.testing.assert_allclose(got["ssim"].cpu().numpy(), mp.reshape(2, -1).mean(1, dtype=np.float64), atol=1e-7)


def test_constant_gt_and_nan(sw, dev):
    pred, gt = frames(3, 20, 24, seed=8)
    gt[0] = 0.5                                                                     # R = gt.max() - gt.min() = 0
    pred[2, 4, 5, 1] = np.nan
    for mode in MODES:
        got = sw.metrics.image_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), mode=mode)
        ref = M.batch(pred, gt, MODES[mode])
        assert ref["range"][0] == 0.0 and ref["psnr"][0] == -np.inf
        assert np.isnan(ref["mse"][2]) and np.isnan(ref["psnr"][2]) and np.isnan(ref["ssim"][2])
        check(got, ref, mode)
        g = {k: got[k].cpu().numpy() for k in got}
        assert g["psnr"][0] == -np.inf and np.isnan(g["ssim"][2]) and np.isfinite(g["ssim"][1])


def test_bit_identical_repeats(sw, dev):
    pred, gt = frames(3, 97, 131, seed=9)
    p, g = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    for mode in MODES:
        runs = [sw.metrics.image_metrics(p, g, mode=mode, want_map=True) for _ in range(3)]
        for r in runs[1:]:
            for k in runs[0]:
                assert torch.equal(r[k], runs[0][k]), (mode, k)


def test_skimage_and_notebook_apis(sw, dev):
    pred, gt = frames(2, 40, 44, seed=10, noise=0.2)
    m = sw.metrics
    for i in range(2):
        R = M.gt_range(gt[i])
        s = m.structural_similarity(gt[i], pred[i], win_size=7, multichannel=True, data_range=gt[i].max() - gt[i].min(),
                                    channel_axis=2)
        assert abs(s - M.ssim(pred[i], gt[i], M.SKIMAGE, R)) < SSIM_TOL
        ps = m.peak_signal_noise_ratio(gt[i], pred[i], data_range=R)
        assert abs(ps - M.psnr(M.mse(pred[i], gt[i]), R)) < PSNR_TOL
        cp, cs, cl = m.calculate_metrics(gt[i], pred[i])
        pc = np.clip(pred[i], 0, 1)
        assert cl is None
        assert abs(cp - M.psnr(M.mse(pc, gt[i]), R)) < PSNR_TOL and abs(cs - M.ssim(pc, gt[i], M.SKIMAGE, R)) < SSIM_TOL
    # the notebook: NCHW device tensors, (pred, gt) order, one batch
    pn, gn = (torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2))).to(dev) for a in (pred, gt))
    ref = M.batch(pred, gt, M.GAUSS11, data_range="pred_rule")
    mse = ref["mse"].mean()
    assert abs(float(m.MSE()(pn, gn)) - mse) <= 1e-12 * mse
    assert abs(float(m.PSNR()(pn, gn)) - 10 * np.log10(1 / mse)) < PSNR_TOL
    assert abs(float(m.SSIM()(pn, gn)) - ref["ssim"].mean()) < SSIM_TOL
    np.testing.assert_allclose(m.SSIM()(pn, gn, size_average=False).cpu().numpy(), ref["ssim"], atol=SSIM_TOL)
    e = m.estim_error(pn, gn)
    assert set(e) == {"mse", "psnr", "ssim"} and abs(e["ssim"] - ref["ssim"].mean()) < SSIM_TOL


def _static_kwargs(sw, dev, seeds):
    embed_fn, ic = sw.embedder.get_embedder(10, 3, 0)
    embeddirs_fn, icv = sw.embedder.get_embedder(4, 3, 0)
    nets = []
    for seed, ab in seeds:
        net = sw.model.vallina_NeRF(D=8, W=256, input_ch=ic, input_ch_views=icv, output_ch=5, skips=[4], use_viewdirs=True)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sw.synth.nerf_state_dict(seed, alpha_bias=ab).items()})
        nets.append(net.to(dev).eval())
    q = lambda inputs, viewdirs, network_fn: sw.render.run_network(inputs, viewdirs, network_fn, embed_fn=embed_fn,
                                                                   embeddirs_fn=embeddirs_fn, netchunk=1024 * 64)
    return dict(ndc=False, near=2., far=6., use_viewdirs=True, network_fn=nets[0], network_query_fn=q, N_samples=32,
                N_importance=32, network_fine=nets[1], white_bkgd=True, perturb=False, raw_noise_std=0.)


def test_render_test_end_to_end(sw, dev, tmp_path):
    """nerf/run.py --render_only --render_test on synth nets: the frames of a second pair of nets are the ground truth."""
    H, W = 24, 32
    K = sw.synth.lego_camera(H, W)[0]
    poses = torch.stack([torch.from_numpy(sw.synth.lego_camera(H, W, theta=th)[1]).float() for th in (0.0, 35.0, 70.0)]).to(dev)
    hwf = (H, W, float(K[0, 0]))
    with torch.no_grad():
        gt, _ = sw.render.render_path(poses, hwf, K, 1024 * 32, _static_kwargs(sw, dev, [(11, -0.25), (12, -1.0)]))
        kw = _static_kwargs(sw, dev, [sw.synth.NET_COARSE, sw.synth.NET_FINE])
        rgbs, met = sw.runner.render_test(poses, hwf, K, 1024 * 32, kw, gt, str(tmp_path / "rt"))
    assert rgbs.shape == (3, H, W, 3) and sorted(os.listdir(tmp_path / "rt")) == ["000.png", "001.png", "002.png", "metrics.json"]
    saved = json.loads((tmp_path / "rt" / "metrics.json").read_text())
    assert saved == met and set(saved) == {"psnr", "ssim"} and len(saved["psnr"]) == 3
    for i in range(3):
        p, s, _ = sw.metrics.calculate_metrics(gt[i], rgbs[i])
        assert saved["psnr"][i] == float(p) and saved["ssim"][i] == float(s)
        R = M.gt_range(gt[i])
        pc = np.clip(rgbs[i], 0, 1)
        assert abs(saved["ssim"][i] - M.ssim(pc, gt[i], M.SKIMAGE, R)) < SSIM_TOL
        assert abs(saved["psnr"][i] - M.psnr(M.mse(pc, gt[i]), R)) < PSNR_TOL
    assert all(-1.0 <= s < 1.0 for s in saved["ssim"]) and all(np.isfinite(saved["psnr"]))


def test_evaluate_dir_on_dnerf_render(sw, dev, tmp_path):
    """d_nerf/metrics.ipynb on the estim/ + gt/ directory that render_dnerf.render_path(save_also_gt=True) writes."""
    from swnerf.png import read_png
    H, W = 24, 28
    e10, _ = sw.embedder.get_embedder(10, 3, 0)
    embeddirs_fn, _ = sw.embedder.get_embedder(4, 3, 0)
    embedtime_fn, _ = sw.embedder.get_embedder(10, 1, 0)
    dn = sw.model.NeRF.get_by_name("direct_temporal", D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27,
                                   input_ch_time=21, use_viewdirs=True, embed_fn=e10, zero_canonical=True)
    dn.load_state_dict({k: torch.from_numpy(v) for k, v in sw.synth.dnerf_state_dict(sw.synth.NET_DNERF[0]).items()})
    dn = dn.to(dev).eval()
    qd = lambda inputs, viewdirs, ts, network_fn: sw.render_dnerf.run_network(
        inputs, viewdirs, ts, network_fn, embed_fn=e10, embeddirs_fn=embeddirs_fn, embedtime_fn=embedtime_fn,
        netchunk=1024 * 64, embd_time_discr=True)
    kw = dict(ndc=False, near=2., far=6., use_viewdirs=True, network_fn=dn, network_query_fn=qd, N_samples=32,
              N_importance=32, white_bkgd=True, perturb=False, raw_noise_std=0.)
    K = sw.synth.lego_camera(H, W)[0]
    poses = torch.stack([torch.from_numpy(sw.synth.lego_camera(H, W, theta=th)[1]).float() for th in (0.0, 30.0, 60.0)]).to(dev)
    _, gt = frames(3, H, W, seed=11)
    with torch.no_grad():
        sw.render_dnerf.render_path(poses, [0.0, 0.5, 1.0], (H, W, float(K[0, 0])), 1024 * 32, kw, gt_imgs=gt,
                                    savedir=str(tmp_path), save_also_gt=True)
    errors = sw.runner.evaluate_dir(str(tmp_path))
    assert ast.literal_eval((tmp_path / "metrics.txt").read_text()) == errors and set(errors) == {"mse", "psnr", "ssim"}
    est = np.stack([read_png(str(tmp_path / "estim" / f"{i:03d}.png")) / 255. for i in (1, 2)]).astype(np.float32)
    g = np.stack([read_png(str(tmp_path / "gt" / f"{i:03d}.png")) / 255. for i in (1, 2)]).astype(np.float32)
    ref = M.batch(est, g, M.GAUSS11, data_range="pred_rule")
    assert abs(errors["mse"] - ref["mse"].mean()) <= 1e-12 * ref["mse"].mean()
    assert abs(errors["psnr"] - 10 * np.log10(1 / ref["mse"].mean())) < PSNR_TOL
    assert abs(errors["ssim"] - ref["ssim"].mean()) < SSIM_TOL
