"""LPIPS without a GPU: weight loading and its errors, the float64 restatement (tests/lpips_ref.py) against hand-computed
values, the seeded nets' dead-unit share, and the runners' output with and without weights through their injection seams."""
import ast
import json
import os

import numpy as np
import pytest
import torch

import lpips_ref as R



def _save_dir(tmp_path, net):
    trunk, lin = R.seeded_weights(net)
    d = tmp_path / f"weights_{net}"
    os.makedirs(d)
    torch.save(trunk, d / ("alexnet-owt-7be5be79.pth" if net == "alex" else "vgg16-397923af.pth"))
    torch.save(lin, d / f"{net}.pth")
    return d, trunk, lin


# ---- weight loading -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_weights_from_dicts_paths_and_directory(tmp_path, monkeypatch, net):
    from swnerf import lpips, metrics
    monkeypatch.delenv("SWNERF_LPIPS_DIR", raising=False)
    d, trunk, lin = _save_dir(tmp_path, net)
    trunk_file = [f for f in os.listdir(d) if f != f"{net}.pth"][0]
    loaded = [lpips.load_weights(net, (trunk, lin)),
              lpips.load_weights(net, (str(d / trunk_file), str(d / f"{net}.pth"))),
              lpips.load_weights(net, (trunk, str(d / f"{net}.pth"))),
              lpips.load_weights(net, str(d)),
              lpips.load_weights(net, None, args=type("A", (), {"lpips_weights": str(d)})())]
    monkeypatch.setenv("SWNERF_LPIPS_DIR", str(d))
    loaded.append(lpips.load_weights(net))
    for convs, lins in loaded:
        assert len(convs) == len(R.CONVS[net]) and [l.numel() for l in lins] == R.CHANNELS[net]
        for (i, ci, co, k, _, _), (w, b) in zip(R.CONVS[net], convs):
            assert torch.equal(w, trunk[f"features.{i}.weight"]) and torch.equal(b, trunk[f"features.{i}.bias"])
            assert w.shape == (co, ci, k, k) and w.dtype == torch.float32 and w.is_contiguous()
        for j, l in enumerate(lins):
            assert torch.equal(l, lin[f"lin{j}.model.1.weight"].reshape(-1))
    m = metrics.LPIPS(net, weights=(trunk, lin))                           # the class reads them the same way
    assert m.net == net and lpips.tap_channels(net) == R.CHANNELS[net]
    assert metrics.LPIPS is lpips.LPIPS and metrics.LPIPS_notebook is lpips.LPIPS_notebook


def test_the_environment_directory_goes_before_args(tmp_path, monkeypatch):
    from swnerf import lpips
    d, trunk, lin = _save_dir(tmp_path, "alex")
    monkeypatch.setenv("SWNERF_LPIPS_DIR", str(d))
    convs, _ = lpips.load_weights("alex", None, args=type("A", (), {"lpips_weights": str(tmp_path / "nowhere")})())
    assert torch.equal(convs[0][0], trunk["features.0.weight"])


def test_missing_key_wrong_shape_and_absent_weights(tmp_path, monkeypatch):
    from swnerf import metrics
    monkeypatch.delenv("SWNERF_LPIPS_DIR", raising=False)
    trunk, lin = R.seeded_weights("alex")
    bad = {k: v for k, v in trunk.items() if k != "features.6.bias"}
    with pytest.raises(ValueError, match=r"features\.6\.bias"):
        metrics.LPIPS("alex", weights=(bad, lin))
    bad = dict(trunk)
    bad["features.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match=r"features\.3\.weight.*\(192, 64, 3, 3\).*\(192, 64, 5, 5\)"):
        metrics.LPIPS("alex", weights=(bad, lin))
    bad = {k: v for k, v in lin.items() if k != "lin4.model.1.weight"}
    with pytest.raises(ValueError, match=r"lin4\.model\.1\.weight"):
        metrics.LPIPS("alex", weights=(trunk, bad))
    bad = dict(lin)
    bad["lin1.model.1.weight"] = torch.zeros(1, 64, 1, 1)
    with pytest.raises(ValueError, match=r"lin1\.model\.1\.weight"):
        metrics.LPIPS("alex", weights=(trunk, bad))
    with pytest.raises(ValueError, match=r"features\.0\.weight"):
        metrics.LPIPS("vgg", weights=({}, {}))
    for net, trunk_name in (("alex", "alexnet-owt-7be5be79.pth"), ("vgg", "vgg16-397923af.pth")):
        with pytest.raises(FileNotFoundError) as e:
            metrics.LPIPS(net)
        text = str(e.value)
        assert trunk_name in text and f"lpips/weights/v0.1/{net}.pth" in text and "SWNERF_LPIPS_DIR" in text
        with pytest.raises(FileNotFoundError, match=f"{net}.pth"):
            metrics.LPIPS(net, weights=str(tmp_path))                       # a directory without the files
    with pytest.raises(FileNotFoundError):
        metrics.LPIPS("alex", weights=(str(tmp_path / "a.pth"), lin))
    with pytest.raises(ValueError, match="squeeze"):
        metrics.LPIPS("squeeze", weights=(trunk, lin))
    with pytest.raises(TypeError):
        metrics.LPIPS("alex", weights=(trunk,))


def test_weight_files_are_read_as_plain_tensors_only(tmp_path, monkeypatch):
    """torch.load(..., map_location='cpu', weights_only=True): no code in a weight file runs"""
    from swnerf import lpips
    seen = []
    real = torch.load

    def spy(f, *a, **k):
        seen.append(k)
        return real(f, *a, **k)
    d, _, _ = _save_dir(tmp_path, "alex")
    monkeypatch.setattr(torch, "load", spy)
    lpips.load_weights("alex", str(d))
    assert len(seen) == 2 and all(k.get("weights_only") is True and k.get("map_location") == "cpu" for k in seen)


def test_input_refusals_come_before_the_gpu():
    from swnerf import metrics
    m = metrics.LPIPS("alex", weights=R.seeded_weights("alex"))
    a = np.zeros((2, 3, 40, 40), np.float32)
    with pytest.raises(ValueError):
        m(a, a[:1])
    with pytest.raises(ValueError):
        m(a, a, layout="nhwc")                                              # 40 channels
    with pytest.raises(ValueError):
        m(a, a, layout="chw")
    with pytest.raises(NotImplementedError):
        m(a.astype(np.int32), a.astype(np.int32))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no GPU"):
            m(a, a)


# ---- the restatement against hand-computed values -------------------------------------------------------------------------
def test_ref_layer_by_hand():
    f0 = torch.tensor([3.0, 4.0], dtype=torch.float64).view(1, 2, 1, 1)     # unit vector (0.6, 0.8)
    f1 = torch.tensor([1.0, 0.0], dtype=torch.float64).view(1, 2, 1, 1)     # unit vector (1, 0)
    lin = torch.tensor([2.0, 0.5], dtype=torch.float64)
    assert abs(float(R.layer(f0, f1, lin)) - (2.0 * 0.16 + 0.5 * 0.64)) < 1e-9      # the 1e-10 in the denominators
    # two pixels, one of them all zero in f1 (the eps path: 0 / 1e-10 = 0): mean of (0.64, 2 * 0.36 + 0.5 * 0.64) over the pixels
    f0 = torch.tensor([[3.0, 3.0], [4.0, 4.0]], dtype=torch.float64).view(1, 2, 1, 2)
    f1 = torch.tensor([[1.0, 0.0], [0.0, 0.0]], dtype=torch.float64).view(1, 2, 1, 2)
    assert abs(float(R.layer(f0, f1, lin)) - 0.5 * (0.64 + (2.0 * 0.36 + 0.5 * 0.64))) < 1e-9
    assert float(R.layer(f0, f0, lin)) == 0.0


def test_ref_toy_net_by_hand():
    """one 1x1 convolution 3 -> 2 with ReLU as the only tap, 1x2 images: every number below is worked out by hand"""
    toy = ([(0, 3, 2, 1, 1, 0)], [("tap", 0)])
    trunk = {"features.0.weight": torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, -1.0]]).view(2, 3, 1, 1),
             "features.0.bias": torch.tensor([0.0, 0.5])}
    lin = {"lin0.model.1.weight": torch.tensor([1.0, 4.0]).view(1, 2, 1, 1)}
    # chosen so that the scaled inputs are simple: x = shift + scale * s  ->  scaling(x) = s
    sh, sc = torch.tensor(R.SHIFT, dtype=torch.float64), torch.tensor(R.SCALE, dtype=torch.float64)
    s0 = torch.tensor([[3.0, 0.0], [3.5, -2.0], [0.0, 1.0]], dtype=torch.float64)           # [channel][pixel]
    s1 = torch.tensor([[0.0, 1.0], [0.5, 0.0], [0.0, 0.5]], dtype=torch.float64)
    in0 = (sh.view(3, 1) + sc.view(3, 1) * s0).view(1, 3, 1, 2)
    in1 = (sh.view(3, 1) + sc.view(3, 1) * s1).view(1, 3, 1, 2)
    assert torch.allclose(R.scaling(in0).view(3, 2), s0, atol=1e-12)
    # features: image 0 pixel 0: relu(3, 3.5 - 0 + .5) = (3, 4); pixel 1: relu(0, -2 - 1 + .5) = (0, 0)
    #           image 1 pixel 0: relu(0, .5 + .5) = (0, 1);      pixel 1: relu(1, 0 - .5 + .5) = (1, 0)
    t0 = R.taps(toy, trunk, R.scaling(in0))[0].view(2, 2)
    assert torch.allclose(t0, torch.tensor([[3.0, 0.0], [4.0, 0.0]], dtype=torch.float64), atol=1e-12)
    # pixel 0: (0.6, 0.8) against (0, 1): 1 * 0.36 + 4 * 0.04 = 0.52; pixel 1: (0, 0) against (1, 0): 1
    want = 0.5 * (0.52 + 1.0)
    assert abs(float(R.lpips_ref(toy, trunk, lin, in0, in1)) - want) < 1e-9
    assert abs(float(R.lpips_ref(toy, trunk, lin, in0, in1, fp32=True)) - want) < 1e-6
    # normalize=True maps x to 2x - 1 first
    assert torch.allclose(R.lpips_ref(toy, trunk, lin, (in0 + 1) / 2, (in1 + 1) / 2, normalize=True), torch.tensor([want], dtype=torch.float64), atol=1e-9)


def test_ref_trunk_shapes():
    for net, (h, w), want in (("alex", (35, 47), [(8, 11), (3, 5), (1, 2), (1, 2), (1, 2)]),
                              ("vgg", (18, 21), [(18, 21), (9, 10), (4, 5), (2, 2), (1, 1)])):
        trunk, _ = R.seeded_weights(net)
        t = R.taps(net, trunk, torch.zeros(1, 3, h, w, dtype=torch.float64))
        assert [tuple(x.shape[1:]) for x in t] == [(c,) + hw for c, hw in zip(R.CHANNELS[net], want)]


@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_seeded_nets_keep_half_of_every_tap_alive(net):
    trunk, _ = R.seeded_weights(net)
    for h, w in R.E2E_SIZES[net]:
        gt, pred = R.seeded_images(3, h, w, R.IMG_SEED)
        for x in (gt, pred, 2 * gt - 1, 2 * pred - 1):
            assert max(R.dead_fractions(net, trunk, x)) <= 0.5


def test_live_bytes_and_plan_follow_the_reference_shapes():
    from swnerf import lpips
    for net in ("alex", "vgg"):
        assert [(c[0], c[1], c[2], c[3], c[4], c[5]) for c in lpips.CONVS[net]] == R.CONVS[net]
        taps = [p for p, (tap, _) in enumerate(R.AFTER[net]) if tap]
        assert list(lpips.TAPS[net]) == taps
        pools = {p + 1: win for p, (_, win) in enumerate(R.AFTER[net]) if win}
        assert lpips.POOL_BEFORE[net] == pools
    m = lpips.LPIPS("vgg", weights=R.seeded_weights("vgg"))
    # conv1_2 at 800 x 800: 64 channels in and out, two images, 4 bytes
    assert m.live_bytes(800, 800) == 2 * 4 * (800 * 800 * 64 * 2)


# ---- the runners: with weights the key is there, without them nothing changes ------------------------------------------
class _FakeLPIPS:
    made = []

    def __init__(self, net="alex", weights=None, device=None, args=None):
        self.net, self.weights = net, weights
        _FakeLPIPS.made.append(self)


def test_render_test_with_and_without_lpips_weights(tmp_path, monkeypatch):
    from swnerf import runner, render, metrics
    frames = np.full((2, 8, 8, 3), 0.5, np.float32)
    seen = {}

    def fake_render_path(poses, hwf, K, chunk, render_kwargs, **k):
        seen["kwargs"] = render_kwargs
        return frames, frames[..., 0]

    def fake_batch(gts, preds, lpips_model=None):
        seen["model"] = lpips_model
        return ([31.5, 29.25], [0.875, 0.5]) if lpips_model is None else ([31.5, 29.25], [0.875, 0.5], [0.125, 0.25])
    monkeypatch.setattr(render, "render_path", fake_render_path)
    monkeypatch.setattr(metrics, "batch_metrics", fake_batch)
    monkeypatch.setattr(metrics, "LPIPS", _FakeLPIPS)
    _, out = runner.render_test(None, (8, 8, 10.0), None, 64, {}, frames, str(tmp_path / "plain"))
    plain = (tmp_path / "plain" / "metrics.json").read_text()
    assert out == {"psnr": [31.5, 29.25], "ssim": [0.875, 0.5]} and plain == json.dumps(out, indent=4) and "lpips" not in plain
    assert seen["model"] is None
    for name, kw, rk in (("arg", {"lpips_weights": "W"}, {"near": 2.0}), ("kwargs", {}, {"near": 2.0, "lpips_weights": "W"})):
        _, out = runner.render_test(None, (8, 8, 10.0), None, 64, rk, frames, str(tmp_path / name), **kw)
        assert out == {"psnr": [31.5, 29.25], "ssim": [0.875, 0.5], "lpips": [0.125, 0.25]}
        assert json.loads((tmp_path / name / "metrics.json").read_text()) == out
        assert isinstance(seen["model"], _FakeLPIPS) and seen["model"].net == "alex" and seen["model"].weights == "W"
        assert seen["kwargs"] == {"near": 2.0}                              # the renderer never sees the key


def test_evaluate_dir_with_and_without_lpips_weights(tmp_path, monkeypatch):
    from swnerf import runner, metrics
    from swnerf.png import write_png
    seen = {}

    class FakeNotebook:
        def __init__(self, weights=None, device=None, args=None):
            self.weights = weights

    def fake(estim, gt, lpips_model=None):
        seen["model"] = lpips_model
        e = {"mse": 0.25, "psnr": 6.020599913279624, "ssim": 0.5}
        if lpips_model is not None:
            e["lpips"] = 0.375
        return e
    monkeypatch.setattr(metrics, "estim_error", fake)
    monkeypatch.setattr(metrics, "LPIPS_notebook", FakeNotebook)
    r = np.random.default_rng(5)
    for sub in ("estim", "gt"):
        os.makedirs(tmp_path / sub)
        for i in range(3):
            write_png(str(tmp_path / sub / f"{i:03d}.png"), (r.random((9, 12, 3)) * 255).astype(np.uint8))
    out = runner.evaluate_dir(str(tmp_path))
    text = (tmp_path / "metrics.txt").read_text()
    assert text == str(out) == "{'mse': 0.25, 'psnr': 6.020599913279624, 'ssim': 0.5}" and seen["model"] is None
    for kw in ({"lpips_weights": "W"}, {"args": type("A", (), {"lpips_weights": "W"})()}):
        out = runner.evaluate_dir(str(tmp_path), **kw)
        assert ast.literal_eval((tmp_path / "metrics.txt").read_text()) == out == {"mse": 0.25, "psnr": 6.020599913279624, "ssim": 0.5, "lpips": 0.375}
        assert isinstance(seen["model"], FakeNotebook) and seen["model"].weights == "W"


def test_the_three_kernels_are_exported_and_refuse_bad_workspace_sizes():
    from swnerf import _lib
    for name in ("swnerf_conv2d_pack", "swnerf_conv2d_nhwc", "swnerf_maxpool2d_nhwc", "swnerf_lpips_layer_workspace_bytes", "swnerf_lpips_layer"):
        assert name in _lib.EXPORTS
    L = _lib.lib()
    f = L.swnerf_lpips_layer_workspace_bytes
    assert f(0, 4, 4) == 0 and f(1, 0, 4) == 0 and f(1, 4, (1 << 20) + 1) == 0
    assert f(1, 1, 1) == 8 and f(3, 800, 800) == 3 * 8 * 256


def test_argument_refusals_name_the_argument():
    """SWNERF_E_ARG with a message, before anything touches a device (the pointers are never followed)"""
    from swnerf import _lib
    L = _lib.lib()
    p = 4096                                                                # a non-NULL, aligned stand-in for every pointer

    def conv(n=1, h=8, w=8, cin=3, cout=4, k=3, s=1, pad=1, act=_lib.ACT_RELU, inp=p):
        return L.swnerf_conv2d_nhwc(inp, n, h, w, cin, p, None, cout, k, s, pad, act, p, None)
    for kw, word in ((dict(k=0), "kernel size"), (dict(k=12), "kernel size"), (dict(s=0), "stride"), (dict(s=5), "stride"),
                     (dict(pad=-1), "padding"), (dict(pad=6), "padding"), (dict(cin=0), "channel"), (dict(cout=0), "channel"),
                     (dict(act=_lib.ACT_ELU), "activation"), (dict(n=-1), "image count"), (dict(h=0), "side"),
                     (dict(h=2, k=5, pad=1), "window"), (dict(inp=None), "NULL"), (dict(inp=p + 2), "aligned")):
        assert conv(**kw) == _lib.E_ARG, kw
        assert word in L.swnerf_last_error().decode(), (kw, L.swnerf_last_error())
    assert conv(n=0, inp=None) == 0                                         # an empty batch is a no-op
    assert L.swnerf_conv2d_pack(p, 4, 3, 12, p, None) == _lib.E_ARG and L.swnerf_conv2d_pack(None, 4, 3, 3, p, None) == _lib.E_ARG
    for args, word in (((p, 1, 8, 8, 4, 4, p, None), "window"), ((p, 1, 2, 8, 4, 3, p, None), "window"), ((p, 1, 8, 8, 0, 2, p, None), "channels"),
                       ((None, 1, 8, 8, 4, 2, p, None), "NULL")):
        assert L.swnerf_maxpool2d_nhwc(*args) == _lib.E_ARG and word in L.swnerf_last_error().decode(), args
    assert L.swnerf_maxpool2d_nhwc(None, 0, 8, 8, 4, 2, None, None) == 0
    for args, word in (((p, p, p, 1, 0, 4, 8, 0, p, p, None, None), "side"), ((p, p, p, 1, 4, 4, 0, 0, p, p, None, None), "channels"),
                       ((p, p, p, 1, 4, 4, 8, 0, None, p, None, None), "NULL"), ((p, p, p, 1, 4, 4, 8, 0, p + 4, p, None, None), "8-byte")):
        assert L.swnerf_lpips_layer(*args) == _lib.E_ARG and word in L.swnerf_last_error().decode(), args
