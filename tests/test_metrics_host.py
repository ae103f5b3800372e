"""Host-side checks of the image-metrics feature (swnerf.metrics, swnerf.png.read_png, runner.render_test /
evaluate_dir): the float64 restatement against scipy and known answers, the PNG decoder, argument refusals, the C-ABI
exports and the output file formats.  No GPU."""
import ast
import json
import os
import struct
import zlib

import numpy as np
import pytest

import metrics_ref as M


def _rng(seed=0):
    return np.random.default_rng(seed)


# ---- the restatement --------------------------------------------------------------------------------------------
def test_skimage_mode_equals_uniform_filter_then_crop():
    ndimage = pytest.importorskip("scipy.ndimage")
    r = _rng(1)
    x = r.random((23, 31, 3))
    y = np.clip(x + 0.1 * r.standard_normal(x.shape), 0, 1)
    R = 1.0
    S = np.empty_like(x)
    for c in range(3):                     # skimage: per channel, uniform_filter(size=7, mode="reflect"), sample covariance
        f = lambda a: ndimage.uniform_filter(a, size=7, mode="reflect")
        X, Y = x[..., c], y[..., c]
        ux, uy = f(X), f(Y)
        vx = 49 / 48 * (f(X * X) - ux * ux)
        vy = 49 / 48 * (f(Y * Y) - uy * uy)
        vxy = 49 / 48 * (f(X * Y) - ux * uy)
        C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
        S[..., c] = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    crop = S[3:-3, 3:-3]
    np.testing.assert_allclose(M.ssim_map(y, x, M.SKIMAGE, R), crop, rtol=0, atol=1e-12)
    assert abs(M.ssim(y, x, M.SKIMAGE, R) - np.mean([crop[..., c].mean() for c in range(3)])) < 1e-13


def test_known_answers():
    x = _rng(2).random((20, 17, 3))
    for mode in (M.SKIMAGE, M.GAUSS11):
        assert abs(M.ssim(x, x, mode, 1.0) - 1.0) < 1e-12
    g = np.full((9, 9, 3), 0.25, np.float32)
    assert abs(M.psnr(M.mse(g + np.float32(0.125), g), 1.0) - 20 * np.log10(8.0)) < 1e-9
    assert abs(M.gauss_weights().sum() - 1.0) < 1e-15
    assert M.gauss_weights().argmax() == 5 and np.allclose(M.gauss_weights(), M.gauss_weights()[::-1])
    assert M.pred_rule(np.array([0.0, 1.0])) == 1.0 and M.pred_rule(np.array([-1.0, 200.0])) == 256.0


# ---- read_png -------------------------------------------------------------------------------------------------------
def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def _filter_row(ft, cur, prev, bpp):
    cur, prev = cur.astype(np.int32), prev.astype(np.int32)
    out = np.zeros_like(cur)
    for x in range(len(cur)):
        a = cur[x - bpp] if x >= bpp else 0
        b = prev[x]
        c = prev[x - bpp] if x >= bpp else 0
        if ft == 0:
            p = 0
        elif ft == 1:
            p = a
        elif ft == 2:
            p = b
        elif ft == 3:
            p = (a + b) >> 1
        else:
            q = a + b - c
            pa, pb, pc = abs(q - a), abs(q - b), abs(q - c)
            p = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
        out[x] = (cur[x] - p) & 0xff
    return out.astype(np.uint8)


def _png(img, filters, n_idat=2, color=None, depth=8, interlace=0):
    h, w, c = img.shape
    color = {3: 2, 4: 6}[c] if color is None else color
    rows, prev = [], np.zeros(w * c, np.uint8)
    for y in range(h):
        cur = img[y].reshape(-1)
        ft = filters[y % len(filters)]
        rows.append(bytes([ft]) + _filter_row(ft, cur, prev, c).tobytes())
        prev = cur
    z = zlib.compress(b"".join(rows), 9)
    cut = [len(z) * k // n_idat for k in range(n_idat + 1)]
    idat = b"".join(_chunk(b"IDAT", z[cut[k]:cut[k + 1]]) for k in range(n_idat))
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color, 0, 0, interlace))
            + _chunk(b"tEXt", b"Software\x00test") + idat + _chunk(b"IEND", b""))


def test_read_png_round_trips_write_png(tmp_path):
    from swnerf.png import write_png, read_png
    img = (_rng(3).random((13, 21, 3)) * 255).astype(np.uint8)
    write_png(str(tmp_path / "a.png"), img)
    np.testing.assert_array_equal(read_png(str(tmp_path / "a.png")), img)


@pytest.mark.parametrize("channels", [3, 4])
def test_read_png_decodes_every_filter_and_split_idat(tmp_path, channels):
    from swnerf.png import read_png
    img = (_rng(4).random((17, 11, channels)) * 255).astype(np.uint8)
    img[5:9] = 250                                                  # saturating sums exercise the & 0xff wrap
    p = tmp_path / "f.png"
    p.write_bytes(_png(img, filters=[1, 2, 3, 4, 0], n_idat=2))
    out = read_png(str(p))
    assert out.shape == (17, 11, 3) and out.dtype == np.uint8
    np.testing.assert_array_equal(out, img[..., :3])


@pytest.mark.parametrize("kw", [dict(depth=16), dict(color=0), dict(color=3), dict(interlace=1)])
def test_read_png_refuses_other_formats(tmp_path, kw):
    from swnerf.png import read_png
    p = tmp_path / "x.png"
    p.write_bytes(_png(np.zeros((4, 4, 3), np.uint8), [0], 1, **kw))
    with pytest.raises(ValueError):
        read_png(str(p))
    p.write_bytes(b"GIF89a")
    with pytest.raises(ValueError):
        read_png(str(p))


# ---- argument refusals (raised before any GPU work) ----------------------------------------------------------------
def test_skimage_api_refusals():
    from swnerf import metrics
    a = np.zeros((16, 16, 3), np.float32)
    ssim = metrics.structural_similarity
    for kw in (dict(win_size=5), dict(gaussian_weights=True), dict(full=True), dict(gradient=True), dict(K1=0.02),
               dict(use_sample_covariance=False), dict(channel_axis=0), dict(foo=1)):
        with pytest.raises(NotImplementedError):
            ssim(a, a, data_range=1.0, **{"channel_axis": 2, **kw})
    with pytest.raises(NotImplementedError):
        ssim(a.astype(np.uint8), a.astype(np.uint8), data_range=255, channel_axis=2)
    with pytest.raises(NotImplementedError):
        ssim(np.zeros((16, 16, 4), np.float32), np.zeros((16, 16, 4), np.float32), data_range=1.0, channel_axis=2)
    with pytest.raises(ValueError):
        ssim(a, a, channel_axis=2)                                                  # no data_range
    with pytest.raises(ValueError):
        ssim(a, a[:15], data_range=1.0, channel_axis=2)
    with pytest.raises(ValueError):
        metrics.peak_signal_noise_ratio(a, a[:, :15])
    with pytest.raises(ValueError):
        metrics.peak_signal_noise_ratio(a, a)                                       # no data_range
    with pytest.raises(ValueError):
        metrics.image_metrics(a[:6], a[:6], mode="skimage")                         # below the window
    with pytest.raises(ValueError):
        metrics.image_metrics(a[:10], a[:10], mode="gauss11")
    with pytest.raises(ValueError):
        metrics.image_metrics(a, a, mode="box")
    with pytest.raises(ValueError):
        metrics.image_metrics(a, a, mode="skimage", data_range="max")
    with pytest.raises(NotImplementedError):
        metrics.SSIM()(a, a, w_size=7)


def test_new_exports_and_workspace_sizes():
    import ctypes
    from swnerf import _lib
    for name in ("swnerf_metrics_workspace_bytes", "swnerf_image_metrics"):
        assert name in _lib.EXPORTS
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert L.swnerf_version() == 112
    f = L.swnerf_metrics_workspace_bytes
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int64] * 3 + [ctypes.c_int]
    assert f(4, 6, 100, 0) == 0 and f(4, 100, 10, 1) == 0 and f(0, 100, 100, 0) == 0 and f(1, 8, 8, 2) == 0
    assert f(1, 7, 7, 0) > 0 and f(1, 11, 11, 1) > 0
    assert f(200, 800, 800, 0) >= 200 * 8 * 13 * 50                   # at least one fp64 partial per 64 x 16 tile


# ---- output formats ------------------------------------------------------------------------------------------------
def test_render_test_writes_metrics_json(tmp_path, monkeypatch):
    from swnerf import runner, render, metrics
    frames = np.full((2, 8, 8, 3), 0.5, np.float32)
    monkeypatch.setattr(render, "render_path", lambda *a, **k: (frames, frames[..., 0]))
    monkeypatch.setattr(metrics, "batch_metrics", lambda gts, preds: ([31.5, 29.25], [0.875, 0.5]))
    rgbs, out = runner.render_test(None, (8, 8, 10.0), None, 64, {}, frames, str(tmp_path / "t"))
    assert rgbs is frames and out == {"psnr": [31.5, 29.25], "ssim": [0.875, 0.5]}
    text = (tmp_path / "t" / "metrics.json").read_text()
    assert json.loads(text) == out
    assert text == json.dumps(out, indent=4) and "lpips" not in text


def test_evaluate_dir_reads_pngs_and_writes_metrics_txt(tmp_path, monkeypatch):
    from swnerf import runner, metrics
    from swnerf.png import write_png
    seen = {}

    def fake(estim, gt):
        seen["estim"], seen["gt"] = estim, gt
        return {"mse": 0.25, "psnr": 6.020599913279624, "ssim": 0.5}
    monkeypatch.setattr(metrics, "estim_error", fake)
    r = _rng(5)
    imgs = {}
    for sub in ("estim", "gt"):
        os.makedirs(tmp_path / sub)
        for i in range(3):
            imgs[sub, i] = (r.random((9, 12, 3)) * 255).astype(np.uint8)
            write_png(str(tmp_path / sub / f"{i:03d}.png"), imgs[sub, i])
    out = runner.evaluate_dir(str(tmp_path))
    assert seen["estim"].shape == (2, 3, 9, 12) and seen["estim"].dtype == np.float32      # 000.png skipped, NCHW
    np.testing.assert_array_equal(seen["gt"][1], (np.transpose(imgs["gt", 2], (2, 0, 1)) / 255.).astype(np.float32))
    text = (tmp_path / "metrics.txt").read_text()
    assert text == str(out) and ast.literal_eval(text) == {"mse": 0.25, "psnr": 6.020599913279624, "ssim": 0.5}
