"""swnerf.images on the GPU: the PNG unfilter bit for bit against png._unfilter, the area down-scale against the float64
statement of tests/images_ref.py, and load_pngs on files.

Unfilter shapes are the smallest that reach each hazard of the skewed wavefront (one workgroup per image, a band of 256 rows,
thread r at pixel x = s - r): (1,1); (3,5); (17,31) odd sizes; (5,600) a row far longer than the band is tall; (257,9) crosses a
row band and is taller than wide; (300,70) a wavefront that never fills.

Resize bounds, for data in [0, 1] and truth T in float64 from float32(u / 255.) inputs: power-of-two integer factors are EXACT
(a sum of at most 64 float32 values within a 2^8 range is exact in fp64 and the scale is a power of two, so the result is
float32(T)); fractional factors are within 2^-24 (one rounding to fp32 is <= 2^-25, the fp64 accumulation error below 2^-45)."""
import numpy as np
import pytest
import torch

import images_ref
import png_ref
from swnerf import _lib, images, png

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (3, 5), (17, 31), (5, 600), (257, 9), (300, 70)]
DEV = "cuda:0"


def _host_unfilter(rows, H, W, c):
    return png._unfilter(rows.tobytes(), H, W, c).reshape(H, W, c)


@pytest.fixture(scope="module")
def pictures():
    return {(H, W, c): png_ref.image(H, W, c, seed=H * 7 + W + c) for (H, W) in SHAPES for c in (3, 4)}


@pytest.mark.parametrize("bpp", [3, 4])
@pytest.mark.parametrize("H,W", SHAPES)
def test_unfilter_every_type_alone_and_mixed(pictures, H, W, bpp):
    """each filter type on every row (so Up, Average and Paeth also meet row 0 with its zero row above), then per-row random types"""
    img = pictures[(H, W, bpp)]
    kinds = [0, 1, 2, 3, 4, png_ref.row_types(H, seed=H + W)]
    rows = np.stack([png_ref.filter_rows(img, t) for t in kinds])
    np.testing.assert_array_equal(_host_unfilter(rows[5], H, W, bpp), img)                       # the reference of the reference
    out = images.unfilter(torch.from_numpy(rows.reshape(len(kinds), -1)).to(DEV), H, W, bpp)
    assert out.dtype == torch.uint8 and out.shape == (len(kinds), H, W, bpp) and out.device == torch.device(DEV)
    got = out.cpu().numpy()
    for k in range(len(kinds)):
        np.testing.assert_array_equal(got[k], img, err_msg=f"types {k}")


@pytest.mark.parametrize("bpp", [3, 4])
def test_unfilter_three_images_with_different_types(bpp):
    H, W = 17, 31
    imgs = [png_ref.image(H, W, bpp, seed=50 + k) for k in range(3)]
    rows = np.stack([png_ref.filter_rows(im, png_ref.row_types(H, seed=60 + k)) for k, im in enumerate(imgs)])
    flat = torch.from_numpy(rows.reshape(-1)).to(DEV)                                            # a flat run of bytes is accepted
    np.testing.assert_array_equal(images.unfilter(flat, H, W, bpp).cpu().numpy(), np.stack(imgs))
    for k in range(3):
        np.testing.assert_array_equal(_host_unfilter(rows[k], H, W, bpp), imgs[k])


def test_unfilter_rgba_into_an_unaligned_output():
    """the C entry point on an `out` that is not 4-byte aligned: pixels are stored byte by byte"""
    H, W, n = 9, 13, 2
    imgs = np.stack([png_ref.image(H, W, 4, seed=70 + k) for k in range(n)])
    rows = np.stack([png_ref.filter_rows(im, png_ref.row_types(H, seed=80 + k)) for k, im in enumerate(imgs)])
    f = torch.from_numpy(rows.reshape(-1)).to(DEV)
    buf = torch.zeros(n * H * W * 4 + 8, dtype=torch.uint8, device=DEV)
    out, status = buf[1:1 + n * H * W * 4], torch.full((n,), -1, dtype=torch.int32, device=DEV)
    assert out.data_ptr() % 4 == 1
    _lib.check(_lib.lib().swnerf_png_unfilter(_lib.ptr(f), n, H, W, 4, _lib.ptr(out), _lib.ptr(status), _lib.stream_of(out)), "png_unfilter")
    np.testing.assert_array_equal(out.cpu().numpy().reshape(n, H, W, 4), imgs)
    assert status.tolist() == [0, 0] and buf[0].item() == 0 and buf[1 + n * H * W * 4:].sum().item() == 0


def test_bad_type_byte_is_reported_and_the_other_images_are_exact():
    H, W, bpp = 17, 31, 4
    imgs = [png_ref.image(H, W, bpp, seed=90 + k) for k in range(3)]
    rows = np.stack([png_ref.filter_rows(im, png_ref.row_types(H, seed=95 + k)) for k, im in enumerate(imgs)])
    rows[1, 7, 0] = 5
    f = torch.from_numpy(rows.reshape(3, -1)).to(DEV)
    out = torch.zeros((3, H, W, bpp), dtype=torch.uint8, device=DEV)
    status = torch.full((3,), -1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().swnerf_png_unfilter(_lib.ptr(f), 3, H, W, bpp, _lib.ptr(out), _lib.ptr(status), _lib.stream_of(out)), "png_unfilter")
    assert status.tolist() == [0, 8, 0]
    np.testing.assert_array_equal(out[0].cpu().numpy(), imgs[0])
    np.testing.assert_array_equal(out[2].cpu().numpy(), imgs[2])
    with pytest.raises(ValueError, match="image 1.*row 7"):
        images.unfilter(f, H, W, bpp)
    assert _lib.lib().swnerf_png_unfilter(_lib.ptr(f), 3, H, W, 2, _lib.ptr(out), _lib.ptr(status), _lib.stream_of(out)) == _lib.E_ARG


def _sources(n, H, W, c, seed):
    rng = np.random.default_rng(seed)
    u8 = rng.integers(0, 256, (n, H, W, c)).astype(np.uint8)
    u8.reshape(-1)[:2] = (0, 255)
    return {"u8": u8, "f32": rng.random((n, H, W, c), dtype=np.float32)}


@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("H,W,h,w", [(8, 8, 4, 4), (16, 24, 2, 3)])
def test_resize_power_of_two_factors_are_exact(H, W, h, w, kind, c):
    src = _sources(3, H, W, c, seed=H + c)[kind]
    T = images_ref.area_mean(src, h, w)
    out = images.area_resize(torch.from_numpy(src).to(DEV), h, w)
    assert out.dtype == torch.float32 and out.shape == (3, h, w, c)
    np.testing.assert_array_equal(out.cpu().numpy(), T.astype(np.float32))


@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("H,W,h,w", [(9, 13, 4, 6), (7, 7, 3, 3)])
def test_resize_fractional_factors_within_one_rounding(H, W, h, w, kind, c):
    src = _sources(3, H, W, c, seed=H + W + c)[kind]
    T = images_ref.area_mean(src, h, w)
    out = images.area_resize(torch.from_numpy(src).to(DEV), h, w).cpu().numpy()
    err = np.abs(out.astype(np.float64) - T).max()
    print(f"area_resize {kind} c={c} ({H},{W})->({h},{w}): max |out - T| = {err:.3e} (bound {2.0 ** -24:.3e})")
    assert err <= 2.0 ** -24


def test_resize_identity_is_the_conversion_and_upscaling_raises():
    s = _sources(2, 5, 7, 4, seed=3)
    for kind, want in (("u8", images_ref.to_float(s["u8"])), ("f32", s["f32"])):
        out = images.area_resize(torch.from_numpy(s[kind]).to(DEV), 5, 7)
        np.testing.assert_array_equal(out.cpu().numpy(), want)
    one = images.area_resize(torch.from_numpy(s["u8"][0]).to(DEV), 5, 7)                        # [H,W,c] in, [h,w,c] out
    np.testing.assert_array_equal(one.cpu().numpy(), images_ref.to_float(s["u8"][0]))
    x = torch.from_numpy(s["u8"]).to(DEV)
    for (h, w) in ((6, 7), (5, 8), (0, 3)):
        with pytest.raises(ValueError, match="not a down-scale"):
            images.area_resize(x, h, w)
    dst = torch.zeros((2, 6, 7, 4), device=DEV)
    assert _lib.lib().swnerf_area_resize(_lib.ptr(x), 1, 2, 5, 7, 4, 6, 7, _lib.ptr(dst), _lib.stream_of(dst)) == _lib.E_ARG
    with pytest.raises(RuntimeError, match="GPU"):
        images.area_resize(torch.from_numpy(s["u8"]), 2, 2)


def test_load_pngs_orders_chunks_and_refuses_mixtures(tmp_path):
    H, W = 9, 7
    rgba = [png_ref.image(H, W, 4, seed=k) for k in range(5)]
    paths = []
    for k, im in enumerate(rgba):
        paths.append(str(tmp_path / f"a{k}.png"))
        png_ref.write_png(paths[-1], im, png_ref.row_types(H, seed=k), idat_chunks=1 + k % 2)
    per = H * (1 + W * 4)
    for chunk in (256 << 20, 2 * per, 1):                                       # one run; runs of two files; one file at a time
        out = images.load_pngs(paths, DEV, chunk_bytes=chunk)
        assert out.dtype == torch.uint8 and out.shape == (5, H, W, 4)
        np.testing.assert_array_equal(out.cpu().numpy(), np.stack(rgba))
    half = images.load_pngs(paths, DEV, out_hw=lambda a, b: (a // 2, b // 2), chunk_bytes=2 * per).cpu().numpy()
    T = images_ref.area_mean(np.stack(rgba), 4, 3)
    assert half.dtype == np.float32 and np.abs(half - T).max() <= 2.0 ** -24
    rgb = png_ref.image(H, W, 3, seed=9)
    p_rgb = str(tmp_path / "rgb.png")
    png_ref.write_png(p_rgb, rgb, 4)
    mixed = [paths[0], p_rgb, paths[1]]
    with pytest.raises(ValueError, match="alpha='add'"):
        images.load_pngs(mixed, DEV)
    out = images.load_pngs(mixed, DEV, alpha="add").cpu().numpy()
    np.testing.assert_array_equal(out[[0, 2]], np.stack(rgba[:2]))
    np.testing.assert_array_equal(out[1], np.concatenate([rgb, np.full((H, W, 1), 255, np.uint8)], -1))
    np.testing.assert_array_equal(images.load_pngs([p_rgb], DEV).cpu().numpy()[0], rgb)
    other = str(tmp_path / "other.png")
    png_ref.write_png(other, png_ref.image(H, W + 1, 4, seed=1), 1)
    with pytest.raises(ValueError, match="one call loads one size"):
        images.load_pngs([paths[0], other], DEV)
    with open(tmp_path / "frame.jpg", "wb") as f:
        f.write(b"\xff\xd8\xff\xe0 no picture")
    try:
        import PIL  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match="PIL"):
            images.load_pngs([str(tmp_path / "frame.jpg")], DEV)
