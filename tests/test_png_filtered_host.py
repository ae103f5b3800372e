"""png.read_png_filtered (the host half of the dataset image stage: parse, check, inflate - no unfiltering) on PNGs written by
tests/png_ref.py with every filter type; what it refuses; read_png and write_png unchanged."""
import struct
import zlib

import numpy as np
import pytest

import png_ref
from swnerf import png

SHAPES = [(1, 1, 3), (1, 1, 4), (3, 5, 4), (17, 31, 3), (9, 2, 4)]


@pytest.mark.parametrize("H,W,c", SHAPES)
def test_filtered_scanlines_unfilter_back_to_the_image(tmp_path, H, W, c):
    img = png_ref.image(H, W, c, seed=H * 100 + W)
    for k, types in enumerate([0, 1, 2, 3, 4, png_ref.row_types(H, seed=W)]):
        path = str(tmp_path / f"t{k}.png")
        png_ref.write_png(path, img, types, idat_chunks=1 + k % 3)
        raw, h, w, ch = png.read_png_filtered(path)
        assert (h, w, ch) == (H, W, c) and len(raw) == H * (1 + W * c)
        rows = np.frombuffer(raw, np.uint8).reshape(H, 1 + W * c)
        np.testing.assert_array_equal(rows, png_ref.filter_rows(img, types))          # nothing was unfiltered
        np.testing.assert_array_equal(png._unfilter(raw, h, w, ch).reshape(H, W, c), img)      # alpha included
        np.testing.assert_array_equal(png.read_png(path), img[..., :3])               # read_png: the same pixels, alpha dropped


def test_read_png_of_write_png_is_unchanged(tmp_path):
    img = png_ref.image(6, 7, 4, seed=3)
    path = str(tmp_path / "w.png")
    png.write_png(path, img)
    raw, h, w, c = png.read_png_filtered(path)
    assert (h, w, c) == (6, 7, 4) and set(np.frombuffer(raw, np.uint8).reshape(6, -1)[:, 0]) == {0}      # write_png: filter type 0
    out = png.read_png(path)
    assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(out, img[..., :3])


def _png(ihdr, payload, extra=b""):
    return (b"\x89PNG\r\n\x1a\n" + png_ref._chunk(b"IHDR", struct.pack(">IIBBBBB", *ihdr)) + extra
            + png_ref._chunk(b"IDAT", zlib.compress(payload)) + png_ref._chunk(b"IEND", b""))


def _refusals():
    good = _png((2, 2, 8, 2, 0, 0, 0), bytes(2 * 7))
    crc = bytearray(good)
    crc[-20] ^= 1                                                    # inside the IDAT body
    return {
        "signature": (b"JFIF" + good[4:], "is not a PNG file"),
        "truncated": (good[:-14], "truncated"),
        "crc": (bytes(crc), "CRC mismatch"),
        "palette": (_png((2, 2, 8, 2, 0, 0, 0), bytes(14), extra=png_ref._chunk(b"PLTE", bytes(3))), "critical chunk"),
        "unknown critical": (_png((2, 2, 8, 2, 0, 0, 0), bytes(14), extra=png_ref._chunk(b"XyZw", b"")), "critical chunk"),
        "no idat": (b"\x89PNG\r\n\x1a\n" + png_ref._chunk(b"IHDR", struct.pack(">IIBBBBB", 2, 2, 8, 2, 0, 0, 0)) + png_ref._chunk(b"IEND", b""), "no IHDR or no IDAT"),
        "16 bit": (_png((2, 2, 16, 2, 0, 0, 0), bytes(2 * 13)), "only 8-bit RGB / RGBA"),
        "grey": (_png((2, 2, 8, 0, 0, 0, 0), bytes(2 * 3)), "only 8-bit RGB / RGBA"),
        "interlaced": (_png((2, 2, 8, 6, 0, 0, 1), bytes(2 * 9)), "only 8-bit RGB / RGBA"),
        "empty": (_png((0, 2, 8, 6, 0, 0, 0), bytes(2)), "only 8-bit RGB / RGBA"),
        "short data": (_png((2, 2, 8, 2, 0, 0, 0), bytes(13)), "image data holds 13 bytes, expected 14"),
    }


@pytest.mark.parametrize("name", sorted(_refusals()))
def test_refuses_what_read_png_refuses_with_its_message(tmp_path, name):
    data, msg = _refusals()[name]
    path = str(tmp_path / "bad.png")
    with open(path, "wb") as f:
        f.write(data)
    errors = []
    for reader in (png.read_png, png.read_png_filtered):
        with pytest.raises(ValueError, match=msg) as e:
            reader(path)
        errors.append(str(e.value))
    assert errors[0] == errors[1]
