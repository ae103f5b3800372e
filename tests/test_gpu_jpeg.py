"""Baseline JPEG frames decoded on the GPU (csrc/jpeg_kernels.hip behind swnerf.images): every byte must equal libjpeg's default
decode, which g19_jpeg.npz (tests/golden/make_golden_jpeg.py) recorded through PIL.  The fixtures are the smallest images at
which each rule can go wrong (1 x 1; chroma planes of at most 2 columns; the first width of the triangle filter; odd sizes and
partial MCUs at 4:4:4 / 4:2:2 / 4:2:0; one component; restart markers; one geometry with three sets of tables).  Every test runs
with PIL made unimportable unless it says otherwise, so nothing here can pass through the host decoder."""
import os
import sys

import numpy as np
import pytest
import torch

import cases
from swnerf import data, fit2d, images

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_jpeg.npz")
BATCH = ["24x16_420_q30", "24x16_420_q75", "24x16_420_q100"]


@pytest.fixture(scope="module")
def g19():
    return dict(np.load(GOLDEN, allow_pickle=False))


@pytest.fixture
def no_pil(monkeypatch):
    for k in ("PIL", "PIL.Image"):
        monkeypatch.setitem(sys.modules, k, None)                       # `from PIL import Image` raises ImportError
    with pytest.raises(RuntimeError, match="PIL"):
        images._pil()


def _baseline(g19):
    return [str(n) for n in g19["names"] if not str(n).endswith("_prog")]


def _file(tmp_path, g19, name, ext=".jpg"):
    p = str(tmp_path / (name + ext))
    with open(p, "wb") as f:
        f.write(g19[name + "_jpg"].tobytes())
    return p


def test_every_baseline_fixture_equals_libjpeg(g19, tmp_path, no_pil):
    names = _baseline(g19)
    assert len(names) == 20
    for n in names:
        want = g19[n + "_rgb"]
        out = images.load_pngs([_file(tmp_path, g19, n)], DEV)
        assert out.dtype == torch.uint8 and out.shape == (1,) + want.shape and out.device == torch.device(DEV)
        np.testing.assert_array_equal(out[0].cpu().numpy(), want, err_msg=f"load_pngs {n}")
        bare = images.decode_jpegs([g19[n + "_jpg"].tobytes()], DEV)
        np.testing.assert_array_equal(bare[0].cpu().numpy(), want, err_msg=f"decode_jpegs {n}")


def test_one_call_decodes_a_batch_with_different_tables(g19, tmp_path, no_pil):
    want = np.stack([g19[n + "_rgb"] for n in BATCH])
    out = images.decode_jpegs([g19[n + "_jpg"].tobytes() for n in BATCH], DEV)
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    rgba = images.decode_jpegs([g19[n + "_jpg"] for n in BATCH], DEV, channels=4).cpu().numpy()          # uint8 arrays are taken as bytes
    np.testing.assert_array_equal(rgba[..., :3], want)
    assert (rgba[..., 3] == 255).all()
    paths = [_file(tmp_path, g19, n) for n in BATCH]
    for chunk in (256 << 20, 1):                                                                   # one run; one file per run, two staging buffers
        np.testing.assert_array_equal(images.load_pngs(paths, DEV, chunk_bytes=chunk).cpu().numpy(), want)
    # runs of different sampling in one call, and sizes that differ
    mixed = ["16x16_444", "16x16_420", "16x16_420", "16x16_422"]
    out = images.decode_jpegs([g19[n + "_jpg"].tobytes() for n in mixed], DEV)
    np.testing.assert_array_equal(out.cpu().numpy(), np.stack([g19[n + "_rgb"] for n in mixed]))
    np.testing.assert_array_equal(images.load_pngs([_file(tmp_path, g19, n) for n in mixed], DEV).cpu().numpy(), out.cpu().numpy())
    with pytest.raises(ValueError, match="one size"):
        images.decode_jpegs([g19["16x16_444_jpg"].tobytes(), g19["17x23_444_jpg"].tobytes()], DEV)
    with pytest.raises(ValueError, match="one call loads one size"):
        images.load_pngs([_file(tmp_path, g19, "16x16_444"), _file(tmp_path, g19, "17x23_444")], DEV)
    with pytest.raises(ValueError, match="not decodable here"):
        images.decode_jpegs([g19["17x23_420_prog_jpg"].tobytes()], DEV)


def test_alpha_add_out_hw_and_a_png_beside_a_jpeg(g19, tmp_path, no_pil):
    import png_ref
    want = np.stack([g19[n + "_rgb"] for n in BATCH])
    paths = [_file(tmp_path, g19, n) for n in BATCH]
    out = images.load_pngs(paths, DEV, alpha="add").cpu().numpy()
    assert out.shape == (3, 24, 16, 4) and (out[..., 3] == 255).all()
    np.testing.assert_array_equal(out[..., :3], want)
    for hw in ((12, 8), (7, 5)):                                                                   # an integer factor, a fractional one
        ref = images.area_resize(torch.from_numpy(want).to(DEV), *hw)
        got = images.load_pngs(paths, DEV, out_hw=hw)
        assert got.dtype == torch.float32 and torch.equal(got, ref)
    ref = images.area_resize(torch.from_numpy(out).to(DEV), 12, 8)
    assert torch.equal(images.load_pngs(paths, DEV, out_hw=lambda H, W: (H // 2, W // 2), alpha="add"), ref)
    rgb = png_ref.image(24, 16, 3, seed=5)
    rgba = png_ref.image(24, 16, 4, seed=6)
    p_rgb, p_rgba = str(tmp_path / "rgb.png"), str(tmp_path / "rgba.png")
    png_ref.write_png(p_rgb, rgb, 4)
    png_ref.write_png(p_rgba, rgba, 3)
    both = images.load_pngs([paths[0], p_rgb, paths[2]], DEV).cpu().numpy()
    np.testing.assert_array_equal(both, np.stack([want[0], rgb, want[2]]))
    with pytest.raises(ValueError, match="alpha='add'"):
        images.load_pngs([paths[0], p_rgba], DEV)
    both = images.load_pngs([p_rgba, paths[1], p_rgb], DEV, alpha="add").cpu().numpy()
    opaque = np.full((24, 16, 1), 255, np.uint8)
    np.testing.assert_array_equal(both, np.stack([rgba, np.concatenate([want[1], opaque], -1), np.concatenate([rgb, opaque], -1)]))


def test_llff_directory_of_camera_jpegs(g19, tmp_path, no_pil):
    base = tmp_path / "scene"
    os.makedirs(base / "images")
    for k, n in enumerate(BATCH):
        with open(base / "images" / f"IMG_{k:04d}.JPG", "wb") as f:
            f.write(g19[n + "_jpg"].tobytes())
    np.save(base / "poses_bounds.npy", cases.g9_poses_bounds(3))
    imgs, poses, bds, render_poses, i_test = data.load_llff_data(str(base), factor=2, device=DEV)
    want = images.area_resize(torch.from_numpy(np.stack([g19[n + "_rgb"] for n in BATCH])).to(DEV), 12, 8)
    assert imgs.dtype == torch.float32 and imgs.shape == (3, 12, 8, 3) and torch.equal(imgs, want)
    assert poses.shape == (3, 3, 5) and bds.shape == (3, 2)
    full = data.load_llff_data(str(base), factor=1, device=DEV)[0]
    np.testing.assert_array_equal(full.cpu().numpy(), np.stack([g19[n + "_rgb"] for n in BATCH]))
    assert sorted(os.listdir(base)) == ["images", "poses_bounds.npy"]


def test_fit2d_load_picture_without_pil(g19, tmp_path, no_pil):
    from types import SimpleNamespace
    p = _file(tmp_path, g19, "17x23_422")
    positions, colors, width, height = fit2d.load_picture(SimpleNamespace(picture_dir=p))
    want = fit2d.picture_tensors(g19["17x23_422_rgb"])
    assert (width, height) == (23, 17) == want[2:]
    assert torch.equal(positions, want[0]) and torch.equal(colors, want[1])


def test_progressive_file_takes_the_pil_route(g19, tmp_path, monkeypatch):
    p = _file(tmp_path, g19, "17x23_420_prog", ".jpeg")
    with monkeypatch.context() as m:
        for k in ("PIL", "PIL.Image"):
            m.setitem(sys.modules, k, None)
        with pytest.raises(RuntimeError, match="PIL"):
            images.load_pngs([p], DEV)
    pytest.importorskip("PIL.Image")
    np.testing.assert_array_equal(images.load_pngs([p], DEV)[0].cpu().numpy(), g19["17x23_420_prog_rgb"])
    # beside a natively decoded file of the same size
    q = _file(tmp_path, g19, "17x23_420")
    out = images.load_pngs([q, p, q], DEV).cpu().numpy()
    np.testing.assert_array_equal(out, np.stack([g19["17x23_420_rgb"], g19["17x23_420_prog_rgb"], g19["17x23_420_rgb"]]))


def test_cut_entropy_segment_names_the_file(g19, tmp_path, no_pil):
    data_ = g19["40x56_420_rst2_jpg"].tobytes()
    p = str(tmp_path / "broken_frame.jpg")
    with open(p, "wb") as f:
        f.write(data_[:len(data_) // 2 + 300])
    good = _file(tmp_path, g19, "40x56_420_rst2")
    with pytest.raises(ValueError, match="broken_frame.jpg"):
        images.load_pngs([good, p, good], DEV)
    with pytest.raises(ValueError, match="broken_frame.jpg"):
        images.load_pngs([p], DEV)
    with pytest.raises(ValueError, match="file 1"):
        images.decode_jpegs([data_, data_[:len(data_) // 2 + 300]], DEV)
