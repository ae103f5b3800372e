"""swnerf.data without pixels: splits, testskip per loader, hwf / K under half_res, near / far, llffhold, the single
transforms.json fallback and the seeded custom shuffle, with the image stage injected (no GPU).  Blender and LLFF numbers against
g9_cameras.npz, the D-NeRF and custom loaders against g18_data.npz - both captured from the reference's own loaders."""
import json
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest

import cases
import cases_data
import png_ref
from swnerf import cameras, data, png, synth


class FakeImages:
    """the image stage: records the call, returns host zeros of the shape load_pngs would return"""

    def __init__(self, hw, channels=4):
        self.hw, self.channels, self.calls = hw, channels, []

    def size(self, path):
        assert os.path.exists(path), path
        return self.hw + (self.channels,)

    def load(self, paths, device, out_hw=None, alpha=None):
        self.calls.append(SimpleNamespace(paths=list(paths), out_hw=out_hw, alpha=alpha))
        for p in paths:
            assert os.path.exists(p), p
        hw = out_hw(*self.hw) if callable(out_hw) else (out_hw or self.hw)
        c = 4 if alpha == "add" else self.channels
        return np.zeros((len(paths),) + tuple(hw) + (c,), np.uint8 if out_hw is None else np.float32)

    def hooks(self):
        return dict(_load_images=self.load, _image_size=self.size)


def _touch(path):
    open(path, "wb").close()


def _blender_dir(base, frames, single=False):
    for s, fr in frames.items():
        os.makedirs(os.path.join(base, s), exist_ok=True)
        for f in fr:
            _touch(os.path.join(base, f["file_path"] + ".png"))
    if single:
        json.dump({"camera_angle_x": synth.LEGO_CAMERA_ANGLE_X, "frames": [f for s in ("train", "val", "test") for f in frames[s]]},
                  open(os.path.join(base, "transforms.json"), "w"))
    else:
        for s, fr in frames.items():
            json.dump({"camera_angle_x": synth.LEGO_CAMERA_ANGLE_X, "frames": fr}, open(os.path.join(base, f"transforms_{s}.json"), "w"))


def test_blender_loader_matches_reference(golden, tmp_path):
    ref = golden("g9_cameras")
    frames = cases.g9_blender_frames()
    _blender_dir(str(tmp_path), frames)
    for half, tag in ((False, "full"), (True, "half")):
        fake = FakeImages((16, 16))
        imgs, poses, render_poses, hwf, i_split = data.load_blender_data(str(tmp_path), half_res=half, testskip=2, **fake.hooks())
        np.testing.assert_array_equal(poses, ref[f"bl_poses_{tag}"])
        assert poses.dtype == np.float32 and render_poses.dtype == np.float32
        np.testing.assert_allclose(render_poses, ref[f"bl_render_{tag}"], atol=1e-6)
        np.testing.assert_allclose(np.array(hwf, np.float64), ref[f"bl_hwf_{tag}"], rtol=1e-12)
        assert [len(s) for s in i_split] == list(ref[f"bl_split_{tag}"])
        assert np.concatenate(i_split).tolist() == list(range(len(poses)))
        assert imgs.shape == (len(poses),) + ((8, 8) if half else (16, 16)) + (4,)
        call, = fake.calls
        want = [f["file_path"] for f in frames["train"]] + [f["file_path"] for s in ("val", "test") for f in frames[s][::2]]
        assert call.paths == [os.path.join(str(tmp_path), p + ".png") for p in want] and call.alpha is None
        assert (call.out_hw(9, 7) == (4, 3)) if half else (call.out_hw is None)


def test_blender_testskip_zero_and_one_keep_every_frame(tmp_path):
    frames = cases.g9_blender_frames()
    _blender_dir(str(tmp_path), frames)
    for skip in (0, 1):
        i_split = data.load_blender_data(str(tmp_path), testskip=skip, **FakeImages((16, 16)).hooks())[4]
        assert [len(s) for s in i_split] == [len(frames[s]) for s in ("train", "val", "test")]


def test_blender_single_transforms_json_is_split_80_10_10(tmp_path):
    frames = cases.g9_blender_frames()
    _blender_dir(str(tmp_path), frames, single=True)
    every = [f for s in ("train", "val", "test") for f in frames[s]]
    n = len(every)
    imgs, poses, render_poses, hwf, i_split = data.load_blender_data(str(tmp_path), testskip=1, **FakeImages((16, 16)).hooks())
    assert [len(s) for s in i_split] == [int(.8 * n), int(.9 * n) - int(.8 * n), n - int(.9 * n)]
    np.testing.assert_array_equal(poses, np.array([f["transform_matrix"] for f in every]).astype(np.float32))      # file order
    assert hwf == cameras.blender_hwf(16, 16, synth.LEGO_CAMERA_ANGLE_X)
    os.remove(tmp_path / "transforms.json")
    _blender_dir(str(tmp_path), {"train": frames["train"]})                  # one of the three alone is an error, not a fallback
    with pytest.raises(FileNotFoundError):
        data.load_blender_data(str(tmp_path), **FakeImages((16, 16)).hooks())


@pytest.mark.parametrize("scene,with_time", [("timed", True), ("untimed", False)])
def test_dnerf_loader_matches_reference(golden, tmp_path, scene, with_time):
    ref = golden("g18_data")
    cases_data.write_dnerf_scene(str(tmp_path), with_time, _touch)
    for half in (False, True):
        tag = f"dn_{scene}_{'half' if half else 'full'}"
        fake = FakeImages(cases_data.IMG_HW)
        imgs, poses, times, render_poses, render_times, hwf, i_split = data.load_blender_dnerf_data(
            str(tmp_path), half_res=half, testskip=cases_data.DNERF_SKIP, **fake.hooks())
        np.testing.assert_array_equal(poses, ref[f"{tag}_poses"])
        np.testing.assert_array_equal(times, ref[f"{tag}_times"])
        assert times.dtype == np.float32 and render_times.dtype == np.float32
        np.testing.assert_allclose(render_poses, ref[f"{tag}_render"], atol=1e-6)
        np.testing.assert_allclose(render_times, ref[f"{tag}_render_times"], atol=1e-7)
        assert render_poses.shape[0] == (6 if with_time else 40)
        np.testing.assert_allclose(np.array(hwf, np.float64), ref[f"{tag}_hwf"], rtol=1e-12)
        assert [len(s) for s in i_split] == list(ref[f"{tag}_split"]) == [5, 3, 4]               # skip = 2 on EVERY split
        assert list(imgs.shape) == list(ref[f"{tag}_imshape"])


def test_dnerf_loader_refusals(tmp_path):
    cases_data.write_dnerf_scene(str(tmp_path), True, _touch)
    with pytest.raises(ValueError, match="non-square"):
        data.load_blender_dnerf_data(str(tmp_path), half_res=True, **FakeImages((16, 12)).hooks())
    assert data.load_blender_dnerf_data(str(tmp_path), half_res=False, **FakeImages((16, 12)).hooks())[5][:2] == [16, 12]
    with pytest.raises(ValueError, match="testskip"):
        data.load_blender_dnerf_data(str(tmp_path), testskip=0, **FakeImages((16, 16)).hooks())
    meta = json.load(open(tmp_path / "transforms_val.json"))
    meta["frames"][0]["time"] = 0.25
    json.dump(meta, open(tmp_path / "transforms_val.json", "w"))
    with pytest.raises(AssertionError, match="Time must start at 0"):
        data.load_blender_dnerf_data(str(tmp_path), **FakeImages((16, 16)).hooks())


def test_custom_loader_matches_reference_under_the_same_seed(golden, tmp_path):
    ref = golden("g18_data")
    cases_data.write_custom_scene(str(tmp_path), _touch)
    for half in (False, True):
        tag = f"cu_{'half' if half else 'full'}"
        fake = FakeImages(cases_data.IMG_HW, channels=3)
        random.seed(cases_data.CUSTOM_SEED)
        imgs, poses, render_poses, K, hwf, i_split = data.load_custom_data(str(tmp_path), half_res=half, testskip=cases_data.CUSTOM_SKIP,
                                                                           **fake.hooks())
        np.testing.assert_array_equal(poses, ref[f"{tag}_poses"])                                # the shuffle, frame for frame
        np.testing.assert_allclose(render_poses, ref[f"{tag}_render"], atol=1e-6)
        np.testing.assert_allclose(K, ref[f"{tag}_K"], rtol=1e-15)
        np.testing.assert_allclose(np.array(hwf, np.float64), ref[f"{tag}_hwf"], rtol=1e-15)
        assert [len(s) for s in i_split] == list(ref[f"{tag}_split"])
        assert list(imgs.shape) == list(ref[f"{tag}_imshape"]) and fake.calls[0].alpha == "add"  # RGB files: alpha appended
    random.seed(cases_data.CUSTOM_SEED + 1)
    other = data.load_custom_data(str(tmp_path), testskip=cases_data.CUSTOM_SKIP, **FakeImages(cases_data.IMG_HW, 3).hooks())[1]
    assert not np.array_equal(other, ref["cu_full_poses"])


def _llff_dir(base, dirs, n, hw):
    pb = cases.g9_poses_bounds(n)
    os.makedirs(base, exist_ok=True)
    np.save(os.path.join(base, "poses_bounds.npy"), pb)
    for d in dirs:
        os.makedirs(os.path.join(base, d))
        for i in range(n):
            _touch(os.path.join(base, d, f"img{i:03d}.png"))
        _touch(os.path.join(base, d, "notes.txt"))
    return pb


def test_llff_loader_matches_reference(golden, tmp_path):
    ref = golden("g9_cameras")
    base = str(tmp_path / "scene")
    pb = _llff_dir(base, ("images", "images_8"), 11, (24, 32))
    assert ref["crc"] == cases.checksum(pb)
    fake = FakeImages((24, 32), channels=4)
    imgs, poses, bds, render_poses, i_test = data.load_llff_data(base, factor=8, **fake.hooks())
    np.testing.assert_allclose(poses, ref["llff_poses_spiral"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(bds, ref["llff_bds_spiral"], rtol=1e-6)
    np.testing.assert_allclose(render_poses, ref["llff_render_spiral"], rtol=1e-5, atol=1e-6)
    assert i_test == int(ref["llff_itest_spiral"][0])
    assert imgs.shape == (11, 24, 32, 3)                                                         # alpha cut, as imread(f)[..., :3]
    call, = fake.calls
    assert call.out_hw is None and [os.path.basename(os.path.dirname(p)) for p in call.paths] == ["images_8"] * 11
    assert call.paths == sorted(call.paths) and not any(p.endswith(".txt") for p in call.paths)


def test_llff_without_minified_directory_downsamples_and_writes_nothing(tmp_path):
    base = str(tmp_path / "scene")
    _llff_dir(base, ("images",), 5, (50, 67))
    before = sorted(os.listdir(base))
    fake = FakeImages((50, 67), channels=3)
    imgs, poses, bds, render_poses, i_test = data.load_llff_data(base, factor=4, **fake.hooks())
    assert fake.calls[0].out_hw == (12, 16) and imgs.shape == (5, 12, 16, 3) and imgs.dtype == np.float32
    assert poses[0, 0, 4] == 12 and poses[0, 1, 4] == 16 and abs(poses[0, 2, 4] - 3260.5 / 4) < 1e-3
    assert sorted(os.listdir(base)) == before
    assert "mogrify" in data.load_llff_data.__doc__
    full = data.load_llff_data(base, factor=None, **FakeImages((50, 67), 3).hooks())
    assert full[0].shape == (5, 50, 67, 3) and full[1][0, 2, 4] == np.float32(3260.5)
    with pytest.raises(NotImplementedError, match="spherify"):
        data.load_llff_data(base, factor=4, spherify=True, **fake.hooks())
    with pytest.raises(ValueError, match="5 images and 4 poses"):
        np.save(os.path.join(base, "poses_bounds.npy"), cases.g9_poses_bounds(4))
        data.load_llff_data(base, factor=4, **fake.hooks())


def _args(**kw):
    return SimpleNamespace(**kw)


def test_load_dataset_blender_and_custom(tmp_path):
    frames = cases.g9_blender_frames()
    bl = str(tmp_path / "bl")
    _blender_dir(bl, frames)
    d = data.load_dataset(_args(dataset_type="blender", datadir=bl, half_res=True, testskip=2), **FakeImages((16, 16)).hooks())
    assert (d["near"], d["far"]) == (2., 6.) and d["hwf"][:2] == [8, 8] and isinstance(d["hwf"][0], int)
    np.testing.assert_array_equal(d["K"], cameras.intrinsics(8, 8, d["hwf"][2]))
    assert len(d["i_split"]) == 3 and d["images"].shape[-1] == 4 and "times" not in d           # RGBA kept: nothing composited
    from swnerf import runner
    t = runner._train_data(d, False)                                                             # the runners take it as it is
    assert t["hwf"] == d["hwf"] and t["K"] is d["K"]
    cu = str(tmp_path / "cu")
    cases_data.write_custom_scene(cu, _touch)
    d = data.load_dataset(_args(dataset_type="custom", datadir=cu, half_res=False, testskip=1), **FakeImages((16, 16), 3).hooks())
    assert (d["near"], d["far"]) == (1., 6.)
    np.testing.assert_array_equal(d["K"], np.array([[21.5, 0, 7.75], [0, 22.25, 8.5], [0, 0, 1]]))
    assert d["hwf"] == [16, 16, (21.5 + 22.25) * .5] and sum(len(s) for s in d["i_split"]) == 13
    for kind in ("deepvoxels", "LINEMOD"):
        with pytest.raises(NotImplementedError, match=kind):
            data.load_dataset(_args(dataset_type=kind, datadir=bl))
    with pytest.raises(ValueError, match="unknown dataset type"):
        data.load_dataset(_args(dataset_type="nope", datadir=bl))


def test_load_dataset_llff_holdout_and_bounds(tmp_path):
    base = str(tmp_path / "scene")
    _llff_dir(base, ("images_8", "images"), 11, (24, 32))
    hooks = FakeImages((24, 32), 3).hooks()
    d = data.load_dataset(_args(dataset_type="llff", datadir=base, factor=8, llffhold=4, no_ndc=False), **hooks)
    assert (d["near"], d["far"]) == (0., 1.)
    assert list(d["i_split"][2]) == [0, 4, 8] == list(d["i_split"][1]) and list(d["i_split"][0]) == [1, 2, 3, 5, 6, 7, 9, 10]
    assert d["poses"].shape == (11, 3, 4) and d["hwf"] == [24, 32, d["hwf"][2]] and abs(d["hwf"][2] - 3260.5 / 8) < 1e-3
    np.testing.assert_array_equal(d["K"], cameras.intrinsics(24, 32, d["hwf"][2]))
    d0 = data.load_dataset(_args(dataset_type="llff", datadir=base, factor=8, llffhold=0, no_ndc=True), **hooks)
    i_test = cameras.llff_from_poses_bounds(cases.g9_poses_bounds(11), (24, 32), 8)[3]
    assert list(d0["i_split"][2]) == [i_test] and i_test not in d0["i_split"][0] and len(d0["i_split"][0]) == 10
    assert d0["near"] == float(d0["bds"].min() * .9) and d0["far"] == float(d0["bds"].max())


def test_load_dataset_with_times(tmp_path):
    base = str(tmp_path / "dn")
    cases_data.write_dnerf_scene(base, True, _touch)
    hooks = FakeImages(cases_data.IMG_HW).hooks()
    d = data.load_dataset(_args(dataset_type="blender", datadir=base, half_res=False, testskip=2), timed=True, **hooks)
    assert (d["near"], d["far"]) == (2., 6.) and d["times"].shape == (12,) and d["render_times"].shape == (6,)
    from swnerf import runner
    assert runner._train_data(d, True)["times"] is d["times"]
    with pytest.raises(ValueError, match="frame times"):
        data.load_dataset(_args(dataset_type="llff", datadir=base), timed=True, **hooks)
    meta = json.load(open(os.path.join(base, "transforms_train.json")))
    meta["frames"][-1]["time"] = 0.9                                             # the last training frame no longer ends at 1
    json.dump(meta, open(os.path.join(base, "transforms_train.json"), "w"))
    with pytest.raises(AssertionError, match="max time must be 1"):
        data.load_dataset(_args(dataset_type="blender", datadir=base, testskip=2), timed=True, **hooks)


def test_image_size_reads_the_header_alone(tmp_path):
    from swnerf import images
    for c in (3, 4):
        path = str(tmp_path / f"s{c}.png")
        png_ref.write_png(path, png_ref.image(5, 9, c, seed=c), 4)
        assert images.image_size(path) == (5, 9, c)
    png.write_png(str(tmp_path / "g.png"), np.zeros((3, 2), np.uint8))
    assert images.image_size(str(tmp_path / "g.png")) == (3, 2, 1)
    with open(tmp_path / "no.png", "wb") as f:
        f.write(b"not a png at all, but longer than thirty-three bytes")
    with pytest.raises(ValueError, match="is not a PNG file"):
        images.image_size(str(tmp_path / "no.png"))
