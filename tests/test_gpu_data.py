"""swnerf.data end to end on the GPU: tiny dataset directories written with tests/png_ref.py (every filter type), loaded
through load_dataset and compared with the numpy pipeline - png._unfilter, then tests/images_ref.py - under the bounds of
test_gpu_images.py (bytes bit for bit; power-of-two factors exact; other factors within 2^-24); two iterations of runner.train
and runner.train_dnerf on what was loaded."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cases
import images_ref
import png_ref
from swnerf import data, png, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _host_pixels(path):
    raw, h, w, c = png.read_png_filtered(path)
    return png._unfilter(raw, h, w, c).reshape(h, w, c)


def _write(path, H, W, c, seed):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    png_ref.write_png(path, png_ref.image(H, W, c, seed), png_ref.row_types(H, seed + 1), idat_chunks=1 + seed % 2)


def _blender_dir(base, H, W, timed=False):
    """4 + 2 + 2 frames; timed: the D-NeRF layout (train times 0 .. 1)"""
    k = 0
    for s, n in (("train", 4), ("val", 2), ("test", 2)):
        frames = []
        for i in range(n):
            f = {"file_path": f"./{s}/r_{i}", "transform_matrix": synth.pose_spherical(40.0 * k, -30.0, 4.0).astype(float).tolist()}
            if timed:
                f["time"] = i / (n - 1)
            frames.append(f)
            _write(os.path.join(base, s, f"r_{i}.png"), H, W, 4, seed=k)
            k += 1
        with open(os.path.join(base, f"transforms_{s}.json"), "w") as fp:
            json.dump({"camera_angle_x": synth.LEGO_CAMERA_ANGLE_X, "frames": frames}, fp)
    return [os.path.join(base, s, f"r_{i}.png") for s, n in (("train", 4), ("val", 2), ("test", 2)) for i in range(n)]


def _check_images(images, paths, dtype, hw=None, channels=4, exact=True):
    want = np.stack([_host_pixels(p) for p in paths])
    if want.shape[-1] < channels:
        want = np.concatenate([want, np.full(want.shape[:-1] + (1,), 255, np.uint8)], -1)
    want = want[..., :channels]
    assert isinstance(images, torch.Tensor) and images.device == torch.device(DEV) and images.dtype == dtype
    got = images.cpu().numpy()
    if hw is None:
        assert got.shape == want.shape
        np.testing.assert_array_equal(got, want)
        return
    T = images_ref.area_mean(want, *hw)
    assert got.shape == T.shape
    err = np.abs(got.astype(np.float64) - T).max()
    print(f"{want.shape[1:3]} -> {hw}: max |out - T| = {err:.3e}")
    if exact:
        np.testing.assert_array_equal(got, T.astype(np.float32))
    else:
        assert err <= 2.0 ** -24


def _args(tmp, **kw):
    a = dict(expname="data", basedir=str(tmp), netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, lrate=5e-4,
             lrate_decay=500, netchunk=1024 * 64, no_reload=True, ft_path=None, N_samples=8, N_importance=8, perturb=1.,
             use_viewdirs=True, i_embed=0, multires=10, multires_views=4, raw_noise_std=0., dataset_type="blender", white_bkgd=True,
             no_ndc=False, lindisp=False, chunk=1024 * 32, N_rand=64, no_batching=True, precrop_iters=0, precrop_frac=.5,
             i_print=1000, i_weights=1000, i_testset=100000, N_iters=2, N_iter=2, seed=0, half_res=False, testskip=1)
    a.update(kw)
    return SimpleNamespace(**a)


def test_blender_dataset_loads_and_trains(tmp_path):
    from swnerf import runner
    base = str(tmp_path / "lego")
    paths = _blender_dir(base, 8, 8)
    args = _args(tmp_path, datadir=base)
    d = data.load_dataset(args, device=DEV)
    _check_images(d["images"], paths, torch.uint8)
    assert d["hwf"][:2] == [8, 8] and [len(s) for s in d["i_split"]] == [4, 2, 2] and d["poses"].shape == (8, 4, 4)
    half = data.load_dataset(_args(tmp_path, datadir=base, half_res=True, testskip=2), device=DEV)
    _check_images(half["images"], paths[:4] + [paths[4], paths[6]], torch.float32, hw=(4, 4))
    assert half["hwf"][:2] == [4, 4] and half["hwf"][2] == d["hwf"][2] / 2.
    torch.manual_seed(0)
    np.random.seed(0)
    rec = runner.train(args, d, device=DEV)
    assert [r["step"] for r in rec] == [1, 2] and all(np.isfinite(r["loss"]) and r["loss"] > 0 for r in rec)


def test_blender_half_res_of_an_odd_size(tmp_path):
    base = str(tmp_path / "odd")
    paths = _blender_dir(base, 9, 7)
    d = data.load_dataset(_args(tmp_path, datadir=base, half_res=True), device=DEV)
    _check_images(d["images"], paths, torch.float32, hw=(4, 3), exact=False)
    assert d["hwf"][:2] == [4, 3] and d["K"][0, 2] == 1.5 and d["K"][1, 2] == 2.


def test_dnerf_dataset_loads_and_trains(tmp_path):
    from swnerf import runner
    base = str(tmp_path / "balls")
    paths = _blender_dir(base, 8, 8, timed=True)
    args = _args(tmp_path, datadir=base, nerf_type="direct_temporal", not_zero_canonical=False, use_two_models_for_fine=False,
                 do_half_precision=False, add_tv_loss=False, tv_loss_weight=1e-4, precrop_iters_time=0)
    d = data.load_dataset(args, timed=True, device=DEV)
    _check_images(d["images"], paths, torch.uint8)
    np.testing.assert_array_equal(d["times"], np.array([0, 1 / 3, 2 / 3, 1, 0, 1, 0, 1], np.float32))
    assert d["render_poses"].shape == (40, 4, 4) and d["render_times"][0] == 0 and d["render_times"][-1] == 1
    torch.manual_seed(0)
    np.random.seed(0)
    rec = runner.train_dnerf(args, d, device=DEV)
    assert [r["step"] for r in rec] == [1, 2] and all(np.isfinite(r["loss"]) and r["loss"] > 0 for r in rec)


def test_llff_dataset_with_and_without_a_minified_directory(tmp_path):
    pb = cases.g9_poses_bounds(5)
    for name, dirs in (("mini", ("images", "images_4")), ("plain", ("images",))):
        base = str(tmp_path / name)
        os.makedirs(base)
        np.save(os.path.join(base, "poses_bounds.npy"), pb)
        for dname in dirs:
            for i in range(5):
                _write(os.path.join(base, dname, f"img{i:03d}.png"), 12, 16, 3, seed=10 * len(dname) + i)
    mini = data.load_dataset(_args(tmp_path, datadir=str(tmp_path / "mini"), dataset_type="llff", factor=4, llffhold=2), device=DEV)
    _check_images(mini["images"], [str(tmp_path / "mini" / "images_4" / f"img{i:03d}.png") for i in range(5)], torch.uint8, channels=3)
    assert mini["hwf"][:2] == [12, 16] and [list(s) for s in mini["i_split"]] == [[1, 3], [0, 2, 4], [0, 2, 4]]
    assert (mini["near"], mini["far"]) == (0., 1.) and mini["poses"].shape == (5, 3, 4)
    plain = data.load_dataset(_args(tmp_path, datadir=str(tmp_path / "plain"), dataset_type="llff", factor=4, llffhold=2), device=DEV)
    _check_images(plain["images"], [str(tmp_path / "plain" / "images" / f"img{i:03d}.png") for i in range(5)], torch.float32, hw=(3, 4),
                  channels=3)
    assert plain["hwf"][:2] == [3, 4] and plain["hwf"][2] == mini["hwf"][2]
    assert sorted(os.listdir(tmp_path / "plain")) == ["images", "poses_bounds.npy"]              # nothing written


def test_custom_dataset_of_rgb_files(tmp_path):
    import random
    base = str(tmp_path / "custom")
    frames = [{"file_path": f"images/f_{i}.png", "transform_matrix": synth.pose_spherical(36.0 * i, -30.0, 4.0).astype(float).tolist()}
              for i in range(10)]
    for i, f in enumerate(frames):
        _write(os.path.join(base, f["file_path"]), 6, 10, 3, seed=i)
    with open(os.path.join(base, "transforms.json"), "w") as fp:
        json.dump({"fl_x": 12., "fl_y": 13., "cx": 5., "cy": 3., "frames": frames}, fp)
    order = list(frames)
    random.seed(3)
    random.shuffle(order)
    random.seed(3)
    d = data.load_dataset(_args(tmp_path, datadir=base, dataset_type="custom"), device=DEV)
    _check_images(d["images"], [os.path.join(base, f["file_path"]) for f in order], torch.uint8)         # alpha 255 appended
    assert [len(s) for s in d["i_split"]] == [8, 1, 1] and (d["near"], d["far"]) == (1., 6.) and d["hwf"] == [6, 10, 12.5]
    random.seed(3)
    h = data.load_dataset(_args(tmp_path, datadir=base, dataset_type="custom", half_res=True), device=DEV)
    _check_images(h["images"], [os.path.join(base, f["file_path"]) for f in order], torch.float32, hw=(3, 5))
    np.testing.assert_array_equal(h["K"], np.array([[6., 0, 2.5], [0, 6.5, 1.5], [0, 0, 1]]))


def test_train_from_dataset_example(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
    import train_from_dataset as ex
    d, rec = ex.main(str(tmp_path), H=16, n_train=3, steps=2, half_res=True)
    assert d["images"].dtype == torch.float32 and tuple(d["images"].shape) == (7, 8, 8, 4) and d["hwf"][:2] == [8, 8]
    assert len(rec) == 2 and all(np.isfinite(r["loss"]) for r in rec)
    assert os.path.exists(os.path.join(str(tmp_path), "train_from_dataset", "000002.tar"))
