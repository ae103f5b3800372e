"""Dataset directories -> what the runners train on: the loaders of dataloader/load_blender.py, load_blender_dnerf.py,
load_llff.py and load_custom_data.py and the `dataset_type` switch of nerf/run.py:431-523 and d_nerf/run_dnerf.py:491-513.
Poses, splits, hwf / K and near / far are host numpy (every pose computation is swnerf.cameras); the frames are decoded and
down-sampled on the device by swnerf.images and STAY there: uint8 at full resolution, float32 after a down-scale.  Nothing is
composited on white here - the batch kernel does that per drawn pixel and runner._gt_rgb for test frames.

Every loader takes `_load_images(paths, device, out_hw=None, alpha=None)` (default images.load_pngs) and `_image_size(path)`
(default images.image_size): the seam the host tests use to run without a GPU."""
import json
import os
import random

import numpy as np

from . import cameras, images as _images

_SPLITS = ("train", "val", "test")


def _hooks(_load_images, _image_size):
    return _load_images or _images.load_pngs, _image_size or _images.image_size


def _half(H, W):
    return H // 2, W // 2


def _read_json(path):
    with open(path) as fp:
        return json.load(fp)


def _blender_metas(basedir):
    """transforms_{train,val,test}.json, or - when none of the three exists - one transforms.json cut 80 / 10 / 10 in file order
    (load_blender.py:62-83).  -> ({split: frames}, camera_angle_x).  The reference reads camera_angle_x from the last split it
    looped over, which on the fallback path is a dict without one (a KeyError there); here it comes from transforms.json."""
    present = [s for s in _SPLITS if os.path.exists(os.path.join(basedir, f"transforms_{s}.json"))]
    if not present:
        meta = _read_json(os.path.join(basedir, "transforms.json"))
        frames = meta["frames"]
        a, b = int(0.8 * len(frames)), int(0.9 * len(frames))
        return {"train": frames[:a], "val": frames[a:b], "test": frames[b:]}, float(meta["camera_angle_x"])
    metas = {s: _read_json(os.path.join(basedir, f"transforms_{s}.json")) for s in _SPLITS}      # a missing one of three: FileNotFoundError
    return {s: metas[s]["frames"] for s in _SPLITS}, float(metas["test"]["camera_angle_x"])


def _gather(basedir, frames, skips, suffix=".png"):
    """-> (paths, poses float32 [N,4,4], i_split, kept frames per split)"""
    paths, poses, counts, kept = [], [], [0], {}
    for s in _SPLITS:
        kept[s] = frames[s][::skips[s]]
        paths += [os.path.join(basedir, f["file_path"] + suffix) for f in kept[s]]
        poses += [np.array(f["transform_matrix"]) for f in kept[s]]
        counts.append(counts[-1] + len(kept[s]))
    poses = np.array(poses).astype(np.float32)
    return paths, poses, [np.arange(counts[i], counts[i + 1]) for i in range(3)], kept


def load_blender_data(basedir, half_res=False, testskip=1, device=None, _load_images=None, _image_size=None):
    """dataloader/load_blender.py:60-152 -> (images, poses [N,4,4] f32, render_poses [360,4,4] f32, [H, W, focal], i_split).
    images: device uint8 [N,H,W,4]; with half_res float32 [N,H//2,W//2,4], the area mean of images.area_resize (the reference:
    cv2.resize INTER_AREA of the float image, one frame at a time).  testskip thins val and test only; 0 means 1."""
    load, size = _hooks(_load_images, _image_size)
    frames, angle = _blender_metas(basedir)
    skips = {s: 1 if (s == "train" or testskip == 0) else testskip for s in _SPLITS}
    paths, poses, i_split, _ = _gather(basedir, frames, skips)
    H, W = size(paths[0])[:2]
    imgs = load(paths, device, out_hw=_half if half_res else None)
    return imgs, poses, cameras.blender_render_poses(360), cameras.blender_hwf(H, W, angle, half_res), i_split


def load_blender_dnerf_data(basedir, half_res=False, testskip=1, device=None, _load_images=None, _image_size=None):
    """dataloader/load_blender_dnerf.py:78-151 -> (images, poses, times [N] f32, render_poses, render_times, [H, W, focal], i_split).
    testskip thins EVERY split, train included.  A frame's time is its 'time' entry, else t / (len - 1) within the thinned split;
    each split must start at time 0.  render_poses: transforms_render.json when present, else the 40-view orbit; render_times
    linspace(0, 1, len).  half_res of a non-square image raises ValueError: the reference hands cv2.resize (H, W) where (W, H)
    belongs and fails on the assignment that follows."""
    load, size = _hooks(_load_images, _image_size)
    if int(testskip) < 1:
        raise ValueError(f"swnerf.data.load_blender_dnerf_data: testskip must be >= 1 (it is the slice step of every split), got {testskip}")
    frames = {s: _read_json(os.path.join(basedir, f"transforms_{s}.json")) for s in _SPLITS}
    angle = float(frames["test"]["camera_angle_x"])
    paths, poses, i_split, kept = _gather(basedir, {s: frames[s]["frames"] for s in _SPLITS}, {s: int(testskip) for s in _SPLITS})
    times = []
    for s in _SPLITS:
        ts = [f["time"] if "time" in f else float(t) / (len(kept[s]) - 1) for t, f in enumerate(kept[s])]
        assert ts[0] == 0, "Time must start at 0"
        times.append(np.array(ts).astype(np.float32))
    times = np.concatenate(times, 0)
    H, W = size(paths[0])[:2]
    if half_res and H != W:
        raise ValueError(f"swnerf.data.load_blender_dnerf_data: half_res of a {H} x {W} image: the reference fails on non-square frames")
    render_json = os.path.join(basedir, "transforms_render.json")
    if os.path.exists(render_json):
        render_poses = np.array([np.array(f["transform_matrix"]) for f in _read_json(render_json)["frames"]]).astype(np.float32)
    else:
        render_poses = cameras.blender_render_poses(40)
    render_times = np.linspace(0., 1., render_poses.shape[0], dtype=np.float32)
    imgs = load(paths, device, out_hw=_half if half_res else None)
    return imgs, poses, times, render_poses, render_times, cameras.blender_hwf(H, W, angle, half_res), i_split


def _llff_files(imgdir):
    return [os.path.join(imgdir, f) for f in sorted(os.listdir(imgdir)) if f.endswith("JPG") or f.endswith("jpg") or f.endswith("png")]


def load_llff_data(basedir, factor=8, recenter=True, bd_factor=.75, spherify=False, path_zflat=False, device=None,
                   _load_images=None, _image_size=None):
    """dataloader/load_llff.py:244-317 -> (images, poses [N,3,5] f32, bds [N,2] f32, render_poses, i_test).
    images: RGB.  images_<factor>/ is read when it exists, as the reference does: device uint8 [N,H,W,3].  When only images/ exists
    the frames are down-sampled ON THE DEVICE to H // factor x W // factor with images.area_resize (float32) and nothing is written
    to disk.  The reference instead shells out to ImageMagick (`mogrify -resize`) and keeps the minified directory; that is a
    different filter, so pixels differ between the two routes.  factor None or 1: images/ as it is.
    spherify=True raises NotImplementedError (swnerf.cameras: its body is missing in the reference)."""
    if spherify:
        raise NotImplementedError("swnerf.data.load_llff_data: spherify is not built (spherify_poses has no body in the reference)")
    load, size = _hooks(_load_images, _image_size)
    poses_arr = np.load(os.path.join(basedir, "poses_bounds.npy"))
    factor = 1 if factor is None else factor
    minified = os.path.join(basedir, f"images_{factor}")
    out_hw = None
    if factor != 1 and os.path.isdir(minified):
        files = _llff_files(minified)
        H, W = size(files[0])[:2]
    else:
        files = _llff_files(os.path.join(basedir, "images"))
        H, W = size(files[0])[:2]
        if factor != 1:
            if int(factor) != factor or factor < 1:
                raise ValueError(f"swnerf.data.load_llff_data: factor {factor}: the on-device down-scale takes integer factors")
            H, W = H // int(factor), W // int(factor)
            out_hw = (H, W)
    if poses_arr.shape[0] != len(files):
        raise ValueError(f"swnerf.data.load_llff_data: {len(files)} images and {poses_arr.shape[0]} poses")
    poses, bds, render_poses, i_test = cameras.llff_from_poses_bounds(poses_arr, (H, W), factor=factor, recenter=recenter,
                                                                     bd_factor=bd_factor, path_zflat=path_zflat)
    imgs = load(files, device, out_hw=out_hw)
    return imgs[..., :3], poses, bds, render_poses, i_test


# load_custom_data.py:57-86: its own pose_spherical ends in diag(1, -1, -1, 1) where load_blender's ends in a signed permutation P;
# P is orthogonal, so diag(1, -1, -1, 1) P^T turns one orbit into the other exactly
_CUSTOM_FROM_BLENDER = (np.diag([1., -1., -1., 1.]) @ np.array([[-1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1.]]).T).astype(np.float32)


def load_custom_data(basedir, half_res=False, testskip=1, device=None, _load_images=None, _image_size=None):
    """dataloader/load_custom_data.py:88-160 -> (images, poses, render_poses [360,4,4], K, [H, W, (fl_x + fl_y) / 2], i_split).
    One transforms.json (file_path with its extension; fl_x, fl_y, cx, cy), its frames shuffled with random.shuffle - the same
    call on the same global generator, so random.seed(s) before it reproduces the reference's split - and cut 80 / 10 / rest;
    testskip thins test only.  RGB frames get an opaque alpha: images are device uint8 [N,H,W,4], float32 with half_res (which
    halves fl, cx, cy as well)."""
    load, size = _hooks(_load_images, _image_size)
    meta = _read_json(os.path.join(basedir, "transforms.json"))
    frames = meta["frames"]
    random.shuffle(frames)
    a, b = int(0.8 * len(frames)), int(0.1 * len(frames))
    split = {"train": frames[:a], "val": frames[a:a + b], "test": frames[a + b:]}
    paths, poses, i_split, _ = _gather(basedir, split, {"train": 1, "val": 1, "test": testskip}, suffix="")
    H, W = size(paths[0])[:2]
    fx, fy, cx, cy = meta["fl_x"], meta["fl_y"], meta["cx"], meta["cy"]
    if half_res:
        H, W, fx, fy, cx, cy = H // 2, W // 2, fx / 2., fy / 2., cx / 2., cy / 2.
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    render_poses = (_CUSTOM_FROM_BLENDER @ cameras.blender_render_poses(360)).astype(np.float32)
    imgs = load(paths, device, out_hw=_half if half_res else None, alpha="add")
    return imgs, poses, render_poses, K, [H, W, (fx + fy) * 0.5], i_split


def load_dataset(args, timed=False, device=None, _load_images=None, _image_size=None):
    """The `dataset_type` switch of nerf/run.py:431-523 (timed=False) and d_nerf/run_dnerf.py:491-513 (timed=True: the D-NeRF
    blender layout with frame times) -> a dict with the keys runner._train_data takes: images, poses, render_poses, hwf, i_split,
    near, far, K (and times, render_times when timed; bds for llff), so `runner.train(args, data.load_dataset(args))` and
    `runner.train_dnerf(args, data.load_dataset(args, timed=True))` work as they stand.
    args: datadir, dataset_type, and where they apply half_res, testskip, factor, llffhold, no_ndc, spherify.
    near / far: blender 2 / 6, custom 1 / 6, llff 0 / 1 or, under no_ndc, min(bds) * .9 / max(bds).  hwf is [int, int, focal] and K
    the pinhole matrix of it unless the loader gave one.  deepvoxels and LINEMOD raise NotImplementedError."""
    kind = args.dataset_type
    opt = lambda name, default: getattr(args, name, default)
    hooks = dict(device=device, _load_images=_load_images, _image_size=_image_size)
    out = {"K": None}
    if kind in ("deepvoxels", "LINEMOD"):
        raise NotImplementedError(f"swnerf.data.load_dataset: dataset_type {kind} is not built (blender, llff and custom are)")
    if timed:
        if kind != "blender":
            raise ValueError(f"swnerf.data.load_dataset: unknown dataset type {kind!r} with frame times (run_dnerf.py reads blender only)")
        imgs, poses, times, render_poses, render_times, hwf, i_split = load_blender_dnerf_data(
            args.datadir, opt("half_res", False), opt("testskip", 1), **hooks)
        i_train = i_split[0]
        min_time, max_time = times[i_train[0]], times[i_train[-1]]
        assert min_time == 0., "time must start at 0"
        assert max_time == 1., "max time must be 1"
        out.update(times=times, render_times=render_times, near=2., far=6.)
    elif kind == "blender":
        imgs, poses, render_poses, hwf, i_split = load_blender_data(args.datadir, opt("half_res", False), opt("testskip", 1), **hooks)
        out.update(near=2., far=6.)
    elif kind == "custom":
        imgs, poses, render_poses, K, hwf, i_split = load_custom_data(args.datadir, opt("half_res", False), opt("testskip", 1), **hooks)
        out.update(near=1., far=6., K=K)
    elif kind == "llff":
        imgs, poses, bds, render_poses, i_test = load_llff_data(args.datadir, opt("factor", 8), recenter=True, bd_factor=.75,
                                                                spherify=opt("spherify", False), **hooks)
        hwf = poses[0, :3, -1]
        poses = poses[:, :3, :4]
        i_test = [i_test]
        if opt("llffhold", 8) > 0:
            i_test = np.arange(imgs.shape[0])[::opt("llffhold", 8)]
        i_val = i_test
        i_train = np.array([i for i in np.arange(int(imgs.shape[0])) if (i not in i_test and i not in i_val)])
        i_split = [i_train, np.asarray(i_val), np.asarray(i_test)]
        near, far = cameras.llff_near_far(bds, opt("no_ndc", False))
        out.update(near=near, far=far, bds=bds)
    else:
        raise ValueError(f"swnerf.data.load_dataset: unknown dataset type {kind!r}")
    H, W, focal = hwf
    H, W = int(H), int(W)
    if out["K"] is None:
        out["K"] = cameras.intrinsics(H, W, focal)
    out.update(images=imgs, poses=poses, render_poses=render_poses, hwf=[H, W, focal], i_split=i_split)
    return out
