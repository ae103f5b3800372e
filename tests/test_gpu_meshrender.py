"""swnerf.mesh rendering on the GPU against the numpy replay of tests/meshrender_ref.py, which tests every pixel against every face
and knows no pixel boxes and no tiers: face ids, coverage and all four counts exactly, the bytes of depth, disparity, barycentrics and
of every shading mode exactly (every step is one IEEE fp64 operation on both sides).  Then the windows, the culling, the NULL outputs,
a face list and a pixel count beyond one grid-stride launch (1024 x 256 threads), compare_views against numpy with the fp64 sums in
their written order, the depth convention against a NeRF's own depth_map, and the two runner entry points."""
import os

import numpy as np
import pytest
import torch

import meshops_ref as R
import meshrender_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, FOCAL = 40, 48, 60.0
INTR = M.intrinsics(H, W, focal=FOCAL)
CASES = M.cases()
BG = (0.25, 0.5, 1.0)
_CACHE = {}


def ref(key, make):
    """reference results, computed once and never modified"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


def gpu_render(v, f, poses, h=H, w=W, K=None, focal=FOCAL, colors=None, normals=None, **kw):
    from swnerf import mesh
    out = mesh.render_views_arrays(dev(v), dev(f, torch.int32), h, w, K, poses, normals=None if normals is None else dev(normals),
                                   colors=None if colors is None else dev(colors), focal=focal, **kw)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in out.items()}


def same(got, want, keys=("depth", "disp", "acc", "bary", "rgb"), counts=True):
    if counts:
        print("counts (bad faces, pairs behind, pairs wide, hits):", got["counts"].tolist())
        assert got["counts"].tolist() == want["counts"].tolist()
    assert np.array_equal(got["face"].reshape(want["face"].shape), want["face"])
    for k in keys:
        assert got[k].reshape(want[k].shape).tobytes() == want[k].tobytes(), k


def replay(name, **kw):
    v, f, poses = CASES[name]
    return ref((name, tuple(sorted(kw.items()))), lambda: M.render(v, f, H, W, INTR, poses, colors=M.vertex_colors(v), **kw))


@pytest.mark.parametrize("name", sorted(CASES))
def test_bit_for_bit_against_the_replay(name):
    v, f, poses = CASES[name]
    got = gpu_render(v, f, poses, colors=M.vertex_colors(v), background=BG)
    want = replay(name, background=BG)
    same(got, want)
    assert got["face"].shape == (len(poses), H, W) and got["rgb"].shape == (len(poses), H, W, 3)
    if name == "whole_image":
        assert got["acc"][0].all() and got["counts"][2] == 3
    if name == "behind":
        assert got["counts"][1] >= 1 and not got["acc"][0].any()
    if name in ("repeated_index", "index_equal_V", "nan_vertex"):
        assert got["counts"][0] == {"repeated_index": 1}.get(name, 2)


@pytest.mark.parametrize("shading", ["normals", "headlight"])
@pytest.mark.parametrize("name", ["sphere", "cut_sphere", "straddles"])
def test_shading_by_normals(name, shading):
    v, f, poses = CASES[name]
    nor = R.vertex_normals(v, f).astype(np.float32)
    col = M.vertex_colors(v) if name != "cut_sphere" else None            # headlight without colours: 0.8 grey
    want = M.render(v, f, H, W, INTR, poses, shading=M.SHADINGS[shading], colors=col, normals=nor, want_counts=False)
    got = gpu_render(v, f, poses, colors=col, normals=nor, shading=shading)
    same(got, want, counts=False)
    hit = got["acc"] > 0
    assert hit.any() and (got["rgb"][hit] >= 0).all() and (got["rgb"][hit] <= 1).all()
    if shading == "headlight" and name == "sphere":
        assert got["rgb"][hit].max() > 0.5 and (got["rgb"][~hit] == 0).all()


def test_normals_are_computed_when_the_mesh_brings_none():
    from swnerf import mesh
    v, f, poses = CASES["sphere"]
    got = gpu_render(v, f, poses, shading="normals")
    nor = mesh.vertex_normals(dev(v), dev(f, torch.int32)).cpu().numpy()
    same(got, M.render(v, f, H, W, INTR, poses, shading=1, normals=nor, want_counts=False), counts=False)


@pytest.mark.parametrize("kw", [dict(cull="back"), dict(cull="front"), dict(near=2.0, far=2.3), dict(near=0.0, far=2.1), dict(near=2.2)],
                         ids=["cull_back", "cull_front", "slab", "far_cut", "near_cut"])
def test_culling_and_depth_windows(kw):
    v, f, poses = CASES["sphere"]
    rkw = dict(kw)
    if "cull" in rkw:
        rkw["cull"] = M.CULLS[rkw["cull"]]
    want, full = replay("sphere", **rkw), replay("sphere")
    got = gpu_render(v, f, poses, colors=M.vertex_colors(v), **kw)
    same(got, want)
    assert 0 < got["counts"][3] < full["counts"][3]
    hit = got["acc"] > 0
    if "near" in kw:
        assert (got["depth"][hit] > kw["near"]).all() and (got["depth"][hit] <= kw.get("far", np.inf)).all()
    if kw == dict(cull="front"):
        assert (got["depth"][hit] > full["depth"].reshape(got["depth"].shape)[hit]).all()       # the far side of the closed surface


def test_background_and_output_subsets():
    v, f, poses = CASES["torus"]
    col = M.vertex_colors(v)
    full = gpu_render(v, f, poses, colors=col)
    white = gpu_render(v, f, poses, colors=col, white_bkgd=True)
    miss = full["acc"] == 0
    assert miss.any() and (white["rgb"][miss] == 1).all() and (full["rgb"][miss] == 0).all()
    assert np.array_equal(white["rgb"][~miss], full["rgb"][~miss])
    for outputs in (("depth",), ("acc", "rgb"), ("bary", "disp"), ("face",), ()):
        got = gpu_render(v, f, poses, colors=col, outputs=outputs)
        assert set(got) == set(outputs) | {"counts"}
        for k in outputs:
            assert got[k].tobytes() == full[k].tobytes(), (outputs, k)
        assert got["counts"].tolist() == full["counts"].tolist()
    got = gpu_render(v, f, poses, outputs=("depth", "face"))               # no colours needed when no colour is asked for
    assert got["depth"].tobytes() == full["depth"].tobytes()


def test_two_calls_give_equal_bytes():
    v, f, poses = CASES["two_spheres"]
    col = M.vertex_colors(v)
    a, b = gpu_render(v, f, poses, colors=col), gpu_render(v, f, poses, colors=col)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_pinhole_matrix_odd_image_and_a_camera_inside():
    v, f, _ = CASES["torus"]
    h, w = 37, 53
    K = np.array([[70.5, 0, 20.25], [0, 64.0, 21.5], [0, 0, 1]])
    poses = np.stack([M.pose(0.9, 0.2, 0.05, M.box_centre(v)), M.pose(-1.1, 1.3, 1.4, M.box_centre(v))])
    col = M.vertex_colors(v)
    pose44 = np.concatenate([poses, np.broadcast_to(np.array([0, 0, 0, 1], np.float32), (2, 1, 4))], 1)
    same(gpu_render(v, f, pose44, h, w, K=K, focal=None, colors=col), M.render(v, f, h, w, M.intrinsics(h, w, K=K), poses, colors=col))


def test_a_rotation_that_is_not_orthonormal_uses_whole_image_boxes():
    v, f, poses = CASES["sphere"]
    p = poses[:1].copy()
    p[0, :3, :3] *= np.float32(1.05)
    p[0, 0, 1] += np.float32(0.1)
    col = M.vertex_colors(v)
    got = gpu_render(v, f, p, colors=col)
    same(got, M.render(v, f, H, W, INTR, p, colors=col))
    assert got["counts"][2] == len(f)


def test_more_faces_than_one_grid_stride_launch():
    """270 000 faces that repeat an index, then the sphere: the image is the sphere's with every face id shifted"""
    v, f, poses = CASES["sphere"]
    pad = 270000
    assert pad + len(f) > 1024 * 256
    junk = np.repeat(np.array([[3, 3, 7]], np.int32), pad, 0)
    col = M.vertex_colors(v)
    got = gpu_render(v, np.concatenate([junk, f]), poses, colors=col)
    want = replay("sphere")
    assert got["counts"].tolist() == [pad] + want["counts"].tolist()[1:]
    shifted = np.where(want["face"] >= 0, want["face"] + pad, -1)
    assert np.array_equal(got["face"].reshape(3, -1), shifted)
    for k in ("depth", "disp", "acc", "bary", "rgb"):
        assert got[k].reshape(want[k].shape).tobytes() == want[k].tobytes(), k


def test_more_pixels_than_one_grid_stride_launch():
    v, f, poses = CASES["sphere"]
    h, w = 520, 512
    assert h * w > 1024 * 256
    col = M.vertex_colors(v)
    got = gpu_render(v, f, poses[:1], h, w, focal=700.0, colors=col, background=BG)
    pix = np.unique(np.concatenate([np.random.default_rng(11).choice(h * w, 4096, replace=False), np.arange((h - 2) * w, h * w)]))
    want = M.render(v, f, h, w, M.intrinsics(h, w, focal=700.0), poses[:1], colors=col, background=BG, pixels=pix, want_counts=False)
    assert 500 < want["acc"].sum() < len(pix)
    assert np.array_equal(got["face"].reshape(1, -1)[:, pix], want["face"])
    for k in ("depth", "disp", "acc"):
        assert got[k].reshape(1, -1)[:, pix].tobytes() == want[k].tobytes(), k
    for k in ("bary", "rgb"):
        assert got[k].reshape(1, -1, 3)[:, pix].tobytes() == want[k].tobytes(), k
    miss = got["face"] < 0
    assert miss.any() and (~miss).any() and (got["acc"] == (~miss)).all()
    assert (got["depth"][miss] == 0).all() and (got["disp"][miss] == 0).all() and (got["bary"][miss] == 0).all()
    assert (got["rgb"][miss] == np.array(BG, np.float32)).all()
    assert (got["depth"][~miss] > 0).all() and got["counts"][3] >= (~miss).sum()


# ---------------------------------------------------------------------------------------------------------------- compare_views
def test_compare_views_against_numpy():
    from swnerf import mesh
    want = replay("sphere")
    acc, depth = want["acc"].reshape(3, H, W), want["depth"].reshape(3, H, W)
    rng = np.random.default_rng(3)
    ref_depth = (depth + rng.standard_normal(depth.shape).astype(np.float32) * np.float32(0.02)).astype(np.float32)
    alpha = np.clip(np.roll(acc, 3, 2) * 0.8 + rng.random(acc.shape) * 0.3, 0, 1).astype(np.float32)
    frames = rng.integers(0, 256, (3, H, W, 4), dtype=np.uint8)
    frames[..., 3] = np.where(np.roll(acc, -2, 1) > 0, rng.integers(100, 256, acc.shape), rng.integers(0, 140, acc.shape))
    out = dict(acc=dev(acc), depth=dev(depth))
    for a, d in ((alpha, ref_depth), (frames[..., 3], ref_depth), (alpha, None), (None, ref_depth)):
        cnt, sums = M.compare(acc, depth, a, d)
        got = mesh.compare_views(out, alpha=None if a is None else dev(a if a.dtype == np.float32 else frames), depth=None if d is None else dev(d))
        assert [got[k].tolist() for k in ("intersection", "union", "mesh_pixels", "ref_pixels")] == cnt.T.tolist()
        assert got["abs_sum"].tobytes() == sums[:, 0].tobytes() and got["sq_sum"].tobytes() == sums[:, 1].tobytes()
        assert got["depth_pixels"].tolist() == sums[:, 2].astype(np.int64).tolist()
        assert np.allclose(got["iou"], cnt[:, 0] / cnt[:, 1], rtol=0, atol=0)
        if d is not None:
            assert (cnt[:, 0] > 0).all() and np.array_equal(got["depth_mae"], sums[:, 0] / sums[:, 2])
            assert np.array_equal(got["depth_rmse"], np.sqrt(sums[:, 1] / sums[:, 2]))
            assert (got["depth_mae"] < 0.05).all()
        else:
            assert np.isnan(got["depth_mae"]).all()
    again = mesh.compare_views(out, alpha=dev(frames), depth=dev(ref_depth))
    first = mesh.compare_views(out, alpha=dev(frames), depth=dev(ref_depth))
    assert again["sq_sum"].tobytes() == first["sq_sum"].tobytes()
    same_mask = mesh.compare_views(out, alpha=dev(acc))
    assert same_mask["iou"].tolist() == [1.0, 1.0, 1.0]


# ----------------------------------------------------------------------------------------------------- the project's depth unit
def test_depth_is_in_the_unit_of_the_nerfs_depth_map():
    """a seeded synthetic net -> nerf_to_mesh -> render_views at a training-style pose, against the net's own render of that pose:
    the silhouettes overlap and the depths subtract directly (t along the unnormalised rays_d).  The sizes of IoU and depth error are
    printed, not gated: they measure how sharp the seeded net's surface is."""
    from swnerf import synth, model, mesh, render
    from oracle import nerf_oracle as O
    net = model.vallina_NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
    seed, ab = synth.NET_FINE
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.nerf_state_dict(seed, alpha_bias=ab).items()})
    net = net.to(DEV).eval()
    h = w = 40
    K, c2w = synth.lego_camera(h, w)
    with torch.no_grad():
        m = mesh.nerf_to_mesh(net, [(-1., 1.), (-1., 2.), (-4., 2.)], resolution=40, density_threshold=0.5, num_views=8, clean={"keep": "all"})
        assert len(m.faces) > 0
        o, d = synth.rays_numpy(h, w, K, c2w)
        maps = render.render_pass(O.make_ray_batch(torch.from_numpy(o), torch.from_numpy(d), 2., 6.).to(DEV), net, 128, want=["acc_map", "depth_map"])
        out = mesh.render_views(m, h, w, K, c2w[None], shading="headlight")
        res = mesh.compare_views(out, alpha=maps["acc_map"].reshape(1, h, w), depth=maps["depth_map"].reshape(1, h, w))
    print(f"synthetic net, {len(m.faces)} faces: IoU {res['iou'][0]:.4f}, depth MAE {res['depth_mae'][0]:.4f}, RMSE {res['depth_rmse'][0]:.4f} "
          f"over {res['depth_pixels'][0]} pixels (mesh {res['mesh_pixels'][0]}, NeRF {res['ref_pixels'][0]} of {h * w})")
    assert res["iou"][0] > 0
    assert np.isfinite(res["depth_mae"][0]) and res["depth_pixels"][0] == res["intersection"][0]


def test_the_example_runs(tmp_path):
    import importlib.util
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    spec = importlib.util.spec_from_file_location("render_mesh_views", os.path.join(root, "examples", "render_mesh_views.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    res, rgbs, disps = ex.main(str(tmp_path), resolution=32, side=32, views=2)
    assert rgbs.shape == (2, 32, 32, 3) and disps.shape == (2, 32, 32) and len(res["iou"]) == 2
    assert sorted(os.listdir(tmp_path / "turntable")) == ["000.png", "001.png", "video.avi"]


# ------------------------------------------------------------------------------------------------------------------- the runners
def test_render_path_mesh_writes_frames_and_a_video(tmp_path):
    import avi_ref
    from swnerf import mesh, runner, png
    v, f, poses = CASES["sphere"]
    m = mesh.Mesh(v, f, R.vertex_normals(v, f).astype(np.float32), M.vertex_colors(v))
    rgbs, disps = runner.render_path_mesh(m, poses, [H, W, FOCAL], None, savedir=str(tmp_path), video=True)
    want = M.render(v, f, H, W, INTR, poses, shading=2, colors=M.vertex_colors(v), normals=m.vertex_normals, background=(1., 1., 1.), want_counts=False)
    assert rgbs.shape == (3, H, W, 3) and disps.shape == (3, H, W)
    assert rgbs.tobytes() == want["rgb"].tobytes() and disps.tobytes() == want["disp"].tobytes()
    for i in range(3):
        img = png.read_png(os.path.join(tmp_path, f"{i:03d}.png"))
        assert img.shape == (H, W, 3) and np.array_equal(img, (255 * np.clip(rgbs[i], 0, 1)).astype(np.uint8))
    avi = avi_ref.parse(open(os.path.join(tmp_path, "video.avi"), "rb").read())
    assert (avi["width"], avi["height"], avi["total_frames"], len(avi["frames"])) == (W, H, 3, 3) and avi["handler"] in (b"MJPG", b"mjpg")
    half, _ = runner.render_path_mesh(m, poses[:1], [H, W, FOCAL], None, render_factor=2, shading="normals")
    assert half.shape == (1, H // 2, W // 2, 3)
    with pytest.raises(ValueError, match="savedir"):
        runner.render_path_mesh(m, poses, [H, W, FOCAL], None, video=True)


def test_evaluate_mesh_on_an_in_memory_dataset(tmp_path):
    from swnerf import mesh, runner
    v, f, poses = CASES["sphere"]
    m = mesh.Mesh(v, f, R.vertex_normals(v, f).astype(np.float32), M.vertex_colors(v))
    want = replay("sphere")
    acc = want["acc"].reshape(3, H, W)
    images = np.zeros((4, H, W, 4), np.uint8)
    images[[0, 1, 3], ..., 3] = (acc * 255).astype(np.uint8)            # frames 0, 1, 3 are the training split; frame 2 is empty
    images[3, :, :5, 3] = 255                                           # frame 3's mask is wider than the object
    all_poses = np.stack([poses[0], poses[1], poses[0], poses[2]])
    data = dict(images=dev(images), poses=all_poses, hwf=[H, W, FOCAL], K=None, i_split=[np.array([0, 1, 3]), np.array([2]), np.array([], np.int64)])
    rep = runner.evaluate_mesh(m, data)
    assert rep["frame"] == [0, 1, 3] and rep["iou"][:2] == [1.0, 1.0] and 0.5 < rep["iou"][2] < 1.0
    assert rep["mesh_pixels"] == acc.sum((1, 2)).astype(np.int64).tolist() and not os.listdir(tmp_path)
    depth = want["depth"].reshape(3, H, W)
    rep = runner.evaluate_mesh(m, data, net_depths=dev(depth + np.float32(0.5) * (depth > 0)), savedir=str(tmp_path / "eval"))
    assert np.allclose(rep["depth_mae"], 0.5, atol=1e-6) and np.allclose(rep["depth_rmse"], 0.5, atol=1e-6)
    assert sorted(os.listdir(tmp_path / "eval")) == ["000.png", "001.png", "002.png", "mesh_eval.json"]
    val = runner.evaluate_mesh(m, data, split="val")
    assert val["frame"] == [2] and val["iou"] == [0.0] and val["ref_pixels"] == [0]
