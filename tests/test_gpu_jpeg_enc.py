"""Baseline JPEG frames encoded on the GPU (csrc/jpeg_enc_kernels.hip behind swnerf.images.encode_jpegs, swnerf.video): every
byte of every file must equal what libjpeg writes for the same pixels, quality and sampling, which g20_jpeg_enc.npz
(tests/golden/make_golden_jpeg_enc.py) recorded through PIL.  The fixtures are the smallest frames at which each rule can go
wrong: 1 x 1; 8 x 8 (a dummy luma row and column at 4:2:0); 24 x 8 (a dummy column); 17 x 23; 40 x 72 (a dummy luma row); 50 x 35
(the last chroma row averages two different rows, an odd width, partial blocks) - each at 4:4:4, 4:2:2, 4:2:0 and grey, at
qualities 8, 50, 90 and 100, with random, smooth and near-constant content."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import avi_ref
import jpeg_enc_ref as R
import jpeg_ref
from swnerf import _lib, images, runner, synth, video

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g20_jpeg_enc.npz")


@pytest.fixture(scope="module")
def g20():
    return dict(np.load(GOLDEN, allow_pickle=False))


@pytest.fixture(scope="module")
def files(g20):
    return R.golden_files(g20)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_every_fixture_equals_libjpeg_byte_for_byte(g20, files):
    """one call per geometry and quality: the three contents of a size go in as one stack"""
    cases = R.golden_cases(g20)
    assert len(cases) == 288
    seen = 0
    for hw in ("1x1", "8x8", "24x8", "17x23", "40x72", "50x35"):
        stack = np.stack([g20[f"px_{hw}_{kind}"] for kind in ("random", "ramp", "flat")])
        for s in ("444", "422", "420", "gray"):
            px = _dev(stack[..., 1:2] if s == "gray" else stack)                  # [N,H,W,1]: a 3-D [3,1,1] would read as one frame
            for q in (8, 50, 90, 100):
                got = images.encode_jpegs(px, quality=q, subsampling=R.SUBSAMPLING_OF[s], components=1 if s == "gray" else 3)
                for kind, data in zip(("random", "ramp", "flat"), got):
                    assert data == files[f"{hw}_{kind}_{s}_q{q}"], (hw, kind, s, q)
                    seen += 1
    assert seen == 288


def test_coefficients_equal_the_entropy_decode_of_the_golden_file(g20, files):
    """the raw device output, dummy blocks included, in the layout swnerf_jpeg_entropy produces"""
    for n, px, ncomp, s, q in R.golden_cases(g20):
        if "_random_" not in n or q not in (8, 90):
            continue
        j = images._jpeg_header(files[n], n)
        coef = images.encode_coefficients(_dev(px), R.quant_tables(q), R.SUBSAMPLING_OF[s], components=ncomp)
        assert coef.shape == (1, j.ncoef) and coef.dtype == torch.int16
        np.testing.assert_array_equal(coef[0].cpu().numpy(), j.coefficients(), err_msg=n)


def test_stack_channels_and_host_input(g20, files):
    want = [files[f"stack_{k}"] for k in range(3)]
    stack = g20["stack_px"]
    assert images.encode_jpegs(_dev(stack)) == want                                        # quality 90, 4:2:0, 3 components: the defaults
    assert images.encode_jpegs(stack) == want                                              # a numpy array goes up through pinned staging
    assert images.encode_jpegs(stack, chunk_bytes=1) == want                               # one frame per chunk: both staging buffers in turn
    assert images.encode_jpegs(_dev(stack), chunk_bytes=1) == want
    rgba = np.concatenate([stack, np.full(stack.shape[:3] + (1,), 9, np.uint8)], -1)
    assert images.encode_jpegs(_dev(rgba)) == want and images.encode_jpegs(rgba) == want   # alpha is ignored
    assert images.encode_jpegs(_dev(stack[1])) == want[1:2] and images.encode_jpegs(stack[1]) == want[1:2]       # one frame, no leading N
    assert images.encode_jpegs(_dev(stack)[:, :, :, :3].flip(0).flip(0)) == want
    f32 = (stack / np.float32(255)).astype(np.float32)                                     # to8b(u / 255) == u for every byte
    assert np.array_equal(R.to8b(f32), stack) and images.encode_jpegs(_dev(f32)) == want
    # one channel: R = G = B with 3 components (the default), Y alone with components=1
    g = stack[..., 1]
    as_rgb = [R.encode(np.repeat(f[..., None], 3, -1), 90, R.S420) for f in g]
    assert images.encode_jpegs(_dev(g)) == as_rgb and images.encode_jpegs(g[..., None]) == as_rgb and images.encode_jpegs(_dev(g[0])) == as_rgb[:1]
    assert images.encode_jpegs(_dev(g), components=1) == [R.encode(f, 90, R.S444, 1) for f in g]
    assert images.encode_jpegs(_dev(g), components=1, subsampling="4:2:2") == [R.encode(f, 90, R.S444, 1) for f in g]     # grey has one sampling
    assert images.encode_jpegs(_dev(stack[:0])) == []
    with pytest.raises(ValueError, match="components"):
        images.encode_jpegs(_dev(stack), components=1)
    with pytest.raises(ValueError, match="subsampling"):
        images.encode_jpegs(_dev(stack), subsampling="4:1:1")
    with pytest.raises(TypeError):
        images.encode_jpegs(stack.astype(np.float64))
    with pytest.raises(ValueError, match="frames must be"):
        images.encode_jpegs(_dev(stack)[..., :2])


def test_float_frames_and_divisor(g20, files):
    f, disp, top = g20["float_px"], g20["disp_px"], float(g20["disp_max"])
    want_f, want_d = [files["float_0"], files["float_1"]], [files["disp_0"], files["disp_1"]]
    assert images.encode_jpegs(_dev(f)) == want_f and images.encode_jpegs(f) == want_f
    assert images.encode_jpegs(_dev(disp), divisor=top) == want_d and images.encode_jpegs(disp, divisor=top) == want_d
    assert images.encode_jpegs(_dev(disp[..., None]), divisor=np.float32(top)) == want_d
    # a divisor is a division, not a multiplication by a reciprocal: x / 3 for x = 3 k / 255 lands on k / 255's float or its neighbour
    x = (np.arange(256, dtype=np.float32) * np.float32(3) / np.float32(255)).reshape(1, 16, 16)
    assert images.encode_jpegs(_dev(x), divisor=3.0, subsampling="4:4:4") == [R.encode(np.repeat(R.to8b(x[0], 3.0)[..., None], 3, -1), 90, R.S444)]


def test_round_trip_equals_libjpegs_decode(g20, files):
    """decode_jpegs(encode_jpegs(x)): the pixels libjpeg decodes from its own file (tests/jpeg_ref.py from the file's coefficients,
    itself pinned to PIL's decode by g19_jpeg.npz)"""
    for n, px, ncomp, s, q in R.golden_cases(g20):
        if not (n.startswith(("50x35_random", "17x23_ramp", "8x8_random", "1x1_flat")) and q in (50, 90)):
            continue
        data = images.encode_jpegs(_dev(px), quality=q, subsampling=R.SUBSAMPLING_OF[s], components=ncomp)
        assert data == [files[n]]
        j = images._jpeg_header(files[n], n)
        want = jpeg_ref.decode(j.coefficients(), j.qt, j.H, j.W, j.ncomp, j.sampling)
        got = images.decode_jpegs(data, device=DEV)
        np.testing.assert_array_equal(got[0].cpu().numpy(), want, err_msg=n)
    # and without the host in between: the device's coefficients straight into swnerf_jpeg_decode
    px, q = g20["px_50x35_random"], 90
    qt = R.quant_tables(q)
    coef = images.encode_coefficients(_dev(px), qt, "4:2:0")
    out = torch.empty((1, 50, 35, 3), dtype=torch.uint8, device=DEV)
    images._jpeg_decode_into(coef, _dev(np.ascontiguousarray(qt[[0, 1, 1]]).view(np.int16)), 1, 50, 35, 3, _lib.JPEG_420, out)
    j = images._jpeg_header(files["50x35_random_420_q90"], "f")
    np.testing.assert_array_equal(out[0].cpu().numpy(), jpeg_ref.decode(j.coefficients(), j.qt, 50, 35, 3, _lib.JPEG_420))


def test_write_jpeg_and_write_video(g20, files, tmp_path):
    stack = g20["stack_px"]
    images.write_jpeg(tmp_path / "one.jpg", _dev(stack[2]))
    assert (tmp_path / "one.jpg").read_bytes() == files["stack_2"]
    images.write_jpeg(tmp_path / "q8.jpg", g20["px_50x35_ramp"], quality=8, subsampling="4:2:2")
    assert (tmp_path / "q8.jpg").read_bytes() == files["50x35_ramp_422_q8"]
    with pytest.raises(ValueError, match="one frame"):
        images.write_jpeg(tmp_path / "no.jpg", _dev(stack))
    assert video.write_video(tmp_path / "v.avi", _dev(stack), fps=30) == str(tmp_path / "v.avi")
    o = avi_ref.parse((tmp_path / "v.avi").read_bytes())
    assert o["frames"] == images.encode_jpegs(_dev(stack)) == [files[f"stack_{k}"] for k in range(3)]
    assert (o["total_frames"], o["stream_frames"], o["width"], o["height"], o["rate"], o["scale"]) == (3, 3, 23, 17, 30, 1)
    assert video.mimwrite(str(tmp_path / "m.mp4"), [f for f in stack], fps=30, quality=8) == str(tmp_path / "m.avi")
    assert avi_ref.parse((tmp_path / "m.avi").read_bytes())["frames"] == o["frames"]
    assert sorted(os.listdir(tmp_path)) == ["m.avi", "one.jpg", "q8.jpg", "v.avi"]


def test_train_writes_the_spiral_videos(tmp_path):
    """two iterations of runner.train with i_video = 2 on synthetic frames and a two-pose render path: both .avi files hold 2
    frames; the rgb frames are libjpeg's files of to8b(rgbs) and decode to exactly what PIL decodes from its own encode of
    to8b(rgbs); the disparity frames likewise of to8b(disps / np.max(disps))."""
    import io
    from PIL import Image
    H = W = 16
    rng = np.random.default_rng(2)
    imgs = rng.uniform(0, 1, (1, H, W, 3)).astype(np.float32)
    poses = np.stack([synth.pose_spherical(30.0 + 40.0 * i, -30.0, 4.0) for i in range(2)]).astype(np.float32)
    focal = float(0.5 * W / np.tan(0.5 * synth.LEGO_CAMERA_ANGLE_X))
    data = (imgs, poses[:1], poses, [H, W, focal], [[0], [], []], 2., 6.)
    args = SimpleNamespace(expname="loop", basedir=str(tmp_path), netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, lrate=5e-4,
                           lrate_decay=500, netchunk=1024 * 64, no_reload=True, ft_path=None, N_samples=64, N_importance=128, perturb=1.,
                           use_viewdirs=True, i_embed=0, multires=10, multires_views=4, raw_noise_std=0., dataset_type="blender",
                           white_bkgd=True, no_ndc=False, lindisp=False, chunk=1024 * 32, N_rand=256, no_batching=True, precrop_iters=0,
                           precrop_frac=.5, i_print=1000, i_weights=1000, i_testset=100000, N_iters=2, seed=0, i_video=2)
    seen = {}
    torch.manual_seed(0)
    np.random.seed(0)
    rec = runner.train(args, data, device=DEV, hooks={"on_video": lambda i, rgbs, disps: seen.update(i=i, rgbs=rgbs.copy(), disps=disps.copy())})
    assert len(rec) == 2 and seen["i"] == 2 and seen["rgbs"].shape == (2, H, W, 3) and seen["disps"].shape == (2, H, W)
    out = os.path.join(str(tmp_path), "loop")
    assert sorted(f for f in os.listdir(out) if f.endswith(".avi")) == ["loop_spiral_000002_disp.avi", "loop_spiral_000002_rgb.avi"]
    rgb8 = R.to8b(seen["rgbs"])
    disp8 = np.repeat(R.to8b(seen["disps"], np.max(seen["disps"]))[..., None], 3, -1)
    for name, frames8 in (("rgb", rgb8), ("disp", disp8)):
        with open(os.path.join(out, f"loop_spiral_000002_{name}.avi"), "rb") as f:
            o = avi_ref.parse(f.read())
        assert (o["total_frames"], o["width"], o["height"], o["rate"], o["scale"]) == (2, W, H, 30, 1) and len(o["frames"]) == 2
        for k in range(2):
            buf = io.BytesIO()
            Image.fromarray(frames8[k], "RGB").save(buf, format="JPEG", quality=90, subsampling=2)
            assert o["frames"][k] == buf.getvalue(), (name, k)
            want = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
            got = images.decode_jpegs([o["frames"][k]], device=DEV)[0].cpu().numpy()
            np.testing.assert_array_equal(got, want, err_msg=f"{name} {k}")
