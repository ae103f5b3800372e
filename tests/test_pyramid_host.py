"""CPU-only checks of the MultiRes D-NeRF host side: the float64 restatement tests/pyramid_ref.py against the golden G15
(tests/golden/make_golden_pyramid.py: the reference's multires_dnerf/pyramid.py on CPU), create_gaussian_kernel, the
level sizes and patch sampling of swnerf.runner, the MultiRes checkpoint format, and the argument errors of
swnerf.pyramid and of its C entry points (raised before any device call)."""
import os
import random
import types

import numpy as np
import pytest
import torch

import pyramid_ref as R
from make_golden_pyramid import CASES, LEVELS, case_input
from swnerf import _lib, checkpoint, pyramid, runner

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_pyramid.npz")


@pytest.fixture(scope="module")
def g15():
    return dict(np.load(GOLDEN, allow_pickle=False))


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_golden_within_ref_dist(g15, name):
    _, shape, k, sigma = CASES[name]
    x = g15[f"{name}_input"]
    assert x.shape == shape and np.array_equal(x, case_input(name))
    want = R.generate(x, LEVELS, k, sigma)
    dist = g15[f"{name}_ref_dist"]
    assert dist.shape == (LEVELS + 1,) and dist.max() < 1e-6          # the reference is fp32-close to the restatement
    for l in range(LEVELS):
        got = g15[f"{name}_level{l}"]
        assert got.shape == (shape[0], shape[1] >> l, shape[2] >> l, 3)
        assert np.abs(got - want[l]).max() <= dist[l]
    rec = R.reconstruct([g15[f"{name}_level{l}"] for l in range(LEVELS)])
    assert np.abs(g15[f"{name}_recon"] - rec).max() <= dist[LEVELS]
    assert np.abs(R.reconstruct(want) - x).max() < 1e-14             # the pyramid is exactly invertible


def test_adjoint_is_the_transpose_of_up():
    rng = np.random.default_rng(3)
    for (h, w), (H, W) in (((4, 6), (9, 13)), ((8, 8), (16, 16)), ((5, 7), (5, 7)), ((3, 2), (7, 9))):
        x, g = rng.random((2, h, w, 3)), rng.random((2, H, W, 3))
        assert abs((R.up(x, (H, W)) * g).sum() - (x * R.up_adjoint(g, (h, w))).sum()) < 1e-10


@pytest.mark.parametrize("name", sorted(CASES))
def test_create_gaussian_kernel_is_bit_equal(g15, name):
    _, _, k, sigma = CASES[name]
    got = pyramid.create_gaussian_kernel(k, sigma)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 1, k, k)
    assert np.array_equal(got.numpy(), g15[f"{name}_kernel"])
    assert tuple(pyramid.create_gaussian_kernel(k, sigma, channels=1).shape) == (1, 1, k, k)


def test_pyramid_hwf():
    assert runner.pyramid_hwf([800, 800, 1111.0], 4) == [[800, 800, 1111.0], [400, 400, 555.5], [200, 200, 277.75], [100, 100, 138.875]]
    assert runner.pyramid_hwf([37.0, 53, 50.0], 4) == [[37, 53, 50.0], [18, 26, 25.0], [9, 13, 12.5], [4, 6, 6.25]]
    with pytest.raises(ValueError):
        runner.pyramid_hwf([4, 4, 1.0], 4)


@pytest.mark.parametrize("side", [400, 800])
def test_initialize_patches_double_and_stay_inside(side):
    pyr_hwf = runner.pyramid_hwf([side, side, 500.0], 4)
    patch = [32 // 2 ** l for l in range(4)]
    random.seed(7)
    torch.manual_seed(7)
    seen = set()
    for draw in range(200):
        cur = 0 if draw % 2 == 0 else 5000                               # both sides of n = 4000
        coords = runner.initialize_patches(pyr_hwf, base_patch_size=32, cur_iter=cur)
        assert len(coords) == 4
        for l in range(3):
            assert coords[l] == (2 * coords[l + 1][0], 2 * coords[l + 1][1])
        for l, (y, x) in enumerate(coords):
            H, W, _ = pyr_hwf[l]
            assert 0 <= y and y + patch[l] <= H and 0 <= x and x + patch[l] <= W, (draw, l, coords)
        seen.add(coords[3])
    assert len(seen) > 20                                                # the draws do move


def test_get_random_patch_coords_small_image():
    assert runner.get_random_patch_coords(16, 64, 16, 0) == (0, 0)
    assert runner.get_random_patch_coords(64, 8, 16, 9999) == (0, 0)


def _args(**over):
    a = dict(layer_num=3, use_viewdirs=True, N_importance=8, N_samples=8, nerf_type="direct_temporal", netdepth=8, netwidth=32,
             netdepth_fine=8, netwidth_fine=32, use_two_models_for_fine=False, not_zero_canonical=False, netchunk=1 << 16,
             lrate=5e-4, basedir=None, expname="exp", ft_path=None, no_reload=False, perturb=1.0, white_bkgd=True,
             raw_noise_std=0.0, dataset_type="blender", no_ndc=False, lindisp=False, do_half_precision=False,
             chunk=1 << 15, global_optimization_epoch=10)
    a.update(over)
    return types.SimpleNamespace(**a)


@pytest.mark.parametrize("two", [False, True])
def test_multires_checkpoint_round_trip(tmp_path, two):
    args = _args(basedir=str(tmp_path), use_two_models_for_fine=two)
    os.makedirs(tmp_path / "exp")
    trains, tests, starts, grads, opts = runner.create_multires(args, device="cpu")
    assert starts == [0, 0, 0] and len(trains) == len(tests) == len(grads) == len(opts) == 3
    ins = [(t["network_fn"].input_ch, t["network_fn"].input_ch_time, t["network_fn"].input_ch_views) for t in trains]
    assert ins == [(123, 17, 123), (63, 9, 63), (63, 9, 63)]             # (20, 8, 20), (10, 4, 10), (10, 4, 10)
    assert all((t["network_fine"] is not None) == two for t in trains)
    assert all(t["perturb"] == 1.0 and s["perturb"] is False and "near" not in t for t, s in zip(trains, tests))
    path = checkpoint.save_multires(str(tmp_path), "exp", 7, 7, [t["network_fn"] for t in trains],
                                    [t["network_fine"] for t in trains], opts)
    assert path.endswith("000007.tar")
    keys = set(torch.load(path, weights_only=False))
    want = {"global_step"} | {f"network_fn_{l}" for l in range(3)} | {f"optimizer_{l}" for l in range(3)}
    if two:
        want |= {f"network_fine_{l}" for l in range(3)}
    assert keys == want
    trains2, _, starts2, _, _ = runner.create_multires(args, device="cpu")
    assert starts2 == [7, 7, 7]
    for a, b in zip(trains, trains2):
        for k in ("network_fn", "network_fine"):
            if a[k] is not None:
                for (n1, p1), (n2, p2) in zip(a[k].state_dict().items(), b[k].state_dict().items()):
                    assert n1 == n2 and torch.equal(p1, p2)
    _, _, starts3, _, _ = runner.create_multires(_args(basedir=str(tmp_path), use_two_models_for_fine=two, no_reload=True), device="cpu")
    assert starts3 == [0, 0, 0]


def test_identity_level_and_refusals(tmp_path):
    os.makedirs(tmp_path / "exp")
    trains, *_ = runner.create_multires(_args(basedir=str(tmp_path), layer_num=4), device="cpu")
    net = trains[3]["network_fn"]
    assert (net.input_ch, net.input_ch_time, net.input_ch_views) == (3, 1, 3)      # (-1, -1, -1): identity encoders
    with pytest.raises(NotImplementedError):
        runner.create_multires(_args(basedir=str(tmp_path), do_half_precision=True), device="cpu")
    with pytest.raises(ValueError):
        runner.create_multires(_args(basedir=str(tmp_path), layer_num=5), device="cpu")


def test_argument_errors():
    x = torch.zeros(1, 7, 9, 3)
    with pytest.raises(ValueError, match="7 x 9"):                        # levels too deep: 4 levels need min(H, W) >= 8
        pyramid.generate_laplacian_pyramid_batch(x, levels=4)
    for k in (2, 4, 9, 0):
        with pytest.raises(ValueError, match="kernel_size"):
            pyramid.generate_laplacian_pyramid_batch(torch.zeros(1, 16, 16, 3), kernel_size=k)
    with pytest.raises(NotImplementedError, match="channels"):
        pyramid.generate_laplacian_pyramid_batch(torch.zeros(1, 16, 16, 5))
    with pytest.raises(ValueError):
        pyramid.generate_laplacian_pyramid_batch(torch.zeros(16, 16, 3))
    with pytest.raises(ValueError):
        pyramid.reconstruct_image_from_pyramid_batch([])
    with pytest.raises(ValueError, match="differ"):
        pyramid.reconstruct_image_from_pyramid_batch([torch.zeros(1, 4, 4, 3), torch.zeros(2, 2, 2, 3)])


def test_c_entry_points_validate_before_any_device_call():
    L = _lib.lib()
    for name in ("swnerf_pyramid_down", "swnerf_pyramid_up_axpy", "swnerf_pyramid_up_adjoint"):
        assert name in _lib.EXPORTS
    err = lambda: L.swnerf_last_error().decode()
    assert L.swnerf_pyramid_down(None, 0, 16, 16, 3, None, 3, None, None) == 0            # n == 0: a no-op
    assert L.swnerf_pyramid_up_axpy(None, 0, 4, 4, 3, None, 1.0, 8, 8, None, None) == 0
    assert L.swnerf_pyramid_up_adjoint(None, 0, 8, 8, 3, 4, 4, None, None) == 0
    assert L.swnerf_pyramid_down(None, 1, 16, 16, 3, None, 3, None, None) == -1 and "NULL" in err()
    assert L.swnerf_pyramid_down(None, 1, 16, 16, 3, None, 4, None, None) == -1 and "kernel size" in err()
    assert L.swnerf_pyramid_down(None, 1, 16, 16, 3, None, 9, None, None) == -1 and "kernel size" in err()
    assert L.swnerf_pyramid_down(None, 1, 16, 16, 5, None, 3, None, None) == -1 and "channels" in err()
    assert L.swnerf_pyramid_down(None, 1, 1, 16, 3, None, 3, None, None) == -1 and "half-size" in err()
    assert L.swnerf_pyramid_down(None, -1, 16, 16, 3, None, 3, None, None) == -1
    assert L.swnerf_pyramid_up_axpy(None, 1, 4, 4, 3, None, 1.0, 8, 8, None, None) == -1 and "NULL" in err()
    assert L.swnerf_pyramid_up_axpy(None, 1, 4, 4, 0, None, 1.0, 8, 8, None, None) == -1 and "channels" in err()
    assert L.swnerf_pyramid_up_axpy(None, 1, 4, 4, 3, None, 1.0, 0, 8, None, None) == -1
    assert L.swnerf_pyramid_up_adjoint(None, 1, 8, 8, 3, 4, 4, None, None) == -1 and "NULL" in err()
    assert L.swnerf_pyramid_up_adjoint(None, 1, 8, 8, 3, 4, (1 << 20) + 1, None, None) == -1
