"""Host side of runner.train_multires (no GPU): the clipped patch sizes, the order in which sampler="numpy" consumes the reference's
random streams, the keyed draws of sampler="device", and the float64 restatement of the joint loss (tests/multires_loss_ref.py)
against finite differences."""
import random

import numpy as np
import pytest
import torch

import multires_loss_ref as M
from swnerf import batching, runner


def _hwf(H, W, levels):
    return runner.pyramid_hwf([H, W, 1.2 * W], levels)


# ---- clipped patch sizes ----------------------------------------------------------------------------------------------------
def test_patch_size_list():
    assert runner.multires_patch_sizes(4) == [32, 16, 8, 4]
    assert runner.multires_patch_sizes(2) == [32, 16] and runner.multires_patch_sizes(1) == [32]


def test_clipped_sizes_40x56():
    hwf = _hwf(40, 56, 4)
    assert [tuple(h[:2]) for h in hwf] == [(40, 56), (20, 28), (10, 14), (5, 7)]
    coords = runner.initialize_patches(hwf, base_patch_size=32, cur_iter=0)
    assert coords == [(0, 0)] * 4                          # the coarsest level is not larger than the base patch
    assert batching.clipped_patch_sizes(hwf, coords, [32, 16, 8, 4]) == [(32, 32), (16, 16), (8, 8), (4, 4)]
    assert batching.clipped_patch_sizes(hwf, [(0, 0)] * 4, [8, 4, 2, 1]) == [(8, 8), (4, 4), (2, 2), (1, 1)]
    assert batching.clipped_patch_sizes(hwf, [(20, 40), (10, 20), (5, 10), (2, 5)], [32, 16, 8, 4]) == [(20, 16), (10, 8), (5, 4), (3, 2)]


def test_clipped_sizes_36x52():
    hwf = _hwf(36, 52, 4)
    assert [tuple(h[:2]) for h in hwf] == [(36, 52), (18, 26), (9, 13), (4, 6)]
    assert batching.clipped_patch_sizes(hwf, [(0, 0)] * 4, [32, 16, 8, 4]) == [(32, 32), (16, 16), (8, 8), (4, 4)]
    # a corner that clips levels 2 and 3 only: 9 - 2 = 7 < 8, 13 - 6 = 7 < 8; 4 - 1 = 3 < 4, 6 - 3 = 3 < 4
    assert batching.clipped_patch_sizes(hwf, [(2, 4), (1, 2), (2, 6), (1, 3)], [32, 16, 8, 4]) == [(32, 32), (16, 16), (7, 7), (3, 3)]


def test_clipped_sizes_12x20_every_level_is_its_patch():
    hwf = _hwf(12, 20, 2)
    coords = runner.initialize_patches(hwf, base_patch_size=32, cur_iter=5000)
    assert coords == [(0, 0), (0, 0)]
    assert batching.clipped_patch_sizes(hwf, coords, runner.multires_patch_sizes(2)) == [(12, 20), (6, 10)]
    assert batching.patch_corners(123, hwf, 32, 0) == [(0, 0), (0, 0)]


def test_clipped_sizes_refuse_a_corner_outside():
    hwf = _hwf(12, 20, 2)
    for coords, sizes in (([(12, 0), (0, 0)], [32, 16]), ([(0, 0), (0, 10)], [32, 16]), ([(0, 0), (0, 0)], [32, 0]), ([(0, 0)], [32, 16])):
        with pytest.raises(ValueError):
            batching.clipped_patch_sizes(hwf, coords, sizes)


# ---- sampler="numpy": the reference's streams in the reference's order ------------------------------------------------------
def test_numpy_sampler_draw_order():
    hwf = _hwf(400, 480, 4)                                # coarsest level 50 x 60: larger than the base patch, so corners are drawn
    i_train = np.arange(3, 20)
    iters = [3997, 3998, 3999, 4000, 4001, 4002]           # both sides of get_random_patch_coords' current_iter < n switch

    def seed():
        random.seed(7)
        torch.manual_seed(7)
        np.random.seed(7)
    seed()
    got = [runner._multires_draw("numpy", 0, i, hwf, i_train) for i in iters]
    seed()
    want = []
    for i in iters:
        coords = runner.initialize_patches(hwf, base_patch_size=32, cur_iter=i)      # patches first ...
        want.append((coords, np.random.choice(i_train)))                             # ... then the frame
    assert got == want
    assert len({c[3] for c, _ in got}) > 1 and len({f for _, f in got}) > 1
    for coords, _ in got:
        assert all(coords[l] == (coords[3][0] << (3 - l), coords[3][1] << (3 - l)) for l in range(4))


# ---- sampler="device": the keyed draws --------------------------------------------------------------------------------------
def test_keyed_draws_are_functions_of_the_key():
    k1, k2 = batching.batch_key(3, 17, 2), batching.batch_key(3, 18, 2)
    assert k1 != k2 and k1 != batching.batch_key(3, 17, 0)
    for f in (lambda k: batching.key_uniform(k, 0), lambda k: batching.key_randint(k, 1, -5, 9), lambda k: batching.key_normal(k, 2, 1.0, 3.0),
              lambda k: batching.patch_corner(k, 50, 60, 32, 10), lambda k: batching.patch_corner(k, 50, 60, 32, 5000)):
        assert f(k1) == f(k1) and f(k1) != f(k2)
    hwf, i_train = _hwf(400, 480, 4), np.arange(3, 20)
    assert runner._multires_draw("device", 5, 9, hwf, i_train) == runner._multires_draw("device", 5, 9, hwf, i_train)
    draws = [runner._multires_draw("device", 5, i, hwf, i_train) for i in range(200)]
    assert {int(f) for _, f in draws} == set(i_train.tolist())                       # every training frame is reached
    assert batching.key_randint(1, 0, 4, 4) == 4
    with pytest.raises(ValueError):
        batching.key_randint(1, 0, 5, 4)


def test_keyed_draw_statistics():
    u = np.array([batching.key_uniform(batching.batch_key(0, i, 2), 0) for i in range(10000)])
    assert 0.0 <= u.min() and u.max() < 1.0 and abs(u.mean() - 0.5) < 0.02
    z = np.array([batching.key_normal(batching.batch_key(0, i, 2), 0, 2.0, 3.0) for i in range(10000)])
    assert abs(z.mean() - 2.0) < 0.15 and abs(z.std() - 3.0) < 0.15
    r = np.array([batching.key_randint(batching.batch_key(0, i, 2), 0, -2, 4) for i in range(10000)])
    assert set(r.tolist()) == set(range(-2, 5))


def test_keyed_corners_stay_inside():
    H, W, patch = 50, 60, 32
    cy, cx = (H - patch) / 2, (W - patch) / 2
    seen_lo, seen_hi = set(), set()
    for i in range(10000):
        key = batching.batch_key(11, i, 2)
        y, x = batching.patch_corner(key, H, W, patch, 100)          # before iteration n: the centre region of get_random_patch_coords
        assert max(0, int(cy - H / 8)) <= y <= min(int(cy + H / 8), H - patch)
        assert max(0, int(cx - W / 8)) <= x <= min(int(cx + W / 8), W - patch)
        seen_lo.add((y, x))
        y, x = batching.patch_corner(key, H, W, patch, 4000)         # from n on: normal, clipped into the image
        assert 0 <= y <= H - patch and 0 <= x <= W - patch
        seen_hi.add((y, x))
    assert {y for y, _ in seen_hi} == set(range(H - patch + 1))      # sigma = H / 4 reaches every admissible corner
    assert {y for y, _ in seen_lo} == set(range(max(0, int(cy - H / 8)), min(int(cy + H / 8), H - patch) + 1))
    hwf = _hwf(400, 480, 4)
    for i in (0, 3999, 4000, 9000):
        coords = batching.patch_corners(batching.batch_key(1, i, 2), hwf, 32, i)
        for (Hl, Wl, _), (y, x), ps in zip(hwf, coords, [32, 16, 8, 4]):
            assert 0 <= y < Hl and 0 <= x < Wl


# ---- the float64 restatement against finite differences ---------------------------------------------------------------------
@pytest.mark.parametrize("add_global", [False, True])
def test_restatement_gradients_match_finite_differences(add_global):
    rng = np.random.default_rng(5)
    sizes = [(8, 8), (4, 4), (2, 2), (1, 1)]
    rgbs = [rng.random((h, w, 3)) for h, w in sizes]
    rgb0s = [rng.random((h, w, 3)) if l != 2 else None for l, (h, w) in enumerate(sizes)]
    targets = [rng.random((h, w, 3)) - 0.3 for h, w in sizes]
    full = rng.random((8, 8, 3))
    out = M.loss_and_grads(rgbs, rgb0s, targets, full, add_global)
    want = sum(out["per_level"]) + sum(m for m in out["per_level0"] if m is not None) + (out["global_loss"] if add_global else 0.0)
    assert out["loss"] == pytest.approx(want, rel=1e-15) and out["per_level0"][2] is None and out["d_rgb0"][2] is None
    eps = 1e-6
    for which, arrs, grads in (("rgb", rgbs, out["d_rgb"]), ("rgb0", rgb0s, out["d_rgb0"])):
        for l, (a, g) in enumerate(zip(arrs, grads)):
            if a is None:
                continue
            fd = np.zeros_like(a)
            for idx in np.ndindex(a.shape):
                keep = a[idx]
                a[idx] = keep + eps
                hi = M.loss_and_grads(rgbs, rgb0s, targets, full, add_global)["loss"]
                a[idx] = keep - eps
                lo = M.loss_and_grads(rgbs, rgb0s, targets, full, add_global)["loss"]
                a[idx] = keep
                fd[idx] = (hi - lo) / (2 * eps)
            assert np.abs(fd - g).max() <= 1e-9, (which, l, np.abs(fd - g).max())        # the loss is quadratic: central differences are exact up to rounding
    if add_global:                                                                       # the global term does reach every level
        base = M.loss_and_grads(rgbs, rgb0s, targets, full, False)["d_rgb"]
        assert all(np.abs(a - b).max() > 1e-4 for a, b in zip(out["d_rgb"], base))
