"""CPU-only checks of the training-batch host side (swnerf/batching.py, runner.train): the keyed permutation's numpy definition
(a bijection for every n, different per key, uniform over keys), the schedules against their formulas at the reference's
defaults, the use_batching cursor, the argument refusals of the three new C entry points (returned before anything touches the
GPU) and the signatures of train / train_dnerf."""
import inspect

import numpy as np
import pytest

from swnerf import _lib, batching, runner


@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 64, 65, 1000, 2 ** 16 - 1, 2 ** 16, 2 ** 16 + 1])
def test_perm_index_np_is_a_permutation(n):
    for key in (0, 0x1234_5678_9ABC_DEF0, 2 ** 64 - 1):
        out = batching.perm_index_np(key, n, np.arange(n))
        assert out.dtype == np.int64 and np.array_equal(np.sort(out), np.arange(n)), (n, key)


def test_two_keys_give_different_permutations():
    a = batching.perm_index_np(7, 1000, np.arange(1000))
    b = batching.perm_index_np(8, 1000, np.arange(1000))
    assert not np.array_equal(a, b) and int((a == b).sum()) < 20                # expected matches of two random permutations: 1
    assert not np.array_equal(a, np.arange(1000))


def test_perm_is_uniform_over_keys():
    """The image of 0 under 4096 consecutive keys at n = 37: every value's count within 5 binomial standard deviations of
    4096 / 37 = 110.7 (sd = sqrt(4096 * (1/37) * (36/37)) = 10.38), i.e. within [58, 163]."""
    counts = np.zeros(37, int)
    for key in range(4096):
        counts[int(batching.perm_index_np(key, 37, np.array([0]))[0])] += 1
    print(counts.min(), counts.max())
    assert counts.min() >= 58 and counts.max() <= 163, counts


def test_perm_refusals():
    with pytest.raises(ValueError):
        batching.perm_index_np(0, 0, [0])
    with pytest.raises(ValueError):
        batching.perm_index_np(0, 2 ** 40, [0])
    with pytest.raises(ValueError):
        batching.perm_index_np(0, 5, [5])
    assert batching.perm_half_bits(1) == 1 and batching.perm_half_bits(4) == 1 and batching.perm_half_bits(5) == 2
    assert batching.perm_half_bits(2 ** 16) == 8 and batching.perm_half_bits(2 ** 16 + 1) == 9


def test_keys_differ_by_seed_step_and_stream():
    keys = {batching.batch_key(s, c, st) for s in (0, 1) for c in range(50) for st in (0, 1)}
    assert len(keys) == 200 and all(0 <= k < 2 ** 64 for k in keys)


def test_schedules_at_reference_defaults():
    # lr: lrate 5e-4, lrate_decay 250 (nerf/utils.py) / 500 (configs/lego.txt)
    for decay in (250, 500):
        for g in (0, 1, 999, 250000):
            assert batching.lr_at(5e-4, decay, g) == 5e-4 * (0.1 ** (g / (decay * 1000)))
    assert batching.lr_at(5e-4, 250, 250000) == pytest.approx(5e-5)
    # precrop: precrop_frac .5 at 800 x 800 and 400 x 400 (configs/lego.txt), an odd size
    assert batching.precrop_window(800, 800, 0.5) == (200, 200) and batching.precrop_crop(800, 800, 0.5) == (200, 200, 400, 400)
    assert batching.precrop_window(400, 400, 0.5) == (100, 100)
    assert batching.precrop_window(37, 53, 0.5) == (int(37 // 2 * 0.5), int(53 // 2 * 0.5)) == (9, 13)
    assert batching.precrop_crop(37, 53, 0.5) == (9, 13, 18, 26)
    # time curriculum: precrop_iters_time 100000 over 50 training frames (run_dnerf.py:650-655)
    for i in (1, 5999, 6000, 50000, 99999):
        assert batching.time_curriculum_max(i, 100000, 50) == max(int(i / float(100000) * 50), 3)
    assert batching.time_curriculum_max(1, 100000, 50) == 3 and batching.time_curriculum_max(50000, 100000, 50) == 25
    assert batching.time_curriculum_max(100000, 100000, 50) is None and batching.time_curriculum_max(1, 0, 50) is None


def test_global_batch_cursor():
    c = batching.EpochCursor(3 * 5 * 7)
    got = [c.next(32) for _ in range(8)]
    assert [n for _, _, n in got] == [32, 32, 32, 9, 32, 32, 32, 9]
    assert [k0 for _, k0, _ in got] == [0, 32, 64, 96] * 2
    assert [e for e, _, _ in got] == [0] * 4 + [1] * 4
    c = batching.EpochCursor(64)                                                # an exact multiple: no empty batch
    assert [c.next(32) for _ in range(3)] == [(0, 0, 32), (0, 32, 32), (1, 0, 32)]


def _train_batch_args(**over):
    one = 1 << 12                                                               # never dereferenced: rejected first
    a = dict(images=one, u8=0, ch=3, n_images=3, H=37, W=53, c2w=one, times=one, i_train=one, n_train=3, y0=0, x0=0, h=37, w=53,
             fx=50., fy=50., cx=26.5, cy=18.5, fb=0, near=2., far=6., cols=11, ndc=0, ndc_focal=50., white=0, key=1, k0=0, n=256,
             ids_in=None, rb=one, target=one, ids_out=None, stream=None)
    a.update(over)
    return list(a.values())


def test_c_entry_points_validate_before_any_device_call():
    L = _lib.lib()
    err = lambda: L.swnerf_last_error().decode()
    one = 1 << 12
    assert L.swnerf_perm_indices(1, 0, 0, 1, one, None) == -1 and "perm_indices" in err()
    assert L.swnerf_perm_indices(1, 1 << 40, 0, 1, one, None) == -1 and "perm_indices" in err()
    assert L.swnerf_perm_indices(1, 10, 5, 6, one, None) == -1 and "perm_indices" in err()
    assert L.swnerf_perm_indices(1, 10, -1, 2, one, None) == -1
    assert L.swnerf_perm_indices(1, 10, 0, -1, one, None) == -1
    assert L.swnerf_perm_indices(1, 10, 0, 4, None, None) == -1 and "NULL" in err()
    assert L.swnerf_perm_indices(1, 10, 3, 0, None, None) == 0
    tb = lambda **o: L.swnerf_train_batch(*_train_batch_args(**o))
    for bad in (dict(images=None), dict(c2w=None), dict(i_train=None)):
        assert tb(**bad) == -1 and "train_batch" in err() and "NULL" in err(), bad
    assert tb(cols=12, times=None) == -1 and "train_batch" in err() and "times" in err()
    assert tb(rb=None) == -1 and "NULL" in err()
    assert tb(target=None) == -1 and "NULL" in err()
    for bad in (dict(h=0), dict(w=0), dict(y0=-1), dict(y0=1), dict(x0=1), dict(h=38), dict(w=54)):
        assert tb(**bad) == -1 and "train_batch" in err() and "window" in err(), bad
    assert tb(k0=3 * 37 * 53 - 255) == -1 and "train_batch" in err() and "domain" in err()
    assert tb(n_train=1, n=37 * 53 + 1) == -1 and "domain" in err()
    assert tb(n=-1) == -1 and tb(k0=-1) == -1
    assert tb(cols=9) == -1 and "columns" in err()
    assert tb(ch=2) == -1 and "channels" in err()
    assert tb(n_images=0) == -1 and tb(n_train=0) == -1 and tb(H=0, h=0) == -1
    assert tb(n_train=1 << 30, H=1 << 10, W=1 << 10, h=1 << 10, w=1 << 10) == -1 and "2^40" in err()
    assert tb(n=0) == 0
    pl = L.swnerf_photo_loss
    assert pl(None, one, one, 4, one, one, one, one, None) == -1 and "photo_loss" in err() and "NULL" in err()
    assert pl(one, one, None, 4, one, one, one, one, None) == -1 and "NULL" in err()
    assert pl(one, one, one, 4, None, one, one, one, None) == -1 and "NULL" in err()
    assert pl(one, one, one, 0, one, one, one, one, None) == -1 and "photo_loss" in err()
    assert pl(one, None, one, 4, one, one, one, one, None) == -1 and "d_rgb0" in err()


def test_python_refusals_without_a_gpu():
    import torch
    with pytest.raises(RuntimeError, match="GPU"):
        batching.RayBatcher(np.zeros((1, 4, 4, 3), np.float32), np.zeros((1, 3, 4), np.float32), [4, 4, 5.0], [0], 2., 6., device="cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        batching.photometric_loss(torch.zeros(4, 3), torch.zeros(4, 3))


def test_train_signatures():
    for fn in (runner.train, runner.train_dnerf):
        p = inspect.signature(fn).parameters
        assert list(p) == ["args", "data", "device", "sampler", "loss_fn", "hooks"]
        assert p["device"].default is None and p["sampler"].default == "device" and p["loss_fn"].default is None and p["hooks"].default is None
    p = inspect.signature(batching.RayBatcher.__init__).parameters
    assert list(p)[1:12] == ["images", "poses", "hwf_or_K", "i_train", "near", "far", "times", "ndc", "use_viewdirs", "white_bkgd", "seed"]
    assert (p["times"].default, p["ndc"].default, p["use_viewdirs"].default, p["white_bkgd"].default, p["seed"].default) == (None, False, True, False, 0)
    assert list(inspect.signature(batching.RayBatcher.image_batch).parameters)[1:6] == ["img_i", "n_rand", "step", "crop", "ids"]
    assert list(inspect.signature(batching.photometric_loss).parameters) == ["rgb", "target", "rgb0"]
