"""Host-side checks of the fused T-NeRF training pass (no GPU): the un-fold algebra of `feature` folded into `layer_9`, the
padded-row rule and the size queries, train_tnerf's refusals, the time curriculum, and the argument checks of the new C entry
points (every case is refused before any device call)."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "sw-nerf_amd"), os.path.join(HERE, "golden"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import tnerf_train_ref as TR   # noqa: E402

E_ARG, E_UNSUPP = -1, -2


def test_unfold_algebra_is_exact():
    """pre_9 = W9f (Wf h7 + bf) + W9d gd + b9 run as ONE layer W' h7 + ... : from G = sum d pre_9 (x) h7 and db' = sum d pre_9 the
    three gradients of the two-layer form follow exactly (float64, against autograd)."""
    g = torch.Generator().manual_seed(1)
    M = 50
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    h7, gd = r(M, 128), r(M, 27)
    Wf, bf, W9, b9 = r(128, 128).requires_grad_(), r(128).requires_grad_(), r(64, 155).requires_grad_(), r(64).requires_grad_()
    pre9 = torch.nn.functional.linear(torch.cat([torch.nn.functional.linear(h7, Wf, bf), gd], -1), W9, b9)
    up = r(M, 64)                                            # d loss / d pre_9
    (pre9 * up).sum().backward()
    G, dbp = (up.T @ h7).numpy(), up.sum(0).numpy()
    dW9f, dWf, dbf = TR.unfold(G, dbp, W9.detach().numpy()[:, :128], Wf.detach().numpy(), bf.detach().numpy())
    scale = lambda t: float(t.abs().max())
    assert np.abs(dW9f - W9.grad.numpy()[:, :128]).max() <= 1e-12 * scale(W9.grad)
    assert np.abs(dWf - Wf.grad.numpy()).max() <= 1e-12 * scale(Wf.grad)
    assert np.abs(dbf - bf.grad.numpy()).max() <= 1e-12 * scale(bf.grad)
    # the gamma(d) columns and the bias of layer_9 are the folded layer's own
    assert np.abs((up.T @ gd).numpy() - W9.grad.numpy()[:, 128:]).max() <= 1e-12 * scale(W9.grad)
    assert np.abs(dbp - b9.grad.numpy()).max() <= 1e-12 * scale(b9.grad)


@pytest.fixture(scope="module")
def L():
    from swnerf import _lib
    return _lib.lib()


def test_padded_rows_and_size_queries(L):
    for n, S in ((1, 2), (5, 31), (5, 32), (5, 33), (7, 65), (4096, 64), (3, 256)):
        assert L.swnerf_train_rows(n, S) == n * ((S + 31) // 32) * 32
    assert L.swnerf_tnerf_act_floats_per_row() == 8 * 128 + 64 == 1088
    assert L.swnerf_tnerf_xs_floats_per_row() == 64 + 32 + 32 == 128
    steps = 32 + 7 * 64                                      # W9f^T (4 x 2) | layers.7..1 transposed (4 x 4)
    assert L.swnerf_packed_bwd_tnerf_floats() == (steps + 16) * 256 + 10 * 32 + 64 * 160 + 64


def _err(L):
    return L.swnerf_last_error().decode()


def test_c_abi_argument_checks_without_gpu(L):
    from swnerf import _lib
    fake = ctypes.c_void_p(16)                              # never dereferenced: every case fails before any device call

    def args(**kw):
        a = _lib.PassArgs()
        a.ray_batch, a.n_rays, a.cols, a.kind, a.packed = fake.value, 4, 12, _lib.NET_TNERF, fake.value
        a.L_pos, a.L_dir, a.L_time, a.n_samples = 10, 4, 10, 64
        a.raw, a.z_out = fake.value, fake.value
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    tr = L.swnerf_render_pass_train_tnerf
    assert tr(None, fake, fake, None) == E_ARG and "NULL args" in _err(L)
    assert tr(args(), None, fake, None) == E_ARG and "NULL pointer" in _err(L)
    assert tr(args(), fake, None, None) == E_ARG and "NULL pointer" in _err(L)
    for kw, code, msg in ((dict(packed=0), E_ARG, "NULL pointer"), (dict(kind=0, cols=11), E_UNSUPP, "T-NeRF (SWNERF_NET_TNERF)"),
                          (dict(cols=11), E_UNSUPP, "12-column"), (dict(n_samples=1), E_UNSUPP, "2 <= n_samples <= 256 (got 1)"),
                          (dict(n_samples=257), E_UNSUPP, "2 <= n_samples <= 256 (got 257)"), (dict(n_rays=-1), E_UNSUPP, "2 <= n_samples"),
                          (dict(L_time=11), E_UNSUPP, "exceed (10,4,10)"), (dict(L_dir=0), E_UNSUPP, "needs view directions"),
                          (dict(n_importance=8), E_ARG, "no hierarchical resampling"), (dict(dx=16), E_ARG, "no position_delta"),
                          (dict(raw=0), E_ARG, "the backward needs raw and the depths"), (dict(z_out=0), E_ARG, "the backward needs raw and the depths"),
                          (dict(raw=20), E_ARG, "16-byte aligned"), (dict(z_vals=16, t_rand=16), E_ARG, "t_rand only applies")):
        assert tr(args(**kw), fake, fake, None) == code and msg in _err(L), (kw, _err(L))
        assert _err(L).startswith("render_pass_train_tnerf: ")
    assert tr(args(n_rays=0, ray_batch=0), None, None, None) == 0          # an empty batch: nothing to do

    bw = L.swnerf_render_pass_backward_tnerf
    ok = [fake, fake, fake, fake, fake, 12, None, 4, 64, 1, None, None, None, None, fake, fake, None]

    def bwd(**ch):
        a = list(ok)
        for k, v in ch.items():
            a[int(k[1:])] = v
        return bw(*a)
    for ch, code, msg in ((dict(a0=None), E_ARG, "NULL pointer"), (dict(a1=None), E_ARG, "NULL pointer"), (dict(a14=None), E_ARG, "NULL pointer"),
                          (dict(a15=None), E_ARG, "NULL pointer"), (dict(a7=-1), E_ARG, "negative n_rays"), (dict(a8=1), E_UNSUPP, "(got 1)"),
                          (dict(a8=257), E_UNSUPP, "(got 257)"), (dict(a5=11), E_ARG, "12-column"),
                          (dict(a1=ctypes.c_void_p(20)), E_ARG, "16-byte aligned"), (dict(a13=ctypes.c_void_p(24)), E_ARG, "16-byte aligned")):
        assert bwd(**ch) == code and msg in _err(L), (ch, _err(L))
        assert _err(L).startswith("render_pass_backward_tnerf: ")
    assert bwd(a7=0) == 0

    arr = (ctypes.c_void_p * 24)(*([fake.value] * 24))
    pk = L.swnerf_pack_net_bwd_tnerf
    assert pk(None, 10, 4, 10, fake, None) == E_ARG and pk(arr, 10, 4, 10, None, None) == E_ARG and "NULL pointer" in _err(L)
    assert pk(arr, 10, 0, 10, fake, None) == E_UNSUPP and pk(arr, 11, 4, 10, fake, None) == E_UNSUPP and "outside" in _err(L)
    arr[7] = None
    assert pk(arr, 10, 4, 10, fake, None) == E_ARG and "params[7]" in _err(L)

    ff = L.swnerf_tnerf_feature_finish
    good = [fake, fake, fake, 155, fake, fake, fake, fake, fake, 155, fake, fake, fake, fake, None]
    for k in (0, 1, 2, 4, 5, 6, 7, 8, 10, 11, 12, 13):
        a = list(good)
        a[k] = None
        assert ff(*a) == E_ARG and "tnerf_feature_finish" in _err(L), k
    for k in (3, 9):
        a = list(good)
        a[k] = 127
        assert ff(*a) == E_ARG and "leading dimension below 128" in _err(L), k


def test_time_curriculum_draw_is_the_reference_lines():
    """run_tnerf.py:646-651: i >= precrop_iters_time draws from all of i_train, else from i_train[:max(int(i / p * n), 3)]."""
    from swnerf.batching import time_curriculum_max
    i_train = np.arange(40)
    for p in (0, 7, 100):
        for i in range(1, 120, 3):
            np.random.seed(i)
            if i >= p:
                want = np.random.choice(i_train)
            else:
                skip_factor = i / float(p) * len(i_train)
                max_sample = max(int(skip_factor), 3)
                want = np.random.choice(i_train[:max_sample])
            np.random.seed(i)
            m = time_curriculum_max(i, p, len(i_train))
            assert np.random.choice(i_train if m is None else i_train[:m]) == want


def test_train_tnerf_argument_refusals(tmp_path):
    from swnerf import runner
    a = types.SimpleNamespace(no_batching=False, N_rand=64, basedir=str(tmp_path), expname="x")
    H = W = 8
    data = (np.zeros((3, H, W, 3), np.float32), np.zeros((3, 4, 4), np.float32), None, [H, W, 10.0], [[0, 1, 2], [], []],
            np.array([0., .5, 1.], np.float32), 2., 6.)
    with pytest.raises(NotImplementedError, match="no frame time"):
        runner.train_tnerf(a, data, device="cpu")
    with pytest.raises(ValueError, match="frame times"):                   # the 7-entry tuple of the static runner
        runner.train_tnerf(a, data[:5] + data[6:], device="cpu")
    a.no_batching = True
    with pytest.raises(ValueError, match="sampler"):
        runner.train_tnerf(a, data, device="cpu", sampler="host")
    import inspect
    assert list(inspect.signature(runner.train_tnerf).parameters) == ["args", "data", "device", "sampler", "loss_fn", "hooks"]
