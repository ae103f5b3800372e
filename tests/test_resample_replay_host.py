"""tests/resample_replay.py pinned to the REFERENCE (the CPU oracle's sample_pdf, ray.py:96-153), not to the kernel: the GPU
tests then hold csrc/resample.h to the replay bit for bit, and this module is why that means something.  Runs without a GPU.

Inputs are those of tests/test_gpu_op_domain.py::pdf_inputs - every bin carries mass, random u plus u on cdf values - so the
replay's float32 arithmetic stays within the project's figure for the op (5e-5) of float64.  In float32 the oracle differs from the
replay in ONE place, the cdf: ATen sums the normaliser in float32 in a machine-dependent blocking, the replay (like the kernel)
in float64 rounded once.  Wherever the two cdfs have the same bits, the samples must too."""
import numpy as np
import pytest
import torch

import resample_replay as RR
from oracle import nerf_oracle as O

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
SHAPES = [(2, 1), (3, 5), (5, 64), (17, 33), (33, 95), (64, 128), (65, 37), (255, 64), (256, 768)]       # (bins, samples)
N = 64


def pdf_inputs(nb, ns, seed):
    rng = np.random.default_rng(seed)
    bins = np.sort(rng.uniform(2, 6, (N, nb)).astype(np.float32), -1)
    w = rng.uniform(0.5, 1.5, (N, nb - 1)).astype(np.float32)
    u = rng.uniform(0, 1, (N, ns)).astype(np.float32)
    cdf, _ = RR.cdf_of(w)
    if ns > 1:
        u[:, 0] = cdf[:, min(1, nb - 1)]                       # ties with an interior / the last cdf value (right=True)
        u[:, -1] = 0.0                                         # draws bins[:, 0] exactly
    if ns > 4:
        u[:, 1] = cdf[:, nb // 2]
        u[:, 2] = np.minimum(cdf[:, -1], np.float32(1.0))
    return bins, w, u


def oracle_cdf32(w):
    """the cdf lines of oracle.nerf_oracle.sample_pdf, in float32"""
    w = T(w) + 1e-5
    cdf = torch.cumsum(w / w.sum(-1, keepdim=True), -1)
    return torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1).numpy()


@pytest.mark.parametrize("nb,ns", SHAPES)
def test_replay_against_the_oracle(nb, ns):
    bins, w, u = pdf_inputs(nb, ns, 1000 * nb + ns)
    rows = same = 0
    worst = 0.0
    for uu in (None, u):
        got = RR.sample_pdf(bins, w, ns, uu)
        assert got.dtype == np.float32 and got.shape == (N, ns)
        u64 = torch.linspace(0., 1., ns).expand(N, ns).double().contiguous() if uu is None else T(uu).double()
        ref64 = O.sample_pdf(T(bins).double(), T(w).double(), ns, det=False, u=u64).numpy()
        err = float(np.abs(got.astype(np.float64) - ref64).max())
        worst = max(worst, err)
        u32 = torch.linspace(0., 1., ns).expand(N, ns).contiguous() if uu is None else T(uu)
        ref32 = O.sample_pdf(T(bins), T(w), ns, det=False, u=u32).numpy()
        q = (oracle_cdf32(w).view(np.int32) == RR.cdf_of(w)[0].view(np.int32)).all(-1)
        rows, same = rows + N, same + int(q.sum())
        assert np.array_equal(got[q].view(np.int32), ref32[q].view(np.int32)), \
            f"nb={nb} ns={ns} det={uu is None}: same float32 cdf as the oracle, other samples"
        if uu is not None and ns > 1:
            assert np.array_equal(got[:, -1], bins[:, 0])
    print(f"\n[replay] sample_pdf nb={nb} ns={ns}: max |replay - float64 oracle| {worst:.2e}; {same} of {rows} rows share the oracle's float32 cdf")
    assert worst <= 5e-5
    assert 2 * same >= rows, f"only {same} of {rows} rows have the oracle's float32 cdf: the bit comparison covers too little"


def test_replay_merge_and_std_against_torch():
    """z_fine = torch.sort(cat) values; z_std = torch.std(unbiased=False) of the float64 samples, rounded once"""
    bins, w, u = pdf_inputs(65, 128, 7)
    z = np.sort(np.random.default_rng(8).uniform(2, 6, (N, 66)).astype(np.float32), -1)
    z[:, 3] = z[:, 2]                                          # a tie inside the coarse list
    s, zf, sd = RR.resample(z, np.concatenate([w[:, :1], w, w[:, :1]], -1), 128, u)
    assert np.array_equal(s.view(np.int32), RR.sample_pdf(RR.mid_bins(z), w, 128, u).view(np.int32))
    assert torch.equal(T(zf), torch.sort(torch.cat([T(z), T(s)], -1), -1)[0])
    assert np.array_equal(sd, torch.std(T(s).double(), -1, unbiased=False).float().numpy())
    assert np.array_equal(RR.mid_bins(z), (.5 * (T(z)[:, 1:] + T(z)[:, :-1])).numpy())


def test_low_mass_bins_take_the_den_rule():
    """What pdf_inputs never produces: bins that carry (almost) no mass.  The replay must enter den < 1e-5 -> 1 there, stay inside
    [bins[0], bins[-1]] and ascend for ascending u; an all-zero weight row gives the uniform pdf."""
    rng = np.random.default_rng(3)
    nb, ns = 65, 128
    bins = np.sort(rng.uniform(2, 6, (N, nb)).astype(np.float32), -1)
    w = np.zeros((N, nb - 1), np.float32)
    w[np.arange(N // 2), rng.integers(0, nb - 1, N // 2)] = 1.0                      # a single spike; the other half all zero
    cdf, _ = RR.cdf_of(w)
    den = np.diff(cdf, axis=-1)
    # an empty bin's pdf is 1e-5 / 1.00064: its float32 cdf step lands on either side of the threshold, ray by ray and bin by bin
    low = den[:N // 2] < 1e-5
    assert low.sum() >= (N // 2) * 8 and (~low).sum() >= (N // 2) * 8, "the spike rays do not straddle den = 1e-5"
    s = RR.sample_pdf(bins, w, ns)
    assert (s >= bins[:, :1]).all() and (s <= bins[:, -1:]).all() and (np.diff(s, axis=-1) >= 0).all()
    uniform = RR.sample_pdf(bins, np.full_like(w, 0.25), ns)
    assert np.array_equal(s[N // 2:].view(np.int32), uniform[N // 2:].view(np.int32))
    # the rule itself: with it switched off, a u inside a massless bin divides by that bin's tiny cdf step instead of by 1
    r = 0
    j = int(np.argmax(w[r]))
    k = int(np.nonzero(low[r] & (np.arange(nb - 1) != j))[0][0])
    u = np.array([[0.5 * (float(cdf[r, k]) + float(cdf[r, k + 1]))]], np.float32)
    got = RR.draw(bins[r:r + 1], cdf[r:r + 1], u)
    lo = np.searchsorted(cdf[r], u[0, 0], side="right")
    b, a = max(lo - 1, 0), min(lo, nb - 1)
    assert cdf[r, a] - cdf[r, b] < 1e-5
    assert got[0, 0] == np.float32(bins[r, b] + np.float32(np.float32(u[0, 0] - cdf[r, b]) * np.float32(bins[r, a] - bins[r, b])))
