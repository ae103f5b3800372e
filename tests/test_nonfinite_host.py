"""The non-finite cases of tests/test_gpu_nonfinite.py (tests/density_regimes.py: POISONS, poison_*), checked where no kernel
runs: the float32 and the float64 evaluation of the CPU oracle agree on the non-finite pattern of every output and every
gradient of every case.  The GPU tests compare float32 kernels with the float64 oracle and demand an equal pattern; without
this module a difference there could be the reference's own (an overflow float32 has and float64 has not).  Also: every case
keeps at least half of its rays clean, the poisoned samples sit on the tile and sweep boundaries, and torch.sort - the
reference of the merge - holds NaN behind everything.  Runs without a GPU."""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from density_regimes import (T, NAMES, POISONS, POISON_S, POISON_PDF, POISON_NB, POISON_UPS, comp_loss, same_nonfinite,
                             poison_positions, poison_comp_inputs, poison_pdf_inputs, poison_fused_noise)

N = 41
B_SIGMA = 0.25                         # tests/test_gpu_fused_tail.py: the constant density of the fused tests' nets


def oracle_comp(raw, z, d, noise, white, ups, dtype):
    """-> (the five outputs, {upstream: d raw}) of the oracle evaluated in `dtype`"""
    conv = lambda a: T(a).to(dtype)
    r = conv(raw).requires_grad_(True)
    outs = O.raw2outputs(r, conv(z), conv(d), 0., white, noise=conv(noise))
    grads = {which: torch.autograd.grad(comp_loss(outs, ups, which, conv), r, retain_graph=True)[0] for which in POISON_UPS}
    return [o.detach() for o in outs], grads


def check_positions(S, rays, j, n):
    assert 2 * len(rays) <= n and len(set(rays.tolist())) == len(rays), "fewer than half of the rays are clean"
    must = {k for k in (0, S - 1, 31, 32, 63, 64) if 0 <= k < S}
    assert must <= set(j.tolist()), (S, sorted(must - set(j.tolist())))
    assert ((0 <= j) & (j < S)).all()


@pytest.mark.parametrize("where", ["density", "colour"])
@pytest.mark.parametrize("kind", list(POISONS))
@pytest.mark.parametrize("S", POISON_S)
def test_compositing_cases_have_one_pattern_in_float32_and_float64(S, kind, where):
    raw, z, d, noise, ups, rays, j = poison_comp_inputs(S, kind, where, N=N)
    check_positions(S, rays, j, N)
    hit = (noise if where == "density" else raw[..., :3])
    assert (~np.isfinite(hit)).sum() == len(rays) and (~np.isfinite(hit)).any(-1).reshape(N, -1).any(-1).sum() == len(rays)
    clean = np.setdiff1d(np.arange(N), rays)
    for white in (False, True):
        o32, g32 = oracle_comp(raw, z, d, noise, white, ups, torch.float32)
        o64, g64 = oracle_comp(raw, z, d, noise, white, ups, torch.float64)
        for name, a, b in zip(NAMES, o32, o64):
            assert same_nonfinite(a, b), f"S={S} {kind} {where} white={white}: {name}"
            assert bool(torch.isfinite(b[clean] if name != "disp" else torch.nan_to_num(b[clean])).all()), name
        for which in POISON_UPS:
            assert same_nonfinite(g32[which], g64[which]), f"S={S} {kind} {where} white={white}: d raw from {which}"
            assert bool(torch.isfinite(g64[which][clean]).all())
        if kind == "nan" and where == "density":                # the rule the kernels are held to: NaN from that sample on
            w = o64[3].numpy()
            for r, k in zip(rays, j):
                assert np.isnan(w[r, k:]).all() and np.isfinite(w[r, :k]).all(), (r, k)
            assert all(bool(torch.isnan(o64[i][rays]).all()) for i in (0, 1, 2, 4))


@pytest.mark.parametrize("kind", list(POISONS))
@pytest.mark.parametrize("S", (33, 65))
def test_fused_noise_cases_have_one_pattern_in_float32_and_float64(S, kind):
    """the fused tests feed the oracle the pass's own raw: here random colours stand for it - the pattern is the density's"""
    noise, z, rays, j = poison_fused_noise(S, kind, B_SIGMA, N=N)
    check_positions(S, rays, j, N)
    rng = np.random.default_rng(S)
    raw = (rng.standard_normal((N, S, 4)) * 1.5).astype(np.float32)
    raw[..., 3] = B_SIGMA
    d = rng.standard_normal((N, 3)).astype(np.float32)
    for white in (False, True):
        o32 = O.raw2outputs(T(raw), T(z), T(d), 0., white, noise=T(noise))
        o64 = O.raw2outputs(T(raw).double(), T(z).double(), T(d).double(), 0., white, noise=T(noise).double())
        for name, a, b in zip(NAMES, o32, o64):
            assert same_nonfinite(a, b), f"S={S} {kind} white={white}: {name}"


@pytest.mark.parametrize("mode", ["det", "random"])
@pytest.mark.parametrize("kind", list(POISONS))
@pytest.mark.parametrize("S,Ni", POISON_PDF)
def test_weight_poison_makes_every_sample_nan_and_sort_holds_nan_last(S, Ni, kind, mode):
    bins, w, u, z, rays, j = poison_pdf_inputs(S, Ni, kind, mode, N=N)
    check_positions(POISON_NB - 1, rays, j, N)
    clean = np.setdiff1d(np.arange(N), rays)
    u64 = torch.linspace(0., 1., Ni).expand(N, Ni) if u is None else T(u)
    s32 = O.sample_pdf(T(bins), T(w), Ni, u=u64.contiguous())
    s64 = O.sample_pdf(T(bins).double(), T(w).double(), Ni, u=u64.double().contiguous())
    assert same_nonfinite(s32, s64)
    assert bool(torch.isnan(s64[rays]).all()) and bool(torch.isfinite(s64[clean]).all())
    zs = torch.sort(torch.cat([T(z), s32], -1), -1)[0]
    assert bool(torch.isnan(zs[rays][:, S:]).all()) and torch.equal(zs[rays][:, :S], T(z)[rays])


@pytest.mark.parametrize("S,Ni", [p for p in POISON_PDF if p[1] > 1])
def test_one_nan_draw_gives_one_nan_sample_held_last(S, Ni):
    bins, w, u, z, rays, j = poison_pdf_inputs(S, Ni, "nan", "random", target="u", N=N)
    check_positions(Ni, rays, j, N)
    s32 = O.sample_pdf(T(bins), T(w), Ni, u=T(u))
    s64 = O.sample_pdf(T(bins).double(), T(w).double(), Ni, u=T(u).double())
    want = np.zeros((N, Ni), bool)
    want[rays, j] = True
    assert np.array_equal(np.isnan(s32.numpy()), want) and np.array_equal(np.isnan(s64.numpy()), want)
    zs = torch.sort(torch.cat([T(z), s32], -1), -1)[0]
    assert np.array_equal(np.isnan(zs.numpy()).sum(-1), want.sum(-1)) and bool(torch.isnan(zs[rays][:, -1]).all())
    assert bool((zs[:, 1:S + Ni - 1] >= zs[:, :S + Ni - 2]).all())


def test_poison_positions_small_batches():
    """N = 13 (the backward tests): six poisoned rays see every boundary of S = 65; a prefix of 3 or 5 rays holds both kinds"""
    rays, j = poison_positions(65, 13, np.random.default_rng(0))
    check_positions(65, rays, j, 13)
    for n in (3, 5):
        assert (rays < n).any() and (rays < n).sum() < n
