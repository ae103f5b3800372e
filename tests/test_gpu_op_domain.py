"""The standalone ops over every shape and range their C-ABI entry points accept (include/swnerf.h, csrc/misc_kernels.hip,
csrc/backward_kernels.hip): embed, raw2outputs and its backward, sample_pdf (+ merge, + std), sample_coarse.

The domain edges are where the kernels change code path: embed halves its rows per workgroup for rows wider than 256 floats and
leaves the float4 store when a block's image is not a multiple of 4 floats; raw2outputs and its backward carry a transmittance
and a suffix sum from one 64-sample sweep to the next; sample_pdf sorts with a bitonic network padded to a power of two and merges
by rank.  Every reference is a vectorised float64 evaluation (numpy / the CPU oracle on float64 tensors) of the same float32
inputs; every element of every case is held to the tolerance - no "mostly" clause.  Finite inputs only: NaN and Inf are
tests/test_gpu_nonfinite.py.

Tolerances are the project's existing ones for these ops (tests/test_gpu_parity.py, tests/test_gpu_backward.py):
  embed 3e-7 abs; raw2outputs atol 2e-6 + rtol 2e-5; its backward atol 2e-6 + rtol 2e-4; sample_pdf atol 5e-5;
  sample_coarse bit-equal without jitter, atol 1e-6 with.  z_std rtol 1e-6 against the kernel's own samples (the kernel sums
  in double and rounds once: 6e-8)."""
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from density_regimes import (T, _np, close, bits, Guarded, REGIMES, UPSTREAM, NAMES,             # the five regimes the ops were always held to
                             comp_inputs, comp_loss, comp_reference)

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sw():
    import swnerf.ray, swnerf.embedder, swnerf.render  # noqa
    import swnerf
    return swnerf


@pytest.fixture(scope="module")
def L_():
    from swnerf import _lib
    return _lib


# ------------------------------------------------------------------------------------------------------------ a. embed
def embed_specials():
    v = [0.0, -0.0, 1e-30, -1e-30, 6.0, -6.0]
    for k in (0, 9, 17, 23):                         # pi/2 * m * 2^-k: on a quadrant boundary once scaled by 2^k
        for m in (1, 2, 3, 5, 7):
            q = float(np.float32(np.pi / 2 * m)) * 2.0 ** -k
            if abs(q) <= 6.0:
                v += [q, -q]
    return np.array(v, np.float32)


def embed_inputs(M, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-6, 6, (M, d)).astype(np.float32)
    sp = embed_specials()
    n = min(sp.size, x.size)
    x.reshape(-1)[:n] = sp[:n]
    return x


def embed_truth(x, L):
    """embedder.py:33-42: [x, sin(2^0 x), cos(2^0 x), ..., sin(2^(L-1) x), cos(2^(L-1) x)], blocks d wide; float64 sin / cos of the
    float32 product (exact in float64 and in float32: a power-of-two scaling)"""
    xd = x.astype(np.float64)
    M, d = x.shape
    y = xd[:, None, :] * (2.0 ** np.arange(L))[None, :, None]                     # [M, L, d]
    assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
    sc = np.stack([np.sin(y), np.cos(y)], 2).reshape(M, 2 * L * d)
    return np.concatenate([xd, sc], 1)


def check_embed(got, x, L, what):
    """-> per-band max |err| ([L]); x columns bit-equal, every sin / cos within 3e-7"""
    M, d = x.shape
    got = _np(got)
    assert got.shape == (M, d * (1 + 2 * L)), (what, got.shape)
    assert np.array_equal(got[:, :d].view(np.int32), x.view(np.int32)), f"{what}: copied x columns differ"
    if L == 0:
        return np.zeros(0)
    err = np.abs(got[:, d:].astype(np.float64) - embed_truth(x, L)[:, d:]).reshape(M, L, 2 * d)
    band = err.max((0, 2))
    assert np.isfinite(got).all() and float(band.max()) <= 3e-7, f"{what}: per-band max |err| {np.array2string(band, precision=2)}"
    return band


@pytest.mark.parametrize("d", range(1, 17))
def test_embed_every_accepted_pair(sw, dev, d):
    """all (d, L) with 1 <= d <= 16, 0 <= L <= 24 at M = 67 (a partial block; an odd image for odd C)"""
    worst = np.zeros(24)
    for L in range(0, 25):
        x = embed_inputs(67, d, 100 * d + L)
        fn, width = sw.embedder.get_embedder(L, d, 0)
        assert width == d * (1 + 2 * L)
        band = check_embed(fn(T(x).to(dev)), x, L, f"embed d={d} L={L}")
        worst[:L] = np.maximum(worst[:L], band)
    print(f"\n[op-domain] embed d={d}: per-band max |err| " + " ".join(f"{e:.2e}" for e in worst))


@pytest.mark.parametrize("d,L", [(3, 10), (3, 4), (1, 10), (3, 16), (16, 24), (5, 7)])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 1023, 4097])
def test_embed_row_counts(sw, dev, d, L, M):
    """whole and partial last blocks, the dword-store fall-back, the halved rows per workgroup (C = 784), leading batch dims"""
    x = embed_inputs(M, d, 7 * M + d + L)
    fn, _ = sw.embedder.get_embedder(L, d, 0)
    got = fn(T(x).to(dev))
    check_embed(got, x, L, f"embed d={d} L={L} M={M}")
    lead = {1: (1, 1, 1), 63: (7, 9), 64: (4, 16), 65: (5, 13), 1023: (3, 341), 4097: (17, 241)}[M]
    got_b = fn(T(x).to(dev).reshape(*lead, d))
    assert got_b.shape == (*lead, d * (1 + 2 * L)) and torch.equal(got_b.reshape(M, -1), got)


def test_embed_beyond_the_domain_is_refused(sw, dev, L_):
    x = torch.zeros((4, 3), device=dev)
    g = Guarded((4, 3 * 51), dev)
    for d, L in ((3, 25), (17, 4), (0, 4), (3, -1)):
        rc = L_.lib().swnerf_embed(L_.ptr(x), 4, d, L, L_.ptr(g.out), L_.stream_of(x))
        assert rc != 0, (d, L)
    assert g.untouched()
    with pytest.raises(NotImplementedError):
        sw.embedder.get_embedder(25, 3, 0)


# ------------------------------------------------------------------------------------ b. device sin/cos = the host build
HOST_SINCOS = r'''
#include "swnerf_common.h"
#include <stdio.h>
#include <stdlib.h>
int main(int argc, char** argv) {          /* in: n floats x; out: for each x, for k < L: sin, cos of x * 2^k as embed_kernel does */
  FILE* fi = fopen(argv[1], "rb"); FILE* fo = fopen(argv[2], "wb"); long n = atol(argv[3]); int L = atoi(argv[4]);
  if (!fi || !fo) return 2;
  float* x = (float*)malloc(n * sizeof(float)); float* o = (float*)malloc((size_t)n * L * 2 * sizeof(float));
  if (fread(x, sizeof(float), n, fi) != (size_t)n) return 3;
  for (long i = 0; i < n; ++i) for (int k = 0; k < L; ++k) sw_sincos_pair(x[i] * (float)(1 << k), &o[(i * L + k) * 2], &o[(i * L + k) * 2 + 1]);
  if (fwrite(o, sizeof(float), (size_t)n * L * 2, fo) != (size_t)n * L * 2) return 4;
  fclose(fo); return 0;
}
'''


def test_device_sincos_equals_host_build(sw, dev, tmp_path):
    """tests/test_host_math.py certifies swnerf_common.h as g++ compiles it; this holds the device build of the same header to it:
    1 M arguments (M x 3 x 10 bands), bit for bit.  Same compile line as test_common_header_on_host."""
    (tmp_path / "h.cpp").write_text(HOST_SINCOS)
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-mfma", "-I", os.path.join(ROOT, "sw-nerf_amd", "csrc"),
                    str(tmp_path / "h.cpp"), "-o", str(tmp_path / "h"), "-lm"], check=True)
    M, d, L = 34953, 3, 10
    x = embed_inputs(M, d, 42)
    x.tofile(tmp_path / "x.bin")
    subprocess.run([str(tmp_path / "h"), str(tmp_path / "x.bin"), str(tmp_path / "o.bin"), str(M * d), str(L)], check=True)
    host = np.fromfile(tmp_path / "o.bin", np.float32).reshape(M, d, L, 2)
    fn, _ = sw.embedder.get_embedder(L, d, 0)
    got = _np(fn(T(x).to(dev)))[:, d:].reshape(M, L, 2, d)
    host = host.transpose(0, 2, 3, 1)                                                  # -> [M, L, (sin, cos), d]
    diff = got.view(np.int32) != host.view(np.int32)
    ulp = np.abs(got.view(np.int32).astype(np.int64) - host.view(np.int32).astype(np.int64))
    print(f"\n[op-domain] device vs host sin/cos: {int(diff.sum())} of {diff.size} differ, max {int(ulp.max())} ulp")
    assert M * d * L >= 1_000_000 and not diff.any()


# ----------------------------------------------------------------------------------------------------- c. compositing
COMP_S_BWD = (2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024)
COMP_S_FWD = COMP_S_BWD + (1025, 2049)
COMP_N = (1, 2, 3, 4, 5, 41)


def check_compositing(impl, regime, S, put, stats=None):
    """impl(raw, z, d, noise=..., white=...) -> the five outputs (differentiable w.r.t. raw when S <= 1024);
    put: numpy -> the implementation's tensor.  Rays are independent, so the N = 41 reference serves every smaller batch."""
    raw, z, d, noise, ups = comp_inputs(regime, S, 1000 * S + REGIMES.index(regime))
    with_grad = S <= 1024
    for white in (False, True):
        for nz in (None, noise):
            ref, ref_g = comp_reference(raw, z, d, nz, white, ups, with_grad)
            for N in COMP_N:
                what = f"raw2outputs {regime} S={S} N={N} white={white} noise={nz is not None}"
                r = put(raw[:N]).requires_grad_(with_grad)
                outs = impl(r, put(z[:N]), put(d[:N]), noise=None if nz is None else put(nz[:N]), white=white)
                for name, o, b in zip(NAMES, outs, ref):
                    e = close(o, b[:N], atol=2e-6, rtol=2e-5, what=f"{what} {name}")
                    if stats is not None:
                        stats["fwd"] = max(stats.get("fwd", 0.0), e)
                if regime == "all_empty":
                    assert bool(torch.isnan(outs[1]).all()) and float(outs[2].detach().abs().max()) == 0.0, what
                if not with_grad:
                    continue
                for which in UPSTREAM:
                    g, = torch.autograd.grad(comp_loss(outs, ups, which, put), r, retain_graph=True)
                    e = close(g, ref_g[which][:N], atol=2e-6, rtol=2e-4, what=f"{what} d raw from d {which}")
                    if stats is not None:
                        stats["bwd"] = max(stats.get("bwd", 0.0), e)
                    if regime == "all_empty":
                        assert float(g[..., 3].abs().max()) == 0.0, what


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("S", COMP_S_FWD)
def test_compositing_against_float64(sw, dev, S, regime):
    stats = {}
    impl = lambda raw, z, d, noise, white: sw.ray.raw2outputs(raw, z, d, 0, white, noise=noise)
    check_compositing(impl, regime, S, lambda a: T(a).to(dev), stats)
    print(f"\n[op-domain] raw2outputs {regime} S={S}: max |err| forward {stats.get('fwd', 0):.2e} backward {stats.get('bwd', 0):.2e}")


def test_compositing_backward_beyond_its_domain_raises(sw, dev):
    """S = 1025 under grad: the backward keeps T and w of a ray in LDS (2 <= S <= 1024) - an error, never a truncated gradient"""
    raw, z, d, _, _ = comp_inputs("mild", 1025, 5, N=3)
    r = T(raw).to(dev).requires_grad_(True)
    with pytest.raises(RuntimeError, match="1024"):
        sw.ray.raw2outputs(r, T(z).to(dev), T(d).to(dev), 0, True)[0].sum().backward()
    assert r.grad is None


def _r2o_abi(L_, raw, z, d, noise, white, outs):
    N, S = z.shape
    L_.check(L_.lib().swnerf_raw2outputs(L_.ptr(raw), L_.ptr(z), L_.ptr(d), L_.ptr(noise), N, S, int(white),
                                         *[L_.ptr(o) for o in outs], L_.stream_of(raw)), "raw2outputs")


def _r2o_shapes(N, S):
    return {"rgb": (N, 3), "disp": (N,), "acc": (N,), "weights": (N, S), "depth": (N,)}


@pytest.mark.parametrize("N,S", [(5, 257), (41, 64), (3, 2049)])
def test_compositing_null_outputs_change_no_bit(dev, L_, N, S):
    """every output pointer of swnerf_raw2outputs may be NULL: the others keep their bits"""
    raw, z, d, noise, _ = comp_inputs("soft_then_wall", S, 11, N=N)
    raw, z, d, noise = (T(a).to(dev) for a in (raw, z, d, noise))
    full = [torch.empty(s, device=dev) for s in _r2o_shapes(N, S).values()]
    _r2o_abi(L_, raw, z, d, noise, True, full)
    for drop in range(-1, 5):                       # -1: every output but rgb NULL
        outs = [torch.empty(s, device=dev) for s in _r2o_shapes(N, S).values()]
        given = [o if (k != drop if drop >= 0 else k == 0) else None for k, o in enumerate(outs)]
        _r2o_abi(L_, raw, z, d, noise, True, given)
        for k, o in enumerate(given):
            if o is not None:
                assert torch.equal(bits(o), bits(full[k])), (NAMES[k], drop)


# ------------------------------------------------------------------------------------------------------ d. sample_pdf
def pdf_inputs(N, nb, ns, seed):
    """tests/test_gpu_parity.py::test_sample_pdf_size_sweep: every bin carries mass, random u plus u on cdf values"""
    rng = np.random.default_rng(seed)
    bins = np.sort(rng.uniform(2, 6, (N, nb)).astype(np.float32), -1)
    w = rng.uniform(0.5, 1.5, (N, nb - 1)).astype(np.float32)
    u = rng.uniform(0, 1, (N, ns)).astype(np.float32)
    wn = w + np.float32(1e-5)
    cdf = np.concatenate([np.zeros((N, 1), np.float32), np.cumsum(wn / wn.sum(-1, keepdims=True), -1, dtype=np.float32)], -1)
    if ns > 1:
        u[:, 0] = cdf[:, min(1, nb - 1)]                       # ties with an interior / the last cdf value (right=True)
        u[:, -1] = 0.0                                         # draws bins[:, 0] exactly
    if ns > 4:
        u[:, 1] = cdf[:, nb // 2]
        u[:, 2] = np.minimum(cdf[:, -1], np.float32(1.0))
    return bins, w, u


def pdf_reference(bins, w, ns, u):
    u64 = torch.linspace(0., 1., ns).expand(bins.shape[0], ns).double() if u is None else T(u).double()
    return O.sample_pdf(T(bins).double(), T(w).double(), ns, det=False, u=u64.contiguous())


@pytest.mark.parametrize("nb", [2, 3, 4, 5, 64, 65, 1023, 1024])
@pytest.mark.parametrize("ns", [1, 2, 63, 64, 65, 1024, 2047, 2048])
def test_sample_pdf_at_its_limits(sw, dev, nb, ns):
    worst = 0.0
    for N in (1, 5):
        bins, w, u = pdf_inputs(N, nb, ns, 10000 * N + 10 * nb + ns)
        for uu in (None, u):
            got = sw.ray.sample_pdf(T(bins).to(dev), T(w).to(dev), ns, det=uu is None, u=None if uu is None else T(uu).to(dev))
            assert got.shape == (N, ns)
            worst = max(worst, close(got, pdf_reference(bins, w, ns, uu), atol=5e-5, what=f"sample_pdf N={N} nb={nb} ns={ns} det={uu is None}"))
            if uu is not None and ns > 1:
                assert np.array_equal(_np(got)[:, -1], bins[:, 0])          # u = 0 draws the first bin edge itself
    print(f"\n[op-domain] sample_pdf nb={nb} ns={ns}: max |err| {worst:.2e}")


def _pdf_abi(L_, bins, w, ns, u, smp, z, zs, sd):
    N, nb = bins.shape
    return L_.lib().swnerf_sample_pdf(L_.ptr(bins), L_.ptr(w), N, nb, ns, L_.ptr(u), L_.ptr(smp), L_.ptr(z),
                                      0 if z is None else z.shape[1], L_.ptr(zs), L_.ptr(sd), L_.stream_of(bins))


def fused_pdf_inputs(N, S, ns, mode, seed, nb=65):
    """mode: det (u = linspace), sorted (given, ascending), random, shuffled_z (random u and the coarse depths out of order).
    Exact ties between the two lists: u = 0 draws bins[:, 0] itself, which is also a coarse depth, and every bin edge is."""
    bins, w, u = pdf_inputs(N, nb, ns, seed)
    rng = np.random.default_rng(seed + 1)
    z = rng.uniform(2, 6, (N, S)).astype(np.float32)
    edges = bins[:, rng.permutation(nb)[:min(S, nb)]]          # bins[:, 0] first once sorted: it is the smallest edge
    edges[:, 0] = bins[:, 0]
    z[:, :edges.shape[1]] = edges
    z = np.sort(z, -1)
    if mode == "sorted":
        u = np.sort(u, -1)
    if mode == "shuffled_z":
        z = rng.permuted(z, axis=1)
    return bins, w, (None if mode == "det" else u), z


@pytest.mark.parametrize("mode", ["det", "sorted", "random", "shuffled_z"])
@pytest.mark.parametrize("S,ns", [(1, 2047), (1024, 1024), (64, 1984), (2047, 1)])
def test_sample_pdf_fused_merge_and_std(dev, L_, S, ns, mode):
    for N in (1, 5):
        bins, w, u, z = fused_pdf_inputs(N, S, ns, mode, 77 * S + ns + N)
        bins, w, z = (T(a).to(dev) for a in (bins, w, z))
        u = None if u is None else T(u).to(dev)
        nan = lambda *shape: torch.full(shape, float("nan"), device=dev)       # a slot the kernel leaves unwritten shows
        smp, zs, sd = nan(N, ns), nan(N, S + ns), nan(N)
        L_.check(_pdf_abi(L_, bins, w, ns, u, smp, z, zs, sd), "sample_pdf")
        what = f"fused sample_pdf S={S} ns={ns} {mode} N={N}"
        plain = nan(N, ns)                                      # the samples are those of the plain call, in draw order
        L_.check(_pdf_abi(L_, bins, w, ns, u, plain, None, None, None), "sample_pdf")
        assert torch.equal(bits(plain), bits(smp)), what
        close(smp, pdf_reference(_np(bins), _np(w), ns, None if u is None else _np(u)), atol=5e-5, what=what)
        assert torch.equal(bits(torch.sort(torch.cat([z, smp], -1), -1)[0]), bits(zs)), f"{what}: z_sorted != sort(cat[z, samples])"
        ties = int((smp[:, :, None] == z[:, None, :]).any(-1).sum()) if S * ns <= 1 << 21 else -1
        assert ties != 0 or (u is not None and ns == 1), f"{what}: the case holds no exact tie"     # a single random u draws none
        s64 = smp.double().cpu()
        ref_sd = ((s64 - s64.mean(-1, keepdim=True)) ** 2).mean(-1).sqrt()
        err = (sd.double().cpu() - ref_sd).abs()
        assert bool((err <= 1e-6 * ref_sd).all()), f"{what}: z_std {sd.tolist()} vs {ref_sd.tolist()}"


def test_sample_pdf_beyond_its_limits_is_refused(sw, dev, L_):
    """nb = 1025, n_samples = 2049, S + n_samples = 2049: SWNERF_E_UNSUPP (-2), nothing launched (no output float written)"""
    N = 3
    for nb, ns, S in ((1025, 64, 0), (64, 2049, 0), (64, 2048, 1), (64, 1025, 1024), (64, 1, 2048)):
        bins, w, u = pdf_inputs(N, nb, ns, nb + ns)
        bins, w, u = (T(a).to(dev) for a in (bins, w, u))
        smp, zs, sd = Guarded((N, ns), dev), Guarded((N, S + ns), dev), Guarded((N,), dev)
        z = torch.sort(torch.rand((N, S), device=dev) * 4 + 2, -1)[0] if S else None
        rc = _pdf_abi(L_, bins, w, ns, u, smp.out, z, zs.out if S else None, sd.out if S else None)
        assert rc == -2, (nb, ns, S, rc)
        with pytest.raises(RuntimeError, match="code -2"):
            L_.check(rc, "sample_pdf")
        assert smp.untouched() and zs.untouched() and sd.untouched(), (nb, ns, S)
    bins, w, u = pdf_inputs(N, 64, 2049, 1)
    with pytest.raises(RuntimeError, match="at most 2048 samples"):
        sw.ray.sample_pdf(T(bins).to(dev), T(w).to(dev), 2049, det=True)


# --------------------------------------------------------------------------------------------------- e. sample_coarse
def coarse_inputs(N, S, seed):
    rng = np.random.default_rng(seed)
    near = rng.uniform(0.5, 3.0, (N, 1)).astype(np.float32)
    far = (near + rng.uniform(0.5, 5.0, (N, 1))).astype(np.float32)
    far[::7] = near[::7]                                       # near == far: every depth of the ray coincides
    o, d = rng.standard_normal((N, 3)).astype(np.float32), rng.standard_normal((N, 3)).astype(np.float32)
    rb = np.concatenate([o, d, near, far], 1)
    return rb, near, far, rng.uniform(0, 1, (N, S)).astype(np.float32)


@pytest.mark.parametrize("S", [1, 2, 3, 63, 64, 65, 257, 1024])
def test_sample_coarse_sizes(sw, dev, S):
    N = 37
    rb, near, far, t_rand = coarse_inputs(N, S, S)
    for lindisp in (False, True):
        for tr in (None, t_rand):
            what = f"sample_coarse S={S} lindisp={lindisp} jitter={tr is not None}"
            z, pts = sw.render.sample_coarse(T(rb).to(dev), S, lindisp, None if tr is None else T(tr).to(dev), want_pts=True)
            ref = O.coarse_z(T(near), T(far), S, lindisp, None if tr is None else T(tr))
            assert z.shape == (N, S) and pts.shape == (N, S, 3)
            if tr is None:
                assert torch.equal(bits(z.cpu()), bits(ref.contiguous())), f"{what}: max |delta| {float((z.cpu() - ref).abs().max()):.3e}"
            else:
                close(z, ref, atol=1e-6, what=what)
            o, d = T(rb[:, None, 0:3]).to(dev), T(rb[:, None, 3:6]).to(dev)
            assert torch.equal(pts, o + d * z[..., None]), f"{what}: pts != o + d * z"


# ---------------------------------------------------------------------------------- f. write guards, without faults
@pytest.mark.parametrize("off", [1024, 1027])
def test_outputs_stay_inside_their_buffers(sw, dev, L_, off):
    """Each op at its largest and at its most ragged shape, through the ABI, every output in the middle of a sentinel-filled
    buffer (16-byte aligned and not): the floats in front and behind keep their bits, the output those of a plain call."""
    st = lambda t: L_.stream_of(t)
    for d, L, M in ((16, 24, 4097), (5, 7, 67), (3, 10, 65), (1, 0, 1)):
        x = T(embed_inputs(M, d, 3)).to(dev)
        g = Guarded((M, d * (1 + 2 * L)), dev, off)
        L_.check(L_.lib().swnerf_embed(L_.ptr(x), M, d, L, L_.ptr(g.out), st(x)), "embed")
        g.check(f"embed d={d} L={L} M={M}")
        assert torch.equal(bits(g.out), bits(sw.embedder.get_embedder(L, d, 0)[0](x)))
    for N, S in ((41, 2049), (5, 65), (1, 2)):
        raw, z, d, noise, _ = comp_inputs("soft_then_wall", S, 13, N=N)
        raw, z, d, noise = (T(a).to(dev) for a in (raw, z, d, noise))
        gs = [Guarded(s, dev, off) for s in _r2o_shapes(N, S).values()]
        _r2o_abi(L_, raw, z, d, noise, True, [g.out for g in gs])
        plain = sw.ray.raw2outputs(raw, z, d, 0, True, noise=noise)
        for g, name, p in zip(gs, NAMES, plain):
            g.check(f"raw2outputs {name} N={N} S={S}")
            assert torch.equal(bits(g.out), bits(p)), name
    for N, nb, S, ns in ((5, 1024, 1024, 1024), (5, 1024, 1, 2047), (3, 5, 3, 65), (1, 2, 1, 1)):
        bins, w, u, z = fused_pdf_inputs(N, S, ns, "random", 17, nb=nb)
        bins, w, u, z = (T(a).to(dev) for a in (bins, w, u, z))
        smp, zs, sd = Guarded((N, ns), dev, off), Guarded((N, S + ns), dev, off), Guarded((N,), dev, off)
        L_.check(_pdf_abi(L_, bins, w, ns, u, smp.out, z, zs.out, sd.out), "sample_pdf")
        for g, name in ((smp, "samples"), (zs, "z_sorted"), (sd, "z_std")):
            g.check(f"sample_pdf {name} N={N} nb={nb} S={S} ns={ns}")
        assert torch.equal(bits(smp.out), bits(sw.ray.sample_pdf(bins, w, ns, u=u)))
        assert torch.equal(bits(zs.out), bits(torch.sort(torch.cat([z, smp.out], -1), -1)[0]))
    for N, S in ((37, 1024), (5, 65), (1, 1)):
        rb, _, _, tr = coarse_inputs(N, S, 19)
        rb, tr = T(rb).to(dev), T(tr).to(dev)
        gz, gp = Guarded((N, S), dev, off), Guarded((N, S, 3), dev, off)
        L_.check(L_.lib().swnerf_sample_coarse(L_.ptr(rb), N, 8, S, 0, L_.ptr(tr), L_.ptr(gz.out), L_.ptr(gp.out), st(rb)), "sample_coarse")
        gz.check(f"sample_coarse z N={N} S={S}")
        gp.check(f"sample_coarse pts N={N} S={S}")
        zp, pp = sw.render.sample_coarse(rb, S, False, tr, want_pts=True)
        assert torch.equal(bits(gz.out), bits(zp)) and torch.equal(bits(gp.out), bits(pp))
