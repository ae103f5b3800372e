"""Density profiles for the compositing tests and their float64 reference (ray.py:155-198 through the CPU oracle), shared by
tests/test_gpu_op_domain.py (the standalone ops) and tests/test_gpu_fused_tail.py (the fused passes and their backward kernels).

REGIMES are the five the standalone ops have been held to since they were written; their seeds and arrays must not move
(test_gpu_op_domain.py derives its seeds from REGIMES.index).  ALL_REGIMES adds `spike`: one opaque sample per ray, everything
else empty, the spike placed on the samples where a tile or sweep boundary of the fused kernels falls.

POISONS and the poison_* helpers are the non-finite cases of tests/test_gpu_nonfinite.py: NaN, +Inf or -Inf on ONE sample of every
other ray - in the density (through `noise`), in a colour column of `raw`, or in a coarse weight of sample_pdf - on the same
boundary samples as the spikes.  tests/test_nonfinite_host.py checks on the CPU that the float32 and the float64 oracle agree on
the non-finite pattern of every such case, so that a pattern difference on the GPU is the kernel's."""
import numpy as np
import torch

from oracle import nerf_oracle as O

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
SENTINEL = 0x5EED5EED                  # a finite float pattern no kernel here produces by accident


def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def close(a, b, atol, rtol=0.0, what=""):
    """every element: |a - b| <= atol + rtol |b|, equal NaN pattern; b is the float64 truth"""
    a, b = _np(a).astype(np.float64), _np(b).astype(np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN pattern differs"
    if a.size == 0:
        return 0.0
    err = np.abs(np.nan_to_num(a) - np.nan_to_num(b))
    lim = atol + rtol * np.abs(np.nan_to_num(b))
    worst = float((err - lim).max())
    assert worst <= 0.0, f"{what}: max err {err.max():.3e} (|ref| up to {np.abs(np.nan_to_num(b)).max():.3e}), worst excess {worst:.3e}"
    return float(err.max())


def bits(t):
    return t.contiguous().view(torch.int32)


class Guarded:
    """n floats in the middle of a larger buffer filled with a sentinel bit pattern: `out` is what a kernel writes, check()
    holds the floats in front of and behind it to their bits.  `off` floats in front (1024: 16-byte aligned; 1027: not)."""
    PAD = 1024

    def __init__(self, shape, dev, off=1024):
        self.n = int(np.prod(shape))
        self.off = off
        self.buf = torch.full((off + self.n + self.PAD,), SENTINEL, dtype=torch.int32, device=dev)
        self.out = self.buf[off:off + self.n].view(torch.float32).view(*shape) if self.n else torch.empty(shape, device=dev)

    def check(self, what):
        torch.cuda.synchronize()
        assert bool((self.buf[:self.off] == SENTINEL).all()), f"{what}: wrote in front of the output"
        assert bool((self.buf[self.off + self.n:] == SENTINEL).all()), f"{what}: wrote behind the output"

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == SENTINEL).all())


REGIMES = ("mild", "wall", "soft_then_wall", "all_opaque", "all_empty")
ALL_REGIMES = REGIMES + ("spike",)
UPSTREAM = ("rgb", "disp", "acc", "weights", "depth", "all")
NAMES = ("rgb", "disp", "acc", "weights", "depth")


def spike_positions(S, N, rng):
    """[N, 1] index of the one opaque sample of each ray: sample 0, the last one, and both sides of a 32-sample tile boundary
    (31 | 32) and of a 64-sample sweep boundary (63 | 64) wherever S allows, in that order over the first rays (nine rays see all
    of them whatever S is); random behind."""
    must = []
    for j in (0, S - 1, 31, 32, 63, 64):
        if 0 <= j < S and j not in must:
            must.append(j)
    j = rng.integers(0, S, N)
    n = min(N, len(must))
    j[:n] = must[:n]
    return j[:, None]


POISONS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
POISON_S = (2, 33, 65, 257)            # compositing: one tile, a tile and a sweep boundary; 257: the standalone op's fifth sweep
POISON_PDF = ((64, 128), (64, 1), (1, 64), (128, 64))       # (S, Ni) at nb = 65: S > Ni, S < Ni, Ni = 1, S = 1
POISON_NB = 65


def poison_positions(S, N, rng):
    """-> (rays [k], samples [k]): the poisoned rays are the odd ones - k = N // 2, so more than half of the rays stay clean and
    a prefix of 3 or 5 rays holds both kinds - and each has ONE poisoned sample, placed by spike_positions' rule: sample 0, the
    last one, 31 | 32 and 63 | 64 where S allows, over the first poisoned rays; random behind."""
    rays = np.arange(1, N, 2)
    assert 2 * len(rays) <= N
    return rays, spike_positions(S, len(rays), rng)[:, 0]


def poison_comp_inputs(S, kind, where, N=41):
    """comp_inputs' mild regime (|sigma| and |rgb| of a few units, depths in 2 .. 6: nothing float32 overflows and float64 does
    not) with POISONS[kind] on one sample of every odd ray: where = "density" (through noise, so raw stays finite) or "colour"
    (column ray-index mod 3 of raw) -> (raw, z, d, noise, ups, rays, samples)"""
    seed = 100 * S + 10 * list(POISONS).index(kind) + ("density", "colour").index(where)
    raw, z, d, noise, ups = comp_inputs("mild", S, 424200 + seed, N=N)
    rays, j = poison_positions(S, N, np.random.default_rng(seed))
    if where == "density":
        noise[rays, j] = POISONS[kind]
    else:
        raw[rays, j, rays % 3] = POISONS[kind]
    return raw, z, d, noise, ups, rays, j


def poison_pdf_inputs(S, Ni, kind, mode, target="weight", N=41):
    """sample_pdf (+ merge) at nb = 65 bins: sorted bins and coarse depths in 2 .. 6, weights in 0.5 .. 1.5, u absent (mode "det") or
    random.  target "weight": POISONS[kind] in one weight of every odd ray; "u": in one draw (mode "random" only)
    -> (bins, w, u or None, z, rays, positions)"""
    seed = 1000 * S + 10 * Ni + list(POISONS).index(kind) + 3 * (mode == "random") + 7 * (target == "u")
    rng = np.random.default_rng(515100 + seed)
    bins = np.sort(rng.uniform(2, 6, (N, POISON_NB)).astype(np.float32), -1)
    w = rng.uniform(0.5, 1.5, (N, POISON_NB - 1)).astype(np.float32)
    z = np.sort(rng.uniform(2, 6, (N, S)).astype(np.float32), -1)
    u = None if mode == "det" else rng.uniform(0, 1, (N, Ni)).astype(np.float32)
    rays, j = poison_positions(Ni if target == "u" else POISON_NB - 1, N, rng)
    if target == "u":
        u[rays, j] = POISONS[kind]
    else:
        w[rays, j] = POISONS[kind]
    return bins, w, u, z, rays, j


POISON_UPS = ("rgb", "acc", "depth", "weights", ("rgb", "acc", "depth", "weights"))     # no disparity: the gradient of
#                                                 max(1e-10, NaN) is an ATen implementation detail, not a rule of the reference


def poison_fused_noise(S, kind, sigma, N=41):
    """the `noise` operand that turns a net's constant density `sigma` into comp_inputs' mild densities, with POISONS[kind] on one
    sample of every odd ray, and sorted depths to give the pass -> (noise, z, rays, samples)"""
    raw, z, _, _, _ = comp_inputs("mild", S, 636300 + S, N=N)
    noise = (raw[..., 3] - np.float32(sigma)).astype(np.float32)
    rays, j = poison_positions(S, N, np.random.default_rng(S + list(POISONS).index(kind)))
    noise[rays, j] = POISONS[kind]
    return noise, z, rays, j


def same_nonfinite(a, b):
    """equal NaN positions, and equal Inf positions and signs (b is the reference)"""
    a, b = _np(a), _np(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.where(np.isinf(b), b, 0), np.where(np.isinf(a), a, 0))


def comp_inputs(regime, S, seed, N=41):
    """densities a trained scene produces (random nets do not); everything float32"""
    rng = np.random.default_rng(seed)
    raw = (rng.standard_normal((N, S, 4)) * 1.5).astype(np.float32)
    idx = np.arange(S)[None, :]
    if regime == "mild":
        sg = rng.standard_normal((N, S)) * 3.0 - 0.5
    elif regime == "wall":                                   # empty space, then a surface from a random sample on
        j = rng.integers(0, S, (N, 1))
        sg = np.where(idx >= j, 10.0 ** rng.uniform(2, 4, (N, S)), -0.1 - np.abs(rng.standard_normal((N, S))))
    elif regime == "soft_then_wall":
        j = rng.integers((S + 1) // 2, S, (N, 1)) if S > 2 else np.ones((N, 1), np.int64)
        sg = np.where(idx >= j, 10.0 ** rng.uniform(1, 3, (N, S)), np.abs(rng.standard_normal((N, S)) * 3.0))
    elif regime == "all_opaque":
        sg = 10.0 ** rng.uniform(3, 6, (N, S))
    elif regime == "spike":                                  # one sample holds the whole ray, every other one is empty
        sg = np.where(idx == spike_positions(S, N, rng), 1e4, -0.1 - np.abs(rng.standard_normal((N, S))))
    else:
        sg = np.full((N, S), -2.0)
    raw[..., 3] = sg.astype(np.float32)
    z = np.sort(rng.uniform(2, 6, (N, S)).astype(np.float32), -1)
    d = rng.standard_normal((N, 3)).astype(np.float32)
    noise = (rng.standard_normal((N, S)) * 0.5).astype(np.float32)
    if regime in ("all_empty", "spike"):
        noise = -np.abs(noise)                               # stays empty under noise: disp NaN, acc 0, every sigma gradient exactly 0
    ups = {"rgb": rng.standard_normal((N, 3)).astype(np.float32), "disp": rng.standard_normal(N).astype(np.float32),
           "acc": rng.standard_normal(N).astype(np.float32), "weights": rng.standard_normal((N, S)).astype(np.float32),
           "depth": rng.standard_normal(N).astype(np.float32)}
    return raw, z, d, noise, ups


def comp_loss(outs, ups, which, conv):
    """sum of <output, upstream gradient> over the outputs named by `which` (a name, a tuple of names, or "all"): the others get
    no gradient (None at the autograd function, NULL at the ABI).  A NaN disparity (acc == 0) carries no gradient in the
    reference either: masked out."""
    tot = None
    for name, o in zip(NAMES, outs):
        if which != "all" and which != name and not (isinstance(which, tuple) and name in which):
            continue
        if name == "disp":
            o = torch.where(torch.isnan(o), torch.zeros_like(o), o)
        t = (o * conv(ups[name])[:o.shape[0]]).sum()
        tot = t if tot is None else tot + t
    return tot


def comp_reference(raw, z, d, noise, white, ups, with_grad, upstream=UPSTREAM):
    """the oracle in float64 on the float32 inputs -> (outputs, {which: d raw})"""
    r = T(raw).double().requires_grad_(with_grad)
    outs = O.raw2outputs(r, T(z).double(), T(d).double(), 0., white, noise=None if noise is None else T(noise).double())
    grads = {}
    if with_grad:
        for which in upstream:
            grads[which], = torch.autograd.grad(comp_loss(outs, ups, which, lambda a: T(a).double()), r, retain_graph=True)
    return [o.detach() for o in outs], grads
