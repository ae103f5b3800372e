"""csrc/resample.h restated in numpy at the kernel's own precisions: wave_sample_pdf, wave_zstd and the rank merge.

The header states where each precision sits, and the library is built with -ffp-contract=off, so every float32 operation below
is one IEEE rounding exactly as on the device:
  w + 1e-5f                          float32
  normaliser                         sum of those in float64, rounded ONCE to float32
  pdf = (w + 1e-5f) / wsum           float32
  cdf[0] = 0, cdf[i + 1]             float64 running sum of the pdf, rounded to float32 per element
  u                                  the given row, or torch.linspace(0, 1, Ni) in float32 (sw_linspace is ATen's formula)
  searchsorted(cdf, u, right=True), below = max(0, i - 1), above = min(nb - 1, i)
  den = cdf[above] - cdf[below];  den < 1e-5f -> 1
  s = bb + (u - cb) / den * (ba - bb)        every operation float32, in this order
  bins of the fused pass             0.5f * (z[i + 1] + z[i]) in float32
  z_std                              mean and variance summed in float64, sqrt in float64, rounded once
  z_fine                             sort(cat[z, samples]) - a merge yields the values of any correct sort
The kernel adds its float64 sums in another order (per-lane partial sums, then a wave scan).  A float64 sum of <= 1024 float32
terms carries a relative error of ~1e-13, so the two orders round to the same float32 unless the exact sum lies within that of
a rounding boundary: `boundary_entries` names such cdf entries, and tests count them instead of tolerating them."""
import numpy as np
import torch

F32 = np.float32
EPS = F32(1e-5)


def mid_bins(z):
    z = np.asarray(z, F32)
    return (F32(0.5) * (z[..., 1:] + z[..., :-1])).astype(F32)


def cdf_of(w):
    """-> (cdf float32 [N, nb], its float64 values before the rounding [N, nb])"""
    w = np.asarray(w, F32)
    wn = (w + EPS).astype(F32)
    wsum = wn.astype(np.float64).sum(-1).astype(F32)
    pdf = (wn / wsum[:, None]).astype(F32)
    c64 = np.concatenate([np.zeros((w.shape[0], 1)), np.cumsum(pdf.astype(np.float64), -1)], -1)
    return c64.astype(F32), c64


def linspace_u(N, Ni):
    return np.broadcast_to(torch.linspace(0., 1., Ni, dtype=torch.float32).numpy(), (N, Ni))


def draw(bins, cdf, u):
    """the inverse cdf of resample.h on a given float32 cdf -> samples [N, Ni] float32, in draw order"""
    bins, cdf, u = np.asarray(bins, F32), np.asarray(cdf, F32), np.asarray(u, F32)
    N, nb = bins.shape
    assert cdf.shape == (N, nb) and u.shape[0] == N
    hi = np.stack([np.searchsorted(cdf[r], u[r], side="right") for r in range(N)])
    below, above = np.maximum(hi - 1, 0), np.minimum(hi, nb - 1)
    take = lambda a, i: np.take_along_axis(a, i, -1)
    cb, ca, bb, ba = take(cdf, below), take(cdf, above), take(bins, below), take(bins, above)
    den = (ca - cb).astype(F32)
    den = np.where(den < EPS, F32(1.0), den).astype(F32)
    t = ((u - cb).astype(F32) / den).astype(F32)
    return (bb + (t * (ba - bb).astype(F32)).astype(F32)).astype(F32)


def sample_pdf(bins, w, Ni, u=None):
    """wave_sample_pdf: bins [N, nb], w [N, nb - 1], u [N, Ni] or None (det) -> samples [N, Ni] float32"""
    cdf, _ = cdf_of(w)
    return draw(bins, cdf, linspace_u(len(cdf), Ni) if u is None else u)


def zstd(samples):
    s = np.asarray(samples, F32).astype(np.float64)
    mean = s.sum(-1, keepdims=True) / s.shape[-1]
    return np.sqrt(((s - mean) ** 2).sum(-1) / s.shape[-1]).astype(F32)


def merge(z, samples):
    return np.sort(np.concatenate([np.asarray(z, F32), np.asarray(samples, F32)], -1), -1)


def resample(z, weights, Ni, u=None):
    """nerf/run.py:394-400,416 as the fused pass runs it: bins = mid-points of z, weights[:, 1:-1] -> (samples, z_fine, z_std)"""
    s = sample_pdf(mid_bins(z), np.asarray(weights, F32)[:, 1:-1], Ni, u)
    return s, merge(z, s), zstd(s)


def boundary_entries(c64_row, rel=2.0 ** -40):
    """indices of the cdf entries of one ray whose float64 value lies within `rel` (relative) of the mid-point of two
    neighbouring float32 values: another summation order may round these the other way"""
    c = np.asarray(c64_row, np.float64)
    f = c.astype(F32)
    other = np.where(f.astype(np.float64) <= c, np.nextafter(f, F32(np.inf)), np.nextafter(f, F32(-np.inf)))
    midpoint = 0.5 * (f.astype(np.float64) + other.astype(np.float64))
    return np.nonzero(np.abs(c - midpoint) <= rel * np.abs(c))[0], other


def explain(bins_row, w_row, u_row, got_row):
    """A ray whose device samples differ from the replay: -> the index of the ONE cdf entry that sits on a float32 rounding
    boundary and, rounded the other way, reproduces the device's samples bit for bit; None when there is no such entry."""
    cdf, c64 = cdf_of(w_row[None])
    idx, other = boundary_entries(c64[0])
    for i in idx:
        alt = cdf.copy()
        alt[0, i] = other[i]
        if np.array_equal(draw(bins_row[None], alt, u_row[None]).view(np.int32), np.asarray(got_row, F32)[None].view(np.int32)):
            return int(i)
    return None


def compare_samples(bins, w, u, got, what):
    """device samples [N, Ni] against the replay, bit for bit -> number of rays explained by a rounding-boundary cdf entry (the
    caller allows one per case); any other difference fails here"""
    bins, w, got = np.asarray(bins, F32), np.asarray(w, F32), np.asarray(got, F32)
    uu = linspace_u(bins.shape[0], got.shape[1]) if u is None else np.asarray(u, F32)
    ref = sample_pdf(bins, w, got.shape[1], uu)
    bad = np.nonzero((ref.view(np.int32) != got.view(np.int32)).any(-1))[0]
    for r in bad:
        i = explain(bins[r], w[r], uu[r], got[r])
        m = np.nonzero(ref[r].view(np.int32) != got[r].view(np.int32))[0]
        assert i is not None, (f"{what}: ray {r}: {m.size} samples differ from the replay of resample.h (first: sample {m[0]}, u {uu[r, m[0]]!r}, "
                               f"device {got[r, m[0]]!r}, replay {ref[r, m[0]]!r}) and no cdf entry sits on a rounding boundary")
    return len(bad)
