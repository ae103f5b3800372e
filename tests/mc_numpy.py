"""Vectorised numpy restatement of the marching-cubes contract of swnerf_mc_count / swnerf_mc_emit (include/swnerf.h), on the
committed case table (sw-nerf_amd/csrc/mc_tables.h).  The GPU kernels are pinned against it; it never calls them.

  inside      f > level, fp32 (NaN is outside)
  vertices    one per crossing grid edge, ordered by (owner point in C order, axis x < y < z)
              t = (level - f0) / (f1 - f0) in fp32, non-finite -> 0.5, clamped to [0, 1];
              coordinate a = (p_a + t) * s_a + o_a, the others p_b * s_b + o_b (fp32)
  normals     -((1 - t) g(p) + t g(p + e_a)) normalised, g = np.gradient rules / spacing; zero or non-finite -> 0
  colours     colour at p + e_a if t > 0.5 else at p
  triangles   (cell in C order of its min corner, table order), int32 indices"""
import os
import re

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "sw-nerf_amd", "csrc", "mc_tables.h")


def load_tables():
    text = open(HEADER).read()
    max_t = int(re.search(r"#define SW_MC_MAX_TRIS (\d+)", text).group(1))
    body = lambda name: text[text.index(name):].split("{", 1)[1].split("};", 1)[0]
    ntri = np.array([int(x) for x in re.findall(r"-?\d+", body("sw_mc_ntri[256]"))], np.int64)
    tri_body = re.sub(r"//[^\n]*", "", body("sw_mc_tri[256]"))
    tri = np.array([int(x) for x in re.findall(r"-?\d+", tri_body)], np.int64).reshape(256, 3 * max_t)
    assert ntri.shape == (256,)
    return ntri, tri


NTRI, TRI = load_tables()


def edge_base(e):
    """(axis, corner offset (di, dj, dk)) of edge e."""
    a = e >> 2
    o = [0, 0, 0]
    b, c = [x for x in range(3) if x != a]
    o[b], o[c] = e & 1, (e >> 1) & 1
    return a, tuple(o)


def _gradient(f, s):
    g = []
    for b in range(3):
        n = f.shape[b]
        out = np.empty_like(f)
        sl = lambda a, z=None: tuple(slice(a, z) if x == b else slice(None) for x in range(3))
        with np.errstate(all="ignore"):
            out[sl(1, n - 1)] = (f[sl(2, None)] - f[sl(0, n - 2)]) / (np.float32(2) * s[b])
            out[sl(0, 1)] = (f[sl(1, 2)] - f[sl(0, 1)]) / s[b]
            out[sl(n - 1, n)] = (f[sl(n - 1, n)] - f[sl(n - 2, n - 1)]) / s[b]
        g.append(out)
    return g


def marching_cubes(f, level, spacing=(1., 1., 1.), origin=(0., 0., 0.), colors=None, return_t=False):
    f = np.ascontiguousarray(f, dtype=np.float32)
    nx, ny, nz = f.shape
    L = np.float32(level)
    s = np.asarray(spacing, np.float32)
    o = np.asarray(origin, np.float32)
    ins = f > L
    N = f.size
    cross = []
    for a in range(3):
        c = np.zeros(f.shape, bool)
        lo = tuple(slice(0, -1) if x == a else slice(None) for x in range(3))
        hi = tuple(slice(1, None) if x == a else slice(None) for x in range(3))
        c[lo] = ins[lo] != ins[hi]
        cross.append(c.ravel())
    mask = cross[0].astype(np.int64) | (cross[1].astype(np.int64) << 1) | (cross[2].astype(np.int64) << 2)
    nv = cross[0].astype(np.int64) + cross[1] + cross[2]
    voff = np.concatenate([[0], np.cumsum(nv)[:-1]]) if N else np.zeros(0, np.int64)
    # vertices: keys owner * 3 + axis, sorted
    keys = np.sort(np.concatenate([np.nonzero(cross[a])[0] * 3 + a for a in range(3)]))
    p, ax = keys // 3, keys % 3
    step = np.array([ny * nz, nz, 1], np.int64)
    q = p + step[ax]
    ff = f.ravel()
    f0, f1 = ff[p], ff[q]
    with np.errstate(all="ignore"):
        t = (L - f0) / (f1 - f0)
    t = np.where(np.isfinite(t), t, np.float32(0.5)).astype(np.float32)
    t = np.minimum(np.maximum(t, np.float32(0)), np.float32(1))
    idx = np.stack(np.unravel_index(p, f.shape), 1).astype(np.int64)
    verts = np.empty((len(p), 3), np.float32)
    for b in range(3):
        pb = idx[:, b].astype(np.float32)
        verts[:, b] = np.where(ax == b, (pb + t) * s[b], pb * s[b]) + o[b]
    G = [g.ravel() for g in _gradient(f, s)]
    with np.errstate(all="ignore"):
        n = np.stack([-((np.float32(1) - t) * G[b][p] + t * G[b][q]) for b in range(3)], 1)
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        r = n / ln[:, None]
    bad = ~(ln > 0) | ~np.isfinite(r).all(1)
    r[bad] = 0
    normals = r.astype(np.float32)
    vcol = None
    if colors is not None:
        cf = np.asarray(colors, np.float32).reshape(N, 3)
        vcol = cf[np.where(t > np.float32(0.5), q, p)]
    # triangles
    cells = np.zeros(f.shape, np.int64)
    inner = (slice(0, -1),) * 3
    for cn in range(8):
        di, dj, dk = cn & 1, (cn >> 1) & 1, (cn >> 2) & 1
        cells[inner] |= ins[di:nx - 1 + di, dj:ny - 1 + dj, dk:nz - 1 + dk].astype(np.int64) << cn
    case = cells.ravel()
    nt = NTRI[case]
    cell = np.repeat(np.arange(N), nt)
    k = np.arange(len(cell)) - np.repeat(np.cumsum(nt) - nt, nt)
    faces = np.empty((len(cell), 3), np.int64)
    for v in range(3):
        e = TRI[case[cell], 3 * k + v]
        owner = np.empty_like(cell)
        a = e >> 2
        for ee in range(12):
            ea, (di, dj, dk) = edge_base(ee)
            sel = e == ee
            owner[sel] = cell[sel] + di * ny * nz + dj * nz + dk
        faces[:, v] = voff[owner] + _popcount(mask[owner] & ((1 << a) - 1))
    out = (verts, faces.astype(np.int32), normals, vcol)
    return out + (t,) if return_t else out


def _popcount(x):
    return (x & 1) + ((x >> 1) & 1) + ((x >> 2) & 1)


# ---------------------------------------------------------------- geometric checks
def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)


def is_closed_oriented_manifold(faces):
    """every directed edge appears once and its reverse once"""
    e = directed_edges(faces)
    if len(e) == 0:
        return True
    m = int(e.max()) + 1
    key = e[:, 0] * m + e[:, 1]
    rev = e[:, 1] * m + e[:, 0]
    uk, cnt = np.unique(key, return_counts=True)
    if (cnt != 1).any():
        return False
    return bool(np.isin(rev, uk).all())


def euler_characteristic(n_verts, faces):
    e = directed_edges(faces)
    undirected = np.unique(np.sort(e, 1), axis=0)
    used = np.unique(np.asarray(faces).ravel()).size
    assert used == n_verts, "unreferenced vertices"
    return n_verts - len(undirected) + len(faces)


def area_volume(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    cr = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    area = 0.5 * np.linalg.norm(cr, axis=1).sum()
    vol = np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0
    return area, vol


# ---------------------------------------------------------------- test fields
def grid(R, lo=-1.0, hi=1.0):
    x = np.linspace(lo, hi, R)
    return np.meshgrid(x, x, x, indexing="ij"), x[1] - x[0]


def sphere(R, r=0.6):
    (X, Y, Z), h = grid(R)
    return (r - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32), h


def torus(R, Rmaj=0.55, rmin=0.22):
    (X, Y, Z), h = grid(R)
    q = np.sqrt(X ** 2 + Y ** 2) - Rmaj
    return (rmin - np.sqrt(q ** 2 + Z ** 2)).astype(np.float32), h


def two_spheres(R):
    (X, Y, Z), h = grid(R)
    a = 0.35 - np.sqrt((X - 0.45) ** 2 + Y ** 2 + Z ** 2)
    b = 0.35 - np.sqrt((X + 0.45) ** 2 + Y ** 2 + Z ** 2)
    return np.maximum(a, b).astype(np.float32), h


def noise(shape, seed=0, pad=True):
    """seeded smooth-ish noise; pad=True surrounds it by a 1-point border far below any level (a closed surface)"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal(shape).astype(np.float32)
    for a in range(3):                                 # a little smoothing so the surface is not all single-cell blobs
        f = (f + np.roll(f, 1, a) + np.roll(f, -1, a)) / np.float32(3)
    f = f.astype(np.float32)
    if pad:
        f = np.pad(f, 1, constant_values=np.float32(-100))
    return f
