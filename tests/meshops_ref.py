"""Vectorised numpy restatement of the mesh clean-up and measurement contract (swnerf_mesh_* of include/swnerf.h, DESIGN.md 6b
"Clean-up and measurement").  The GPU kernels and csrc/meshops_math.h are pinned against it; it never calls them.

  components   min-label propagation over the edges (a, b), (b, c) of every face, with pointer jumping, until nothing changes:
               label = the smallest vertex index of the component; table rows (label, faces, vertices), ascending
  selection    at least min_faces faces, then the `keep` largest by face count, a tie to the smaller label
  compaction   verts[mask], remap[faces[fmask]]
  incidence    stable argsort of the flattened faces: corner ids 3 f + k per vertex, ascending
  smoothing    out = float32(p + float64(s) * (S / (2 n) - p)), S added corner by corner in (vertex, corner id) order in float64
               (np.add.at applies its updates in index order)
  normals      the float64 face crosses added in the same order, normalised
  measure      per-face terms in float64 exactly as csrc/meshops_math.h writes them; sums by math.fsum (correctly rounded)"""
import math

import numpy as np

import mc_numpy as M


# ---------------------------------------------------------------------------------------------------------------- components
def vertex_labels(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    lab = np.arange(V, dtype=np.int64)
    if len(f) == 0:
        return lab
    a = np.concatenate([f[:, 0], f[:, 1]])
    b = np.concatenate([f[:, 1], f[:, 2]])
    while True:
        m = np.minimum(lab[a], lab[b])
        new = lab.copy()
        np.minimum.at(new, a, m)
        np.minimum.at(new, b, m)
        new = new[new]                                     # pointer jumping: labels only ever name a vertex of the same component
        if np.array_equal(new, lab):
            return lab
        lab = new


def component_table(faces, V):
    """-> (vlabel int64 [V], table int64 [C,3] = (label, faces, vertices) in ascending label order)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    lab = vertex_labels(f, V)
    labels, nv = np.unique(lab, return_counts=True)
    nf = np.zeros(V, np.int64)
    if len(f):
        np.add.at(nf, lab[f[:, 0]], 1)
    return lab, np.stack([labels, nf[labels], nv], 1).reshape(-1, 3)


def select(table, keep=1, min_faces=1):
    rows = [r for r in np.asarray(table, np.int64).reshape(-1, 3).tolist() if r[1] >= min_faces]
    if keep != "all":
        rows = sorted(rows, key=lambda r: (-r[1], r[0]))[:keep]
    return np.array(sorted(rows), np.int64).reshape(-1, 3)


def compact(verts, faces, vlabel, kept_labels, *rest):
    """-> (verts[mask], remap[faces[fmask]], *[r[mask] for r in rest])"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    mask = np.isin(vlabel, kept_labels)
    fmask = mask[f[:, 0]] if len(f) else np.zeros(0, bool)
    remap = np.cumsum(mask) - 1
    return (verts[mask], remap[f[fmask]].astype(np.int32).reshape(-1, 3)) + tuple(None if r is None else r[mask] for r in rest)


# ----------------------------------------------------------------------------------------------------------------- incidence
def incidence(faces, V):
    flat = np.asarray(faces, np.int64).reshape(-1)
    items = np.argsort(flat, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=V))])
    return offsets.astype(np.int32), items.astype(np.int32)


# ----------------------------------------------------------------------------------------------------------------- smoothing
def smooth_step(verts, faces, s):
    P = np.asarray(verts, np.float32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(P)
    if len(f) == 0:
        return P.copy()
    offsets, items = incidence(f, V)
    c = items.astype(np.int64)
    owner = f.reshape(-1)[c]                               # ascending, corners ascending within a vertex
    fi, k = c // 3, c % 3
    n1, n2 = f[fi, (k + 1) % 3], f[fi, (k + 2) % 3]
    idx = np.repeat(owner, 2)
    nb = np.stack([n1, n2], 1).reshape(-1)                 # per corner: next, then previous
    S = np.zeros((V, 3), np.float64)
    np.add.at(S, idx, P[nb].astype(np.float64))
    n = np.diff(offsets).astype(np.int64)
    p = P.astype(np.float64)
    with np.errstate(all="ignore"):
        m = S / (2 * n).astype(np.float64)[:, None]
        out = (p + np.float64(np.float32(s)) * (m - p)).astype(np.float32)
    out[n == 0] = P[n == 0]
    return out


def smooth(verts, faces, iterations=10, lam=0.5, mu=-0.53):
    P = np.asarray(verts, np.float32).copy()
    for _ in range(iterations):
        P = smooth_step(P, faces, lam)
        P = smooth_step(P, faces, mu)
    return P


def face_cross(verts, faces):
    P = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    u, v = P[f[:, 1]] - P[f[:, 0]], P[f[:, 2]] - P[f[:, 0]]
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)


def vertex_normals(verts, faces):
    """float64 [V,3] (the device rounds each component to float32)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(verts)
    S = np.zeros((V, 3), np.float64)
    if len(f):
        _, items = incidence(f, V)
        c = items.astype(np.int64)
        np.add.at(S, f.reshape(-1)[c], face_cross(verts, f)[c // 3])
    with np.errstate(all="ignore"):
        ln = np.sqrt((S[:, 0] * S[:, 0] + S[:, 1] * S[:, 1]) + S[:, 2] * S[:, 2])
        r = S / ln[:, None]
    r[~(ln > 0) | ~np.isfinite(r).all(1)] = 0
    return r


# ------------------------------------------------------------------------------------------------------------------- measure
def face_terms(verts, faces):
    """float64 [F,5]: area, volume, three first moments, operation for operation as meshops_face_terms"""
    P = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    c = face_cross(verts, f)
    a, b, d = P[f[:, 0]], P[f[:, 1]], P[f[:, 2]]
    area = 0.5 * np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    kx = b[:, 1] * d[:, 2] - b[:, 2] * d[:, 1]
    ky = b[:, 2] * d[:, 0] - b[:, 0] * d[:, 2]
    kz = b[:, 0] * d[:, 1] - b[:, 1] * d[:, 0]
    vol = ((a[:, 0] * kx + a[:, 1] * ky) + a[:, 2] * kz) / 6.0
    mom = [vol * (((a[:, q] + b[:, q]) + d[:, q]) / 4.0) for q in range(3)]
    return np.stack([area, vol] + mom, 1)


def edge_counts(faces):
    """-> (undirected edges, boundary edges, non-manifold edges): an edge is boundary when it occurs once in all, non-manifold
    when it occurs more than twice or twice in one direction"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f) == 0:
        return 0, 0, 0
    e = M.directed_edges(f)
    lo, hi = e.min(1), e.max(1)
    fwd = (e[:, 0] <= e[:, 1]).astype(np.int64)
    key = lo * (int(hi.max()) + 1) + hi
    uk, inv = np.unique(key, return_inverse=True)
    n_f = np.bincount(inv, weights=fwd, minlength=len(uk)).astype(np.int64)
    n_b = np.bincount(inv, weights=1 - fwd, minlength=len(uk)).astype(np.int64)
    tot = n_f + n_b
    return len(uk), int((tot == 1).sum()), int(((tot > 2) | (n_f >= 2) | (n_b >= 2)).sum())


def measure(verts, faces):
    """dict with the fields of swnerf.mesh.measure plus `terms` (the [F,5] per-face terms) and `sums` (their math.fsum)"""
    P = np.asarray(verts, np.float32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    t = face_terms(P, f)
    sums = np.array([math.fsum(t[:, q].tolist()) for q in range(5)])
    ref = np.unique(f)
    E, nb, nm = edge_counts(f)
    _, table = component_table(f, len(P))
    lo = P[ref].min(0).astype(np.float64) if len(ref) else None
    hi = P[ref].max(0).astype(np.float64) if len(ref) else None
    return dict(terms=t, sums=sums, area=sums[0], volume=sums[1], moments=sums[2:5], bbox_min=lo, bbox_max=hi,
                referenced_vertices=len(ref), edges=E, boundary_edges=nb, nonmanifold_edges=nm,
                n_components=int((table[:, 1] > 0).sum()), euler=len(ref) - E + len(f), closed=nb == 0 and nm == 0)


# ------------------------------------------------------------------------------------------------------------------ fixtures
def mc(field, level, h):
    """mc_numpy's marching cubes on a [-1, 1]^3 grid of spacing h -> (verts, faces, normals)"""
    v, f, n, _ = M.marching_cubes(field, level, (h, h, h), (-1., -1., -1.))
    return v, f, n


def floater_field(R=20):
    """a radius-0.5 sphere and three radius-0.12 blobs: the floater case (482 vertices, 948 faces; components of 812, 56, 40, 40)"""
    (X, Y, Z), h = M.grid(R)
    f = 0.5 - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)
    for (cx, cy, cz) in ((0.8, 0.8, 0.8), (-0.8, 0.7, -0.75), (0.75, -0.8, 0.1)):
        f = np.maximum(f, 0.12 - np.sqrt((X - cx) ** 2 + (Y - cy) ** 2 + (Z - cz) ** 2))
    return f.astype(np.float32), h


def fan(n=300):
    """a cone: apex 0 of valence n over a ring of n vertices (open at the base)"""
    a = 2 * np.pi * np.arange(n) / n
    v = np.concatenate([[[0., 0., 1.]], np.stack([np.cos(a), np.sin(a), np.zeros(n)], 1)]).astype(np.float32)
    k = np.arange(n)
    f = np.stack([np.zeros(n, np.int64), 1 + k, 1 + (k + 1) % n], 1).astype(np.int32)
    return v, f


def fixtures():
    """name -> (verts float32 [V,3], faces int32 [F,3], marching-cubes normals or None)"""
    out = {}
    for name, (field, h), level in (("two_spheres", M.two_spheres(16), 0.), ("sphere", M.sphere(16), 0.), ("torus", M.torus(20), 0.),
                                    ("floaters", floater_field(20), 0.)):
        out[name] = mc(field, level, h)
    v, f, n, _ = M.marching_cubes(M.noise((10, 10, 10), seed=3), 0.3)
    out["noise"] = (v, f, n)
    sv, sf, sn = out["sphere"]
    out["open_sphere"] = (sv, sf[sv[sf].mean(1)[:, 2] <= 0], None)
    out["fan"] = fan(300) + (None,)
    out["empty"] = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None)
    out["triangle"] = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32), None)
    out["duplicated_face"] = (sv, np.concatenate([sf, sf[7:8]]), None)
    out["unreferenced"] = (np.concatenate([sv[:2], sv, np.ones((1, 3), np.float32) * 5]), sf + 2, None)
    out["repeated_index"] = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32), np.array([[0, 0, 1], [1, 2, 3]], np.int32), None)
    return out
