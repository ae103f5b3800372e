"""Numpy replay of mesh welding and decimation by vertex clustering (swnerf_mesh_cluster / _collapse / _collapse_emit of
include/swnerf.h, DESIGN.md 6b "Welding and decimation"), operation for operation as csrc/meshops_math.h writes it: fp64, one
rounding per operation (numpy's elementwise ufuncs never contract), sums in a fixed order (np.add.at applies its updates in index
order).  The GPU kernels and the header are pinned against it bit for bit; it never calls them.

  cell       i = floor((float64(p) - float64(o)) / float64(h)) per axis; valid iff 0 <= i < 2^21 on all three
  origin     default: the per-axis minimum by the ordered uint32 key of meshops_float_key
  label      the smallest vertex index with the same cell
  collapse   g = vlabel[face]; degenerate when two agree; duplicates share the triple rotated to its smallest label, the first stays
  members    all vertices of a label, ascending; mean = fp64 sum in that order / count
  quadric    every face with a corner of the label once, ascending: n = cross(p1 - p0, p2 - p0), d = -((n0 x + n1 y) + n2 z) at p0;
             A += n n^T (6 entries), b += n d; R = A + eps tr I; y = adj(R) (-(A m + b)) / det(R); x = m + y, or m"""
import numpy as np

import meshops_ref as R

WELD, MEAN, QUADRIC = "weld", "mean", "quadric"
CELL_LIMIT = float(2 ** 21)


def spacing(name):
    """the grid spacing a fixture of meshops_ref.fixtures() was extracted at (1 for the index-space noise meshes and the hand-made ones)"""
    return {"two_spheres": 2. / 15, "sphere": 2. / 15, "open_sphere": 2. / 15, "duplicated_face": 2. / 15, "unreferenced": 2. / 15,
            "torus": 2. / 19, "floaters": 2. / 19}.get(name, 1.)


def float_key(x):
    u = np.asarray(x, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def default_origin(verts):
    P = np.asarray(verts, np.float32).reshape(-1, 3)
    if len(P) == 0:
        return np.zeros(3, np.float32)
    k = float_key(P)
    return P[np.argmin(k, 0), np.arange(3)].copy()


def cell_index(verts, origin, h):
    """-> (idx float64 [V,3], valid bool [V])"""
    P = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        t = np.floor((P - np.asarray(origin, np.float32).astype(np.float64)[None, :]) / np.float64(np.float32(h)))
        valid = ((t >= 0.0) & (t < CELL_LIMIT)).all(1)
    return t, valid


def cluster(verts, h, origin=None):
    """-> dict(vlabel int64 [V] or None, clusters, invalid, origin float32 [3])"""
    P = np.asarray(verts, np.float32).reshape(-1, 3)
    o = default_origin(P) if origin is None else np.asarray(origin, np.float32).reshape(3)
    t, valid = cell_index(P, o, h)
    invalid = int((~valid).sum())
    if invalid:
        return dict(vlabel=None, clusters=0, invalid=invalid, origin=o)
    i = t.astype(np.uint64)
    key = i[:, 0] | (i[:, 1] << np.uint64(21)) | (i[:, 2] << np.uint64(42))
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    vlabel = first[inv.reshape(-1)].astype(np.int64)
    return dict(vlabel=vlabel, clusters=len(first), invalid=0, origin=o)


def rotate(g):
    """rows of g rotated so that the smallest entry leads (rows with equal entries are not used by the callers)"""
    s = np.argmin(g, 1)
    k = (s[:, None] + np.arange(3)[None, :]) % 3
    return np.take_along_axis(g, k, 1)


def collapse(faces, vlabel, V):
    """-> dict(bad) when an index is out of range, else dict(keep bool [F], labels (in use, ascending), vmap int64 [V] (-1: unused),
    V_out, F_out, degenerate, duplicate, bad=0)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    bad = int(((f < 0) | (f >= V)).sum())
    if bad:
        return dict(bad=bad)
    g = vlabel[f] if len(f) else np.zeros((0, 3), np.int64)
    deg = (g[:, 0] == g[:, 1]) | (g[:, 1] == g[:, 2]) | (g[:, 0] == g[:, 2])
    keep = np.zeros(len(f), bool)
    idx = np.flatnonzero(~deg)
    if len(idx):
        _, first = np.unique(rotate(g[idx]), axis=0, return_index=True)          # the first occurrence: the smallest face index
        keep[idx[first]] = True
    labels = np.unique(g[keep])
    vmap = np.full(V, -1, np.int64)
    vmap[labels] = np.arange(len(labels))
    return dict(keep=keep, labels=labels, vmap=vmap, g=g, V_out=len(labels), F_out=int(keep.sum()), degenerate=int(deg.sum()),
                duplicate=int((~deg).sum() - keep.sum()), bad=0)


def member_mean(A, vlabel):
    """float64 [V,3]: row l = the mean of the rows of A labelled l, added in ascending vertex order (rows of non-labels are NaN)"""
    A = np.asarray(A, np.float32).astype(np.float64)
    S = np.zeros_like(A)
    np.add.at(S, vlabel, A)
    n = np.bincount(vlabel, minlength=len(A)).astype(np.float64)
    with np.errstate(all="ignore"):
        return S / n[:, None]


def quadric_system(verts, faces, vlabel):
    """-> (A float64 [V,6] = xx, xy, xz, yy, yz, zz; b float64 [V,3]) per label, every face with a corner of the label once, in
    ascending face order"""
    P = np.asarray(verts, np.float32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(P)
    A, b = np.zeros((V, 6)), np.zeros((V, 3))
    if len(f) == 0:
        return A, b
    gl = vlabel[f].reshape(-1)
    order = np.argsort(gl, kind="stable")                          # (label, corner id) ascending
    lab, face = gl[order], order // 3
    firstc = np.ones(len(order), bool)
    firstc[1:] = (lab[1:] != lab[:-1]) | (face[1:] != face[:-1])
    lab, face = lab[firstc], face[firstc]
    n = R.face_cross(P, f)
    p0 = P[f[:, 0]].astype(np.float64)
    d = -((n[:, 0] * p0[:, 0] + n[:, 1] * p0[:, 1]) + n[:, 2] * p0[:, 2])
    for q, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        np.add.at(A[:, q], lab, (n[:, i] * n[:, j])[face])
    for q in range(3):
        np.add.at(b[:, q], lab, (n[:, q] * d)[face])
    return A, b


def quadric_solve(A, b, m, eps):
    """-> (y float64 [N,3], det, tr, lam) for rows of A [N,6], b [N,3], m [N,3]: the header's adjugate solve"""
    Axx, Axy, Axz, Ayy, Ayz, Azz = (A[:, q] for q in range(6))
    with np.errstate(all="ignore"):
        tr = (Axx + Ayy) + Azz
        lam = np.float64(eps) * tr
        Rxx, Ryy, Rzz, Rxy, Rxz, Ryz = Axx + lam, Ayy + lam, Azz + lam, Axy, Axz, Ayz
        rx = -(((Axx * m[:, 0] + Axy * m[:, 1]) + Axz * m[:, 2]) + b[:, 0])
        ry = -(((Axy * m[:, 0] + Ayy * m[:, 1]) + Ayz * m[:, 2]) + b[:, 1])
        rz = -(((Axz * m[:, 0] + Ayz * m[:, 1]) + Azz * m[:, 2]) + b[:, 2])
        c00, c01, c02 = Ryy * Rzz - Ryz * Ryz, Rxz * Ryz - Rxy * Rzz, Rxy * Ryz - Rxz * Ryy
        c11, c12, c22 = Rxx * Rzz - Rxz * Rxz, Rxy * Rxz - Rxx * Ryz, Rxx * Ryy - Rxy * Rxy
        det = (Rxx * c00 + Rxy * c01) + Rxz * c02
        y = np.stack([((c00 * rx + c01 * ry) + c02 * rz) / det, ((c01 * rx + c11 * ry) + c12 * rz) / det,
                      ((c02 * rx + c12 * ry) + c22 * rz) / det], 1)
    return y, det, tr, lam


def quadric_points(verts, faces, vlabel, labels, origin, h, eps):
    """float64 [len(labels),3]: the representative of every label of `labels`"""
    P = np.asarray(verts, np.float32)
    m = member_mean(P, vlabel)[labels]
    A, b = quadric_system(P, faces, vlabel)
    y, det, tr, _ = quadric_solve(A[labels], b[labels], m, eps)
    idx, _ = cell_index(P[labels], origin, h)
    h64 = np.float64(np.float32(h))
    with np.errstate(all="ignore"):
        x = m + y
        lo = np.asarray(origin, np.float32).astype(np.float64)[None, :] + idx * h64
        hi = lo + h64
        ok = (tr > 0.0) & np.isfinite(tr) & (det > 0.0) & np.isfinite(det) & (np.isfinite(x) & (x >= lo) & (x <= hi)).all(1)
    return np.where(ok[:, None], x, m)


def simplify(verts, faces, normals=None, colors=None, h=1., placement=QUADRIC, eps=1e-3, origin=None):
    """-> dict(verts float32, faces int32, normals (float32 for weld, float64 otherwise, None when none came in), colors, vlabel,
    clusters, V_out, F_out, degenerate, duplicate, origin), or dict(invalid=n) / dict(bad=n) for a refused mesh"""
    P = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    c = cluster(P, h, origin)
    if c["invalid"]:
        return dict(invalid=c["invalid"])
    vlabel, o = c["vlabel"], c["origin"]
    k = collapse(f, vlabel, len(P))
    if k["bad"]:
        return dict(bad=k["bad"])
    labels = k["labels"]
    fo = k["vmap"][k["g"][k["keep"]]].astype(np.int32).reshape(-1, 3)
    col = None
    if placement == WELD:
        vo = P[labels]
        no = None if normals is None else np.asarray(normals, np.float32)[labels]
        col = None if colors is None else np.asarray(colors, np.float32)[labels]
    else:
        x = member_mean(P, vlabel)[labels] if placement == MEAN else quadric_points(P, f, vlabel, labels, o, h, eps)
        vo = x.astype(np.float32)
        no = None if normals is None else R.vertex_normals(vo, fo)
        col = None if colors is None else member_mean(colors, vlabel)[labels].astype(np.float32)
    return dict(verts=vo.reshape(-1, 3), faces=fo, normals=no, colors=col, vlabel=vlabel, clusters=c["clusters"], V_out=k["V_out"], F_out=k["F_out"],
                degenerate=k["degenerate"], duplicate=k["duplicate"], origin=o, labels=labels, keep=k["keep"])


def first_occurrence_merge(verts, faces):
    """The textbook exact merge: equal rows of verts become their first occurrence -> (vlabel, verts', faces') with degenerate and
    duplicate faces left in (the caller compares on meshes that have none)"""
    P = np.asarray(verts, np.float32).reshape(-1, 3)
    _, first, inv = np.unique(P, axis=0, return_index=True, return_inverse=True)
    vlabel = first[inv.reshape(-1)]
    labels = np.unique(vlabel)
    remap = np.full(len(P), -1, np.int64)
    remap[labels] = np.arange(len(labels))
    return vlabel, P[labels], remap[vlabel[np.asarray(faces, np.int64)]].astype(np.int32)
