"""Numpy replay of the mesh renderer's contract (swnerf_mesh_render_* and swnerf_mesh_view_compare of include/swnerf.h,
csrc/meshrender_math.h, DESIGN.md 6b "Mesh rendering").  The GPU kernels and the header are pinned against it; it never calls them.

  rays      float32, the operations of get_rays (ray_dir of csrc/ray_rows.h) one numpy operation each
  hits      EVERY pixel against EVERY face - no boxes, no tiers - in float64 with the header's operation order; the z-buffer is the
            minimum over the faces of (float32 bits of t) << 32 | face id
  boxes     meshrender_box per (view, face), replayed only for the two counters that depend on it (pairs behind the camera, pairs
            whose box holds more than 64 pixels); the image itself never looks at a box, so a box that is too tight shows
  compare   the fp64 sums in the written order: lane sums over pixels l, l + 1024, .., folded in halves"""
import numpy as np

NARROW_PIXELS = 64
CULLS = {None: 0, "none": 0, "back": 1, "front": 2}
SHADINGS = {"colors": 0, "normals": 1, "headlight": 2}
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
CMP_LANES = 1024
STANDARD_VIEWS = ((0.3, -0.4, 2.5), (2.0, 0.7, 3.0))
TIE_VIEW = (0.0, 0.0, 2.5)
f32, f64 = np.float32, np.float64


def intrinsics(H, W, K=None, focal=None):
    """-> float32 (fx, fy, cx, cy) as get_rays casts them: the focal branch centres at W / 2, H / 2 evaluated in double"""
    if K is None:
        return f32(focal), f32(focal), f32(W * 0.5), f32(H * 0.5)
    K = np.asarray(K, f64)
    return f32(K[0, 0]), f32(K[1, 1]), f32(K[0, 2]), f32(K[1, 2])


def pose(theta, phi, r, centre=(0., 0., 0.)):
    """c2w = Ry(theta) Rx(phi) T(0, 0, r) in float32, the translation then moved to `centre` -> float32 [3,4]"""
    c, s = f32(np.cos(f32(theta))), f32(np.sin(f32(theta)))
    Ry = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]], f32)
    c, s = f32(np.cos(f32(phi))), f32(np.sin(f32(phi)))
    Rx = np.array([[1, 0, 0], [0, c, -s], [0, s, c]], f32)
    R = (Ry @ Rx).astype(f32)
    t = (R @ np.array([0, 0, r], f32)).astype(f32) + np.asarray(centre, f32)
    return np.concatenate([R, t.astype(f32)[:, None]], 1).astype(f32)


def box_centre(verts):
    v = np.asarray(verts, f32)
    return ((v.min(0) + v.max(0)) * f32(0.5)).astype(f32) if len(v) else np.zeros(3, f32)


def views(verts, which=STANDARD_VIEWS):
    c = box_centre(verts)
    return np.stack([pose(*v, centre=c) for v in which])


def ray_dirs(H, W, intr, c2w, pixels=None):
    """float32 [P,3] for the pixel indices `pixels` (all H W of them, row-major, by default)"""
    fx, fy, cx, cy = intr
    idx = np.arange(H * W, dtype=np.int64) if pixels is None else np.asarray(pixels, np.int64)
    px, py = (idx % W).astype(f32), (idx // W).astype(f32)
    r = np.asarray(c2w, f32)[:3, :3]
    with np.errstate(all="ignore"):
        a = ((px - cx) / fx).astype(f32)
        b = (-(py - cy) / fy).astype(f32)
        m = f32(-1.)
        return np.stack([(a * r[i, 0] + b * r[i, 1]) + m * r[i, 2] for i in range(3)], 1).astype(f32)


def face_ok(verts, faces):
    """bool [F]: every index in 0..V-1, no repeated index, every coordinate finite"""
    v = np.asarray(verts, f32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    if ok.any():
        fin = np.isfinite(v).all(1)
        ok[ok] = fin[f[ok]].all(1)
    return ok


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _edge(d, p, q):
    return (d[0] * (p[1] * q[2] - p[2] * q[1]) + d[1] * (p[2] * q[0] - p[0] * q[2])) + d[2] * (p[0] * q[1] - p[1] * q[0])


def hit_terms(tri, o, d):
    """tri = (p0, p1, p2) float32 [..,3] each, o float32 [3], d float32 [..,3], broadcastable -> U, V, W, det, t (float64), t_f (float32)"""
    o = np.asarray(o, f32).astype(f64)
    A, B, C = ([p[..., k].astype(f64) - o[k] for k in range(3)] for p in tri)
    dd = [d[..., k].astype(f64) for k in range(3)]
    with np.errstate(all="ignore"):
        U, V, W = _edge(dd, B, C), _edge(dd, C, A), _edge(dd, A, B)
        det = (U + V) + W
        t = ((U * _dot(A, dd) + V * _dot(B, dd)) + W * _dot(C, dd)) / det / _dot(dd, dd)
        tf = t.astype(f32)
    return U, V, W, det, t, tf


def hit_mask(U, V, W, det, tf, near, far, cull):
    with np.errstate(all="ignore"):
        inside = ((U >= 0) & (V >= 0) & (W >= 0)) | ((U <= 0) & (V <= 0) & (W <= 0))
        ok = (det != 0) & inside & np.isfinite(tf) & (tf > f32(near)) & (tf <= f32(far))
        if cull == 1:
            ok &= ~(det > 0)
        if cull == 2:
            ok &= ~(det < 0)
    return ok


def zbuffer(verts, faces, o, d, near=0., far=np.inf, cull=0, chunk=256):
    """every ray against every valid face -> (keys uint64 [P], stats): hits, ties (hits with a zero edge value) and per-ray front
    (det < 0) and back hit counts"""
    v = np.asarray(verts, f32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    P = len(d)
    keys = np.full(P, EMPTY, np.uint64)
    stats = dict(hits=0, ties=0, front=np.zeros(P, np.int64), back=np.zeros(P, np.int64))
    ids = np.nonzero(face_ok(v, f))[0]
    for s in range(0, len(ids), chunk):
        fid = ids[s:s + chunk]
        tri = [v[f[fid, k]][None, :, :] for k in range(3)]
        U, V, W, det, _, tf = hit_terms(tri, o, d[:, None, :])
        ok = hit_mask(U, V, W, det, tf, near, far, cull)
        stats["hits"] += int(ok.sum())
        stats["ties"] += int((ok & ((U == 0) | (V == 0) | (W == 0))).sum())
        stats["front"] += (ok & (det < 0)).sum(1)
        stats["back"] += (ok & (det > 0)).sum(1)
        k = (tf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | fid.astype(np.uint64)[None, :]
        keys = np.minimum(keys, np.where(ok, k, EMPTY).min(1))
    return keys, stats


# ---------------------------------------------------------------------------------------------------------------------- boxes
def view_boxes(r, fx, fy, H, W):
    r = np.asarray(r, f32).astype(f64)
    with np.errstate(all="ignore"):
        dev = 0.0
        for i in range(3):
            for j in range(3):
                e = ((r[0, i] * r[0, j] + r[1, i] * r[1, j]) + r[2, i] * r[2, j]) - (1.0 if i == j else 0.0)
                m = abs(e)
                if not m <= dev:
                    dev = m
        sx, sy = f64(fx) + f64(W), f64(fy) + f64(H)
        return bool(dev <= 2.0 ** -20 and fx > 0 and fy > 0 and sx * sx / f64(fx) <= 131072.0 and sy * sy / f64(fy) <= 131072.0)


def boxes(verts, faces, c2w, intr, H, W):
    """meshrender_box for every valid face of one view -> (cls int [F'] 0 skip / 1 projected / 2 image, pixels int64 [F'], box int64 [F',4])"""
    fx, fy, cx, cy = (f64(x) for x in intr)
    v = np.asarray(verts, f32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[face_ok(v, f)]
    c2w = np.asarray(c2w, f32)
    r, o = c2w[:3, :3].astype(f64), c2w[:3, 3].astype(f64)
    use = view_boxes(c2w[:3, :3], intr[0], intr[1], H, W)
    n = len(f)
    px, py = np.zeros((n, 3)), np.zeros((n, 3))
    front, behind = np.zeros((n, 3), bool), np.zeros((n, 3), bool)
    with np.errstate(all="ignore"):
        for k in range(3):
            q = [v[f[:, k], a].astype(f64) - o[a] for a in range(3)]
            xc = (r[0, 0] * q[0] + r[1, 0] * q[1]) + r[2, 0] * q[2]
            yc = (r[0, 1] * q[0] + r[1, 1] * q[1]) + r[2, 1] * q[2]
            zc = (r[0, 2] * q[0] + r[1, 2] * q[1]) + r[2, 2] * q[2]
            dz = -zc
            s = 2.0 ** -12 * ((np.abs(q[0]) + np.abs(q[1])) + np.abs(q[2]))
            front[:, k] = (dz > 0) & (dz >= s)
            behind[:, k] = (dz < 0) & (dz <= -s)
            px[:, k] = cx + fx * xc / dz
            py[:, k] = cy - fy * yc / dz
        skip = behind.all(1)
        allf = front.all(1)
        xlo, xhi, ylo, yhi = px.min(1), px.max(1), py.min(1), py.max(1)
        proj = use & allf & np.isfinite(xlo) & np.isfinite(xhi) & np.isfinite(ylo) & np.isfinite(yhi) & ~skip
        x0, x1 = np.floor(xlo) - 1.0, np.ceil(xhi) + 1.0
        y0, y1 = np.floor(ylo) - 1.0, np.ceil(yhi) + 1.0
        wm, hm = W - 1.0, H - 1.0
        bx0 = np.where(x0 < 0, 0.0, np.where(x0 > wm, wm + 1.0, x0))
        bx1 = np.where(x1 > wm, wm, np.where(x1 < 0, -1.0, x1))
        by0 = np.where(y0 < 0, 0.0, np.where(y0 > hm, hm + 1.0, y0))
        by1 = np.where(y1 > hm, hm, np.where(y1 < 0, -1.0, y1))
    box = np.stack([np.where(proj, bx0, 0), np.where(proj, bx1, wm), np.where(proj, by0, 0), np.where(proj, by1, hm)], 1)
    box = np.nan_to_num(box).astype(np.int64)
    pixels = np.where((box[:, 1] < box[:, 0]) | (box[:, 3] < box[:, 2]), 0, (box[:, 1] - box[:, 0] + 1) * (box[:, 3] - box[:, 2] + 1))
    cls = np.where(skip, 0, np.where(proj, 1, 2))
    return cls, np.where(skip, 0, pixels), box


# -------------------------------------------------------------------------------------------------------------------- shading
def _clip01(x):
    return np.where(x < 0, 0.0, np.where(x > 1, 1.0, x))


def shade(mode, U, V, W, det, col, nor, d):
    """col / nor: None or three float32 [M,3] arrays (the face's vertex rows); d float32 [M,3] -> float32 [M,3]"""
    with np.errstate(all="ignore"):
        b = [U / det, V / det, W / det]
        M = len(U)
        c = np.full((M, 3), 0.8)
        if col is not None:
            c = np.stack([_clip01((b[0] * col[0][:, k].astype(f64) + b[1] * col[1][:, k].astype(f64)) + b[2] * col[2][:, k].astype(f64)) for k in range(3)], 1)
        if mode == 0:
            return c.astype(f32)
        n = [(b[0] * nor[0][:, k].astype(f64) + b[1] * nor[1][:, k].astype(f64)) + b[2] * nor[2][:, k].astype(f64) for k in range(3)]
        ln = np.sqrt(_dot(n, n))
        nh = np.stack([n[k] / ln for k in range(3)], 1)
        nh[~np.isfinite(nh).all(1)] = 0.0
        if mode == 1:
            return (0.5 * nh + 0.5).astype(f32)
        dd = [d[:, k].astype(f64) for k in range(3)]
        dl = np.sqrt(_dot(dd, dd))
        dh = [dd[k] / dl for k in range(3)]
        w = np.abs(_dot([nh[:, k] for k in range(3)], dh))
        return (c * w[:, None]).astype(f32)


# --------------------------------------------------------------------------------------------------------------------- render
def render(verts, faces, H, W, intr, poses, near=0., far=np.inf, cull=0, shading=0, colors=None, normals=None, background=(0., 0., 0.),
           pixels=None, want_counts=True):
    """-> dict(face int32 [N,P], depth, disp, acc float32 [N,P], bary, rgb float32 [N,P,3], counts int64 [4], ties, front, back);
    P = H W (row-major), or len(pixels) when a list of pixel indices is given (then `counts` has no hit total: counts[3] = -1)."""
    v = np.asarray(verts, f32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    poses = np.asarray(poses, f32).reshape(-1, 3, 4)
    N = len(poses)
    P = H * W if pixels is None else len(pixels)
    out = dict(face=np.full((N, P), -1, np.int32), depth=np.zeros((N, P), f32), disp=np.zeros((N, P), f32), acc=np.zeros((N, P), f32),
               bary=np.zeros((N, P, 3), f32), rgb=np.empty((N, P, 3), f32), ties=0, front=np.zeros((N, P), np.int64), back=np.zeros((N, P), np.int64))
    out["rgb"][:] = np.asarray(background, f32)
    counts = np.zeros(4, np.int64)
    if N > 0 and len(f) > 0:
        counts[0] = int((~face_ok(v, f)).sum())
    for n in range(N):
        o = poses[n, :, 3]
        d = ray_dirs(H, W, intr, poses[n], pixels)
        keys, st = zbuffer(v, f, o, d, near, far, cull)
        counts[3] += st["hits"]
        out["ties"] += st["ties"]
        out["front"][n], out["back"][n] = st["front"], st["back"]
        if want_counts and len(f):
            cls, npx, _ = boxes(v, f, poses[n], intr, H, W)
            counts[1] += int((cls == 0).sum())
            counts[2] += int((npx > NARROW_PIXELS).sum())
        hit = np.nonzero(keys != EMPTY)[0]
        if len(hit) == 0:
            continue
        fid = (keys[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        tri = [v[f[fid, k]] for k in range(3)]
        U, V_, W_, det, _, tf = hit_terms(tri, o, d[hit])
        assert np.array_equal(tf.view(np.uint32).astype(np.uint64), keys[hit] >> np.uint64(32))
        with np.errstate(all="ignore"):
            out["face"][n, hit] = fid
            out["depth"][n, hit] = tf
            out["disp"][n, hit] = (1.0 / tf.astype(f64)).astype(f32)
            out["acc"][n, hit] = 1
            out["bary"][n, hit] = np.stack([U / det, V_ / det, W_ / det], 1).astype(f32)
        col = None if colors is None else [np.asarray(colors, f32)[f[fid, k]] for k in range(3)]
        nor = None if normals is None else [np.asarray(normals, f32)[f[fid, k]] for k in range(3)]
        out["rgb"][n, hit] = shade(shading, U, V_, W_, det, col, nor, d[hit])
    if pixels is not None:
        counts[3] = -1
    out["counts"] = counts
    return out


# -------------------------------------------------------------------------------------------------------------------- compare
def ordered_sum(x):
    """the written order: lane sums over elements l, l + 1024, .. from 0.0, then folded in halves"""
    x = np.asarray(x, f64).reshape(-1)
    rows = -(-len(x) // CMP_LANES)
    pad = np.zeros(rows * CMP_LANES)
    pad[:len(x)] = x
    s = np.zeros(CMP_LANES)
    for row in pad.reshape(rows, CMP_LANES):
        s = s + row
    w = CMP_LANES // 2
    while w >= 1:
        s = s[:w] + s[w:2 * w]
        w //= 2
    return float(s[0])


def compare(acc, depth=None, alpha=None, ref_depth=None):
    """acc, depth, ref_depth float32 [N,H,W]; alpha float32 (covered iff > 0.5) or uint8 (covered iff >= 128) [N,H,W]; without an alpha
    the reference covers where ref_depth > 0 -> (counts int64 [N,4], sums float64 [N,3])"""
    acc = np.asarray(acc, f32)
    N = acc.shape[0]
    m = acc.reshape(N, -1) > f32(0.5)
    if alpha is None:
        r = np.asarray(ref_depth, f32).reshape(N, -1) > 0
    else:
        a = np.asarray(alpha).reshape(N, -1)
        r = a >= 128 if a.dtype == np.uint8 else a.astype(f32) > f32(0.5)
    counts = np.stack([(m & r).sum(1), (m | r).sum(1), m.sum(1), r.sum(1)], 1).astype(np.int64)
    sums = np.zeros((N, 3))
    if depth is not None and ref_depth is not None:
        d = np.asarray(depth, f32).reshape(N, -1).astype(f64) - np.asarray(ref_depth, f32).reshape(N, -1).astype(f64)
        both = m & r
        for n in range(N):
            dn = np.where(both[n], d[n], 0.0)
            sums[n] = [ordered_sum(np.abs(dn)), ordered_sum(dn * dn), ordered_sum(both[n].astype(f64))]
    return counts, sums


# ------------------------------------------------------------------------------------------------------------------- fixtures
def special_meshes():
    """name -> (verts, faces, poses) of the single-face cases: a triangle over the whole image, one that straddles the camera plane, one
    behind the camera, and the identity-rotation camera at (0.1, -0.2, 2) they are seen from"""
    cam = np.array([[[1, 0, 0, 0.1], [0, 1, 0, -0.2], [0, 0, 1, 2.0]]], f32)
    tri = np.array([[0, 1, 2]], np.int32)
    return dict(
        whole_image=(np.array([[-9, -9, 0], [9, -9, 0], [0, 12, 0]], f32), tri, cam),
        straddles=(np.array([[-0.5, -0.4, 0], [0.6, -0.3, 0.5], [0.1, 0.3, 3.5]], f32), tri, cam),
        behind=(np.array([[-1, -1, 3], [1, -1, 3.5], [0, 1, 4]], f32), tri, cam),
    )


def square():
    """two triangles in the plane z = 0 and the camera at (0.1, -0.2, 2) with the identity rotation: depth is o_z = 2 wherever covered"""
    v = np.array([[-0.4, -0.3, 0], [0.5, -0.3, 0], [0.5, 0.45, 0], [-0.4, 0.45, 0]], f32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32), special_meshes()["behind"][2]


def cases():
    """name -> (verts, faces, poses [N,3,4]): the meshes every implementation is compared on, at W x H = 48 x 40, focal 60.  The closed
    fixtures and the open sphere are seen from the two standard views and the tie view; the single faces from the identity camera
    and the two standard views about the origin; then the faces that are never followed and the empty inputs."""
    import meshops_ref as R
    import meshfill_ref as Hf
    fx = R.fixtures()
    out = {}
    for name in ("sphere", "torus", "two_spheres"):
        v, f, _ = fx[name]
        out[name] = (v, f, views(v, STANDARD_VIEWS + (TIE_VIEW,)))
    v, f = Hf.cut_sphere()[:2]
    out["cut_sphere"] = (v, f, views(v, STANDARD_VIEWS + (TIE_VIEW,)))
    for name, (v, f, cam) in special_meshes().items():
        out[name] = (v, f, np.concatenate([cam, views(np.zeros((1, 3), f32))]))
    sv, sf, _ = fx["sphere"]
    p = out["sphere"][2]
    out["repeated_index"] = (sv, np.concatenate([sf[:300], [[5, 5, 9]], sf[300:]]).astype(np.int32), p)
    out["index_equal_V"] = (sv, np.concatenate([[[0, 1, len(sv)]], sf, [[-1, 2, 3]]]).astype(np.int32), p)
    nv = np.concatenate([sv, [[np.nan, 0, 0]], [[0, np.inf, 0]]]).astype(f32)
    out["nan_vertex"] = (nv, np.concatenate([sf, [[0, 1, len(sv)], [2, len(sv) + 1, 3]]]).astype(np.int32), p)
    out["no_vertices"] = (np.zeros((0, 3), f32), np.zeros((0, 3), np.int32), p)
    out["no_faces"] = (sv, np.zeros((0, 3), np.int32), p)
    out["no_views"] = (sv, sf, np.zeros((0, 3, 4), f32))
    return out


def vertex_colors(verts):
    """a smooth colour per vertex that leaves [0, 1] in places, so the clip is exercised"""
    v = np.nan_to_num(np.asarray(verts, f32), nan=0.0, posinf=0.0, neginf=0.0)
    return (f32(0.5) + f32(0.9) * v[:, ::-1]).astype(f32)
