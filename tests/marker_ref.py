"""Helpers of the marker tests: a synthetic renderer, a numpy replay of csrc/marker_kernels.hip and a synthetic scene.

Coordinates are the detector's: pixel (i, j) covers [j, j + 1) x [i, i + 1), its centre is (j + 0.5, i + 0.5).

The replay restates every stage (DESIGN.md 6k "Markers").  The integer stages - grey, the box-sum threshold, the labels, the
per-component reductions, the coarse corners and the rejection flags - are pure integer functions of the input, so the device
must give the same bits.  Refinement and decoding are written in float64 with the formulae of csrc/marker_math.h, which the
device evaluates in float32."""
import numpy as np

BLACK, WHITE, BACKGROUND = 25., 230., 128.
FLAG_BORDER, FLAG_ONE_SIDED, FLAG_SMALL_QUAD = 1, 2, 4
SIDE_POINTS, PROFILE_HALF, MIN_CONTRAST, MIN_LINE_POINTS, MERGE_DIST = 24, 8, 40., 8, 4.


# ---- renderer ----------------------------------------------------------------------------------------------------------
def square_to_quad(q):
    """3x3 H with H (u, v, 1) ~ the point of quad q [4,2] at (u, v) of the unit square, corners (0,0) (1,0) (1,1) (0,1)"""
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = np.asarray(q, np.float64)
    dx1, dx2, sx = x1 - x2, x3 - x2, x0 - x1 + x2 - x3
    dy1, dy2, sy = y1 - y2, y3 - y2, y0 - y1 + y2 - y3
    den = dx1 * dy2 - dy1 * dx2
    g, h = (sx * dy2 - sy * dx2) / den, (dx1 * sy - dy1 * sx) / den
    return np.array([[x1 - x0 + g * x1, x3 - x0 + h * x3, x0], [y1 - y0 + g * y1, y3 - y0 + h * y3, y0], [g, h, 1.]])


def marker_cells(bits, border_white=None):
    """6 x 6 cell values (1 = white): a black border round the 4 x 4 payload `bits`; border_white = (row, col) of one border
    cell to paint white (a marker that must be refused)"""
    cells = np.zeros((6, 6), np.int64)
    cells[1:5, 1:5] = np.asarray(bits).reshape(4, 4)
    if border_white is not None:
        cells[border_white] = 1
    return cells


def render_marker(H, W, quads, bits_list, noise=0., seed=0, ss=4, border_white=None, background=BACKGROUND):
    """uint8 [H, W]: each 6 x 6 marker with its one-cell white quiet zone warped so that its corners 0..3 (cell coordinates
    (0,0) (6,0) (6,6) (0,6)) land on quads[k], over a grey background; ss x ss samples per pixel; Gaussian noise of the given
    sigma from default_rng(seed)."""
    sub = (np.arange(ss) + 0.5) / ss
    full = np.full((H * ss, W * ss), float(background))
    for q, bits in zip(quads, bits_list):
        Hq = square_to_quad(q)
        outer = Hq @ np.array([[-1 / 6., 7 / 6., 7 / 6., -1 / 6.], [-1 / 6., -1 / 6., 7 / 6., 7 / 6.], [1., 1., 1., 1.]])
        outer = outer[:2] / outer[2]                                  # the quiet zone's corners: only its bounding box is visited
        j0, j1 = max(int(np.floor(outer[0].min())), 0), min(int(np.ceil(outer[0].max())) + 1, W)
        i0, i1 = max(int(np.floor(outer[1].min())), 0), min(int(np.ceil(outer[1].max())) + 1, H)
        if j0 >= j1 or i0 >= i1:
            continue
        xs = (np.arange(j0, j1)[:, None] + sub[None, :]).reshape(-1)
        ys = (np.arange(i0, i1)[:, None] + sub[None, :]).reshape(-1)
        X, Y = np.meshgrid(xs, ys)
        img = full[i0 * ss:i1 * ss, j0 * ss:j1 * ss]
        Hi = np.linalg.inv(Hq)
        w = Hi[2, 0] * X + Hi[2, 1] * Y + Hi[2, 2]
        u = 6. * (Hi[0, 0] * X + Hi[0, 1] * Y + Hi[0, 2]) / w
        v = 6. * (Hi[1, 0] * X + Hi[1, 1] * Y + Hi[1, 2]) / w
        inside = (w > 0) & (u >= -1) & (u < 7) & (v >= -1) & (v < 7)
        cu, cv = np.clip(np.floor(u), 0, 5).astype(np.int64), np.clip(np.floor(v), 0, 5).astype(np.int64)
        cell = marker_cells(bits, border_white)[cv, cu]
        quiet = (u < 0) | (u >= 6) | (v < 0) | (v >= 6)
        full[i0 * ss:i1 * ss, j0 * ss:j1 * ss] = np.where(inside, np.where(quiet | (cell == 1), WHITE, BLACK), img)
    img = full.reshape(H, ss, W, ss).mean(axis=(1, 3))
    if noise > 0:
        img = img + np.random.default_rng(seed).normal(0., noise, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def payload_of(bits):
    """the 16 bits row-major from corner 0, first cell in bit 15"""
    return int(sum(int(b) << (15 - k) for k, b in enumerate(np.asarray(bits).reshape(-1))))


def bits_of(payload):
    return np.array([(int(payload) >> (15 - k)) & 1 for k in range(16)], np.int64).reshape(4, 4)


def rotate_payload(payload, k):
    """the payload read from corner k of the marker whose payload from corner 0 is `payload`"""
    return payload_of(np.rot90(bits_of(payload), k))


def random_bits(rng):
    """a payload whose four rotations differ"""
    while True:
        bits = rng.integers(0, 2, (4, 4))
        if len({rotate_payload(payload_of(bits), k) for k in range(4)}) == 4:
            return bits


def fixture_frames(count=80, H=240, W=320, seed=2024, noise=2.):
    """The fixture set: `count` frames, one marker each of side 20..84 px, any rotation, every corner moved by at most 0.12 of
    the side, all four corners at least 12 px inside the frame.  -> frames uint8 [count, H, W], quads [count, 4, 2] (clockwise
    with y down, from the marker's corner 0), payloads [count]."""
    rng = np.random.default_rng(seed)
    frames, quads, payloads = [], [], []
    base = np.array([[-.5, -.5], [.5, -.5], [.5, .5], [-.5, .5]])
    for k in range(count):
        side = 20. + 64. * k / max(count - 1, 1)
        while True:
            ang = rng.uniform(0, 2 * np.pi)
            R = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
            jit = rng.uniform(-1, 1, (4, 2))
            jit *= (0.12 * side * rng.uniform(0, 1, (4, 1))) / np.maximum(np.linalg.norm(jit, axis=1, keepdims=True), 1e-9)
            q = (base * side) @ R.T + jit + np.array([rng.uniform(0, W), rng.uniform(0, H)])
            if q[:, 0].min() >= 12 and q[:, 0].max() <= W - 12 and q[:, 1].min() >= 12 and q[:, 1].max() <= H - 12:
                break
        bits = random_bits(rng)
        frames.append(render_marker(H, W, [q], [bits], noise=noise, seed=seed + 1 + k))
        quads.append(q)
        payloads.append(payload_of(bits))
    return np.stack(frames), np.stack(quads), np.array(payloads, np.int64)


# ---- replay: integer stages --------------------------------------------------------------------------------------------
def grey(frames):
    """uint8 [..., H, W, c] -> uint8 [..., H, W]"""
    f = np.asarray(frames)
    if f.shape[-1] == 1:
        return f[..., 0].copy()
    f = f.astype(np.int64)
    return ((4899 * f[..., 0] + 9617 * f[..., 1] + 1868 * f[..., 2] + 8192) >> 14).astype(np.uint8)


def dark_mask(g, r, C=7):
    """g uint8 [H, W] -> uint8 [H, W]: 1 where g * cnt < s - C * cnt over the (2 r + 1)^2 window clipped to the image"""
    H, W = g.shape
    S = np.zeros((H + 1, W + 1), np.int64)
    S[1:, 1:] = np.cumsum(np.cumsum(g.astype(np.int64), 0), 1)
    i0, i1 = np.maximum(np.arange(H) - r, 0), np.minimum(np.arange(H) + r + 1, H)
    j0, j1 = np.maximum(np.arange(W) - r, 0), np.minimum(np.arange(W) + r + 1, W)
    s = S[i1][:, j1] - S[i0][:, j1] - S[i1][:, j0] + S[i0][:, j0]
    cnt = (i1 - i0)[:, None] * (j1 - j0)[None, :]
    return (g.astype(np.int64) * cnt < s - C * cnt).astype(np.uint8)


def label(mask):
    """uint8 [H, W] -> int32 [H, W]: -1 on light pixels, else the smallest linear index of the pixel's 8-connected component.
    Union-find by hooking and pointer jumping on whole arrays."""
    H, W = mask.shape
    dark = mask.astype(bool)
    big = H * W
    L = np.where(dark, np.arange(H * W).reshape(H, W), big).astype(np.int64)
    flat_dark = np.flatnonzero(dark.reshape(-1))
    while True:
        P = np.full((H + 2, W + 2), big, np.int64)
        P[1:-1, 1:-1] = L
        m = L.copy()
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                m = np.minimum(m, P[dy:dy + H, dx:dx + W])
        m = np.where(dark, m, big).reshape(-1)
        Lf = L.reshape(-1).copy()
        before = Lf.copy()
        np.minimum.at(Lf, Lf[flat_dark], m[flat_dark])          # hook the roots
        Lf[flat_dark] = np.minimum(Lf[flat_dark], m[flat_dark])
        while True:                                             # pointer jumping
            nxt = Lf.copy()
            nxt[flat_dark] = Lf[Lf[flat_dark]]
            if np.array_equal(nxt, Lf):
                break
            Lf = nxt
        L = Lf.reshape(H, W)
        if np.array_equal(Lf, before):
            break
    return np.where(dark, L, -1).astype(np.int32)


def _key_argmax(value, idx):
    """the entry with the largest value, the smallest linear index among equals: the device's atomicMax on (value, ~index)"""
    best = value.max()
    return int(idx[value == best].min())


def candidates(labels, min_area=100):
    """-> int32 [m, 11]: label, area, flags, then the coarse corners x0 y0 .. x3 y3 (pixel indices) of every component of at
    least min_area pixels in ascending label order.  Flags: 1 touches the image border, 2 lies on one side of P1P2, 4 integer
    quad area below min_area.  Corners: P1 (farthest from the centroid), P4, P2 (farthest from P1), P3 - clockwise with y down."""
    H, W = labels.shape
    lab = labels.reshape(-1).astype(np.int64)
    idx = np.flatnonzero(lab >= 0)
    order = np.argsort(lab[idx], kind="stable")
    idx = idx[order]
    roots, start, area = np.unique(lab[idx], return_index=True, return_counts=True)
    out = []
    for root, s, a in zip(roots, start, area):
        if a < min_area:
            continue
        p = idx[s:s + a]
        y, x = p // W, p % W
        flags = FLAG_BORDER if (x.min() == 0 or y.min() == 0 or x.max() == W - 1 or y.max() == H - 1) else 0
        cx2, cy2 = (4 * int(x.sum()) + a) // (2 * a), (4 * int(y.sum()) + a) // (2 * a)
        p1 = _key_argmax((2 * x - cx2) ** 2 + (2 * y - cy2) ** 2, p)
        y1, x1 = divmod(p1, W)
        p2 = _key_argmax((x - x1) ** 2 + (y - y1) ** 2, p)
        y2, x2 = divmod(p2, W)
        cr = (x2 - x1) * (y - y1) - (y2 - y1) * (x - x1)
        x3 = y3 = x4 = y4 = 0
        cp = cn = 0
        if cr.max() > 0:
            cp = int(cr.max())
            y3, x3 = divmod(_key_argmax(cr, p), W)
        if cr.min() < 0:
            cn = int(-cr.min())
            y4, x4 = divmod(_key_argmax(-cr, p), W)
        if cp == 0 or cn == 0:
            flags |= FLAG_ONE_SIDED
        if cp + cn < 2 * min_area:
            flags |= FLAG_SMALL_QUAD
        out.append([root, a, flags, x1, y1, x4, y4, x2, y2, x3, y3])
    return np.array(out, np.int32).reshape(-1, 11)


# ---- replay: refinement and decoding (float64) -------------------------------------------------------------------------
def bilinear(g, x, y):
    H, W = g.shape
    fx, fy = min(max(x - 0.5, 0.), W - 1.), min(max(y - 0.5, 0.), H - 1.)
    x0, y0 = int(np.floor(fx)), int(np.floor(fy))
    x1, y1 = min(x0 + 1, W - 1), min(y0 + 1, H - 1)
    wx, wy = fx - x0, fy - y0
    top = float(g[y0, x0]) * (1. - wx) + float(g[y0, x1]) * wx
    bot = float(g[y1, x0]) * (1. - wx) + float(g[y1, x1]) * wx
    return top * (1. - wy) + bot * wy


def edge_crossing(g, px, py, nx, ny):
    """offset along the normal of the mid-level crossing nearest 0, or None when the profile's contrast is below 40"""
    prof = [bilinear(g, px + (0.5 * m - 4.) * nx, py + (0.5 * m - 4.) * ny) for m in range(2 * PROFILE_HALF + 1)]
    lo, hi = min(prof), max(prof)
    if hi - lo < MIN_CONTRAST:
        return None
    mid = 0.5 * (lo + hi)
    best = None
    for m in range(2 * PROFILE_HALF):
        v0, v1 = prof[m] - mid, prof[m + 1] - mid
        if (v0 < 0) != (v1 < 0):
            o = (0.5 * m - 4.) + 0.5 * v0 / (v0 - v1)
            if best is None or abs(o) < abs(best):
                best = o
    return best


def fit_line(pts):
    """total least squares -> (mean, unit direction)"""
    pts = np.asarray(pts, np.float64)
    mx, my = 0., 0.
    for x, y in pts:
        mx += x
        my += y
    mx, my = mx / len(pts), my / len(pts)
    sxx = sxy = syy = 0.
    for x, y in pts:
        sxx += (x - mx) * (x - mx)
        sxy += (x - mx) * (y - my)
        syy += (y - my) * (y - my)
    th = 0.5 * np.arctan2(2. * sxy, sxx - syy)
    return (mx, my), (np.cos(th), np.sin(th))


def refine(g, corners):
    """corners [4,2] pixel centres -> (refined [4,2] float64, payload) or None"""
    c = np.asarray(corners, np.float64)
    lines = []
    for k in range(4):
        a, b = c[k], c[(k + 1) % 4]
        d = b - a
        ln = float(np.hypot(d[0], d[1]))
        if ln < 1e-6:
            return None
        nx, ny = d[1] / ln, -d[0] / ln
        pts = []
        for i in range(SIDE_POINTS):
            t = 0.15 + 0.7 * i / (SIDE_POINTS - 1)
            px, py = a[0] + t * d[0], a[1] + t * d[1]
            o = edge_crossing(g, px, py, nx, ny)
            if o is not None:
                pts.append((px + o * nx, py + o * ny))
        if len(pts) < MIN_LINE_POINTS:
            return None
        lines.append(fit_line(pts))
    q = np.zeros((4, 2))
    for k in range(4):
        (m1, d1), (m2, d2) = lines[(k + 3) % 4], lines[k]
        det = d1[0] * d2[1] - d1[1] * d2[0]
        if abs(det) < 1e-6:
            return None
        s = ((m2[0] - m1[0]) * d2[1] - (m2[1] - m1[1]) * d2[0]) / det
        q[k] = (m1[0] + s * d1[0], m1[1] + s * d1[1])
    Hm = square_to_quad(q)
    if not np.all(np.isfinite(Hm)):
        return None
    vals = np.zeros((6, 6))
    for b in range(6):
        for a in range(6):
            u, v = (a + 0.5) / 6., (b + 0.5) / 6.
            w = Hm[2, 0] * u + Hm[2, 1] * v + 1.
            vals[b, a] = bilinear(g, (Hm[0, 0] * u + Hm[0, 1] * v + Hm[0, 2]) / w, (Hm[1, 0] * u + Hm[1, 1] * v + Hm[1, 2]) / w)
    lo, hi = vals.min(), vals.max()
    if not (hi - lo >= MIN_CONTRAST):
        return None
    white = vals >= 0.5 * (lo + hi)
    border = np.ones((6, 6), bool)
    border[1:5, 1:5] = False
    if white[border].any():
        return None
    return q, payload_of(white[1:5, 1:5].astype(np.int64))


def detect_radius(g, r, C=7, min_area=100):
    """one radius: -> (mask, labels, candidates, [(label, quad, payload)] of the survivors in label order)"""
    mask = dark_mask(g, r, C)
    labels = label(mask)
    cand = candidates(labels, min_area)
    found = []
    for row in cand:
        if row[2]:
            continue
        res = refine(g, row[3:].reshape(4, 2).astype(np.float64) + 0.5)
        if res is not None:
            found.append((int(row[0]), res[0], res[1]))
    return mask, labels, cand, found


def detect(frame, radii=(11, 41), C=7, min_area=100):
    """frame uint8 [H, W] or [H, W, c] -> [(quad [4,2] float64, payload)]: the survivors of the first radius in label order,
    then those of each later radius whose centre is farther than 4 px from every survivor of an earlier radius"""
    g = frame if frame.ndim == 2 else grey(frame)
    out, earlier = [], []
    for r in radii:
        found = detect_radius(g, r, C, min_area)[3]
        centres = [q.mean(0) for _, q, _ in found]
        for (_, q, p), c in zip(found, centres):
            if all(np.hypot(*(c - e)) > MERGE_DIST for e in earlier):
                out.append((q, p))
        earlier += centres
    return out


def match_rotation(quad, truth_quad):
    """k with quad[i] ~ truth_quad[(i + k) % 4]"""
    return int(np.argmin([np.abs(quad - np.roll(truth_quad, -k, axis=0)).max() for k in range(4)]))


# ---- scene -------------------------------------------------------------------------------------------------------------
def look_at(eye, target, up=(0., 0., 1.)):
    """camera-to-world [4,4] of the nerf convention: x right, y up, the camera looks down -z"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = eye - target
    z /= np.linalg.norm(z)
    x = np.cross(np.asarray(up, np.float64), z)
    x /= np.linalg.norm(x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, eye
    return T


def project_nerf(T, P, fx, fy, cx, cy):
    """world points [m,3] -> (u, v) in the coordinates of get_rays (pixel index j has u = j at its centre)"""
    pc = (np.asarray(P, np.float64) - T[:3, 3]) @ T[:3, :3]
    return np.stack([cx + fx * pc[:, 0] / -pc[:, 2], cy - fy * pc[:, 1] / -pc[:, 2]], 1)


def make_scene(n_views=8, H=240, W=320, edge=0.08, seed=7, noise=2.):
    """A planar marker of edge `edge` at a tilted pose and n_views nerf-convention cameras on a ring above it.
    -> dict(frames uint8 [n,H,W], poses [n,4,4], fx, fy, cx, cy, corners3d [4,3] (OpenCV order: clockwise seen from the front,
    from the top-left), uv [n,4,2] exact projections in get_rays coordinates, bits [4,4])"""
    rng = np.random.default_rng(seed)
    a, b = 0.35, -0.2
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    R = Ry @ Rx
    centre = np.array([0.03, -0.02, 0.05])
    local = 0.5 * edge * np.array([[-1, 1, 0], [1, 1, 0], [1, -1, 0], [-1, -1, 0]], np.float64)
    corners3d = local @ R.T + centre
    fx = fy = 420.
    cx, cy = W / 2., H / 2.
    bits = random_bits(rng)
    frames, poses, uvs = [], [], []
    for k in range(n_views):
        ang = 2 * np.pi * k / n_views + 0.2
        eye = centre + R @ np.array([0.32 * np.cos(ang), 0.32 * np.sin(ang), 0.45])
        T = look_at(eye, centre + R @ np.array([0.02 * np.cos(3 * ang), 0.02 * np.sin(2 * ang), 0.]), up=R[:, 1])
        uv = project_nerf(T, corners3d, fx, fy, cx, cy)
        frames.append(render_marker(H, W, [uv + 0.5], [bits], noise=noise, seed=seed + 100 + k))
        poses.append(T)
        uvs.append(uv)
    return dict(frames=np.stack(frames), poses=np.stack(poses), fx=fx, fy=fy, cx=cx, cy=cy, corners3d=corners3d,
                uv=np.stack(uvs), bits=bits, edge=edge)
