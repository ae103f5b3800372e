"""Numpy restatement of the hole-filling contract (swnerf_mesh_boundary / _boundary_loops / _fill_emit of include/swnerf.h, DESIGN.md
6b "Hole filling").  The GPU kernels and csrc/meshops_math.h are pinned against it; it never calls them.

  boundary   half-edge c = 3 f + k runs faces[f][k] -> faces[f][(k+1)%3]; it is a boundary half-edge iff tail != head and its
             undirected edge occurs exactly once over all faces (np.unique of the edge keys)
  next       the boundary half-edge leaving head(c), defined iff that head has exactly one leaving and one entering
  loops      a plain walk along next from every half-edge in ascending order: the walk that returns to its start is a loop and the
             start is its leader (the smallest id: every smaller one was visited before); the others are unfillable
  fill       n == 3: the face (p1, p0, p2); n >= 4: one new vertex and the faces (p_{r+1}, p_r, c); only loops of n <= max_edges
  vertex     fp64 sums of runs of 64 consecutive ranks, each added in rank order from 0.0, the run sums added in run order from 0.0,
             the total divided by n and rounded once to float32"""
import numpy as np

RUN = 64


def half_edges(faces):
    """-> (tail, head) int64 [3F] in half-edge id order"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)


def boundary(faces, V):
    """-> dict(bhe = boundary half-edge ids ascending, next = index into bhe or -1, tail, head)"""
    tail, head = half_edges(faces)
    if len(tail) == 0:
        z = np.zeros(0, np.int64)
        return dict(bhe=z, next=z, tail=z, head=z)
    lo, hi = np.minimum(tail, head), np.maximum(tail, head)
    _, inv, cnt = np.unique(lo * (V + 1) + hi, return_inverse=True, return_counts=True)
    bhe = np.nonzero((tail != head) & (cnt[inv] == 1))[0]
    t, h = tail[bhe], head[bhe]
    nout, nin = np.bincount(t, minlength=V), np.bincount(h, minlength=V)
    simple = (nout == 1) & (nin == 1)
    leaving = np.full(V, -1, np.int64)
    leaving[t[::-1]] = np.arange(len(bhe))[::-1]             # any one of them; it is read only where there is exactly one
    nxt = np.where(simple[h], leaving[h], -1)
    return dict(bhe=bhe, next=nxt, tail=t, head=h)


def self_edges(faces, V):
    """half-edges with tail == head whose edge {x, x} occurs once: measure() counts these among its boundary edges (it has no
    tail != head clause), hole filling does not - so measure().boundary_edges == boundary_edges + self_edges, and the two agree
    on every mesh without a face that repeats an index"""
    tail, head = half_edges(faces)
    x = tail[tail == head]
    return int((np.bincount(x, minlength=V) == 1).sum()) if len(x) else 0


def loops(faces, V):
    """-> dict(boundary_edges, table int64 [L,2] = (leader half-edge id, n) ascending, loop_offsets int64 [L+1], loop_vertices int64
    (p_0 .. p_{n-1} of every loop), unfillable_edges)"""
    b = boundary(faces, V)
    nxt, bhe, tail = b["next"].tolist(), b["bhe"], b["tail"]
    nb = len(nxt)
    seen = [False] * nb
    table, verts = [], []
    for s in range(nb):
        if seen[s]:
            continue
        path, i = [], s
        while i >= 0 and not seen[i]:
            seen[i] = True
            path.append(i)
            i = nxt[i]
        if i == s:                                           # back at the start: a cycle, and s is its smallest id
            table.append((int(bhe[s]), len(path)))
            verts.extend(path)
    table = np.array(table, np.int64).reshape(-1, 2)
    lv = tail[np.array(verts, np.int64)] if verts else np.zeros(0, np.int64)
    off = np.concatenate([[0], np.cumsum(table[:, 1])]).astype(np.int64)
    return dict(boundary_edges=nb, table=table, loop_offsets=off, loop_vertices=lv, unfillable_edges=nb - len(lv))


def blocked_means(A, loop_vertices, starts, lengths):
    """float32 [len(starts), 3]: the blocked fp64 mean of A[loop_vertices[s : s + n]] for every (s, n)"""
    A = np.asarray(A, np.float32)
    out = np.zeros((len(starts), 3), np.float32)
    if len(starts) == 0:
        return out
    nruns = (lengths + RUN - 1) // RUN
    run_loop = np.repeat(np.arange(len(starts)), nruns)
    first = np.concatenate([[0], np.cumsum(nruns)])
    run_k = np.arange(first[-1]) - first[run_loop]
    run_lo = starts[run_loop] + RUN * run_k
    run_n = np.minimum(RUN, lengths[run_loop] - RUN * run_k)
    part = np.zeros((first[-1], 3), np.float64)
    for q in range(RUN):
        on = run_n > q
        part[on] += A[loop_vertices[run_lo[on] + q]].astype(np.float64)
    for i in range(len(starts)):
        tot = np.cumsum(np.concatenate([np.zeros((1, 3)), part[first[i]:first[i + 1]]]), 0)[-1]      # cumsum adds in order
        out[i] = (tot / np.float64(lengths[i])).astype(np.float32)
    return out


def fill(verts, faces, colors=None, max_edges=None):
    """-> dict(verts, faces, colors or None, info) of the filled mesh, and the loops() fields"""
    P = np.asarray(verts, np.float32)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    V = len(P)
    lp = loops(f, V)
    n, off, lv = lp["table"][:, 1], lp["loop_offsets"], lp["loop_vertices"]
    on = np.ones(len(n), bool) if max_edges is None else n <= max_edges
    fan = on & (n >= 4)
    newv = V + np.cumsum(fan) - 1
    new_faces = []
    for i in np.nonzero(on)[0]:
        p = lv[off[i]:off[i + 1]]
        if n[i] == 3:
            new_faces.append(np.array([[p[1], p[0], p[2]]], np.int64))
        else:
            new_faces.append(np.stack([np.roll(p, -1), p, np.full(n[i], newv[i])], 1))
    add_f = np.concatenate(new_faces).astype(np.int32) if new_faces else np.zeros((0, 3), np.int32)
    add_v = blocked_means(P, lv, off[:-1][fan], n[fan])
    add_c = None if colors is None else blocked_means(colors, lv, off[:-1][fan], n[fan])
    info = dict(boundary_edges=lp["boundary_edges"], loops=len(n), filled_loops=int(on.sum()), filled_edges=int(n[on].sum()),
                skipped_loops=int((~on).sum()), unfillable_edges=lp["unfillable_edges"], new_vertices=int(fan.sum()), new_faces=len(add_f))
    out = dict(lp)
    out.update(verts=np.concatenate([P, add_v]), faces=np.concatenate([f, add_f]),
               colors=None if colors is None else np.concatenate([np.asarray(colors, np.float32), add_c]), info=info)
    return out


# ------------------------------------------------------------------------------------------------------------------ fixtures
def permuted(faces, seed):
    """the faces in a seeded random order, every face's corners rotated by a seeded amount (the same surface)"""
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    f = f[rng.permutation(len(f))]
    k = rng.integers(0, 3, len(f))
    return np.stack([f[np.arange(len(f)), (k + q) % 3] for q in range(3)], 1).astype(np.int32)


def cut_sphere():
    """the r = 0.6 sphere on the 24-point grid, cut by the box at z = x[13] -> (verts, faces, normals, analytic cap volume)"""
    import mc_numpy as M
    field, h = M.sphere(24)
    x = np.linspace(-1., 1., 24)
    v, f, n, _ = M.marching_cubes(field[:, :, :14], 0., (h, h, h), (-1., -1., -1.))
    hh = x[13] + 0.6
    return v, f, n, np.pi * hh * hh * (3 * 0.6 - hh) / 3


def corner_sphere():
    """a sphere centred (0.8, 0.8, 0.8), r = 0.7, on the 16-grid: cut by three box faces at a corner"""
    import mc_numpy as M
    (X, Y, Z), h = M.grid(16)
    field = (0.7 - np.sqrt((X - 0.8) ** 2 + (Y - 0.8) ** 2 + (Z - 0.8) ** 2)).astype(np.float32)
    v, f, n, _ = M.marching_cubes(field, 0., (h, h, h), (-1., -1., -1.))
    return v, f, n


def cut_torus():
    """torus(20) cut by the box at z = x[9]: two concentric loops, 56 and 24"""
    import mc_numpy as M
    field, h = M.torus(20)
    v, f, n, _ = M.marching_cubes(field[:, :, :10], 0., (h, h, h), (-1., -1., -1.))
    return v, f, n


def open_noise(shape=(10, 10, 10), seed=3):
    import mc_numpy as M
    v, f, n, _ = M.marching_cubes(M.noise(shape, seed=seed, pad=False), 0.3)
    return v, f, n


def pinched():
    """fan(12) and fan(10) shifted by (2, 0, 0) with the coincident ring vertex (1, 0, 0) merged, plus open_sphere shifted by
    (0, 5, 0): 74 boundary edges, one loop of 52, 22 unfillable"""
    import meshops_ref as R
    v1, f1 = R.fan(12)
    v2, f2 = R.fan(10)
    v2 = v2 + np.array([2, 0, 0], np.float32)
    j = 1 + 5                                                # fan(10)'s ring vertex at angle pi: (-1, 0, 0) + (2, 0, 0) = fan(12)'s ring vertex 1
    assert np.allclose(v2[j], v1[1], atol=1e-6)
    f2 = f2.astype(np.int64) + len(v1)
    f2[f2 == len(v1) + j] = 1
    sv, sf, _ = R.fixtures()["open_sphere"]
    v = np.concatenate([v1, v2, sv + np.array([0, 5, 0], np.float32)]).astype(np.float32)
    f = np.concatenate([f1.astype(np.int64), f2, sf.astype(np.int64) + len(v1) + len(v2)]).astype(np.int32)
    return v, f
