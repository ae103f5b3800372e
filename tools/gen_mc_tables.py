#!/usr/bin/env python3
"""Generate sw-nerf_amd/csrc/mc_tables.h, the marching-cubes case table, procedurally (no published table is copied).

Conventions (shared by the HIP kernels, tests/mc_numpy.py and this generator):
  corner c in 0..7 sits at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) along (x, y, z) = (i, j, k) from the cell's min corner;
  case bit c is set iff corner c is INSIDE (f > level, strict fp32; NaN is outside).
  edge e in 0..11 runs along axis a = e >> 2 from base corner offset: along a 0, along the lower other axis (e & 1), along the
  higher other axis ((e >> 1) & 1).  The vertex of edge e belongs to the grid point at that base corner (its owner).

Construction, per case:
  1. on each of the 6 cube faces, walk the 4 corners counter-clockwise around the face's OUTWARD normal.  Every maximal run of
     inside corners is entered through one crossing edge and left through another; it yields one segment entry -> exit.  An
     ambiguous face (inside corners on a diagonal) has two runs of one corner each: the inside corners are SEPARATED.  The rule
     reads nothing but the face's own corner signs, so the two cells sharing a face build the same segment (reversed).
  2. every crossing edge lies on two faces and is the head of one segment and the tail of another: chaining the segments gives
     closed, consistently oriented loops.
  3. each loop is fan-triangulated, from the first vertex (in loop order) whose fan keeps every diagonal off the cube faces: a
     diagonal between two vertices on one face could also be built by the neighbour across that face, and the surface would
     stop being a manifold there (a loop that crosses an ambiguous face twice).  With this walk direction the triangle
     (v0, v1, v2) has its geometric normal (v1 - v0) x (v2 - v0) pointing away from the inside corners - outward from the
     dense region.

`--check` regenerates the header in memory and fails when the committed file differs."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "sw-nerf_amd", "csrc", "mc_tables.h")


def corner(di, dj, dk):
    return di | (dj << 1) | (dk << 2)


def corner_off(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def edge_id(axis, base):
    """edge along `axis` starting at corner offset `base` (its coordinate along axis is 0)."""
    b, c = [x for x in range(3) if x != axis]
    return axis * 4 + base[b] + 2 * base[c]


def edge_corners(e):
    a = e >> 2
    b, c = [x for x in range(3) if x != a]
    off = [0, 0, 0]
    off[b], off[c] = e & 1, (e >> 1) & 1
    c0 = corner(*off)
    off[a] = 1
    return c0, corner(*off)


def faces():
    """6 faces as 4 corners, counter-clockwise around the outward normal."""
    out = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3                  # (a, b, c) right-handed: e_b x e_c = e_a
        for side in (0, 1):
            def cor(ub, uc):
                o = [0, 0, 0]
                o[a], o[b], o[c] = side, ub, uc
                return corner(*o)
            ring = [cor(0, 0), cor(1, 0), cor(1, 1), cor(0, 1)]   # CCW around +e_a
            out.append(ring if side == 1 else ring[::-1])         # the min face's outward normal is -e_a
    return out


def edge_between(c0, c1):
    o0, o1 = corner_off(c0), corner_off(c1)
    a = [x for x in range(3) if o0[x] != o1[x]]
    assert len(a) == 1
    base = tuple(min(o0[x], o1[x]) for x in range(3))
    return edge_id(a[0], base)


def face_segments(case, ring):
    """segments (entry edge, exit edge) of one face, walked counter-clockwise around its outward normal."""
    ins = [bool(case >> c & 1) for c in ring]
    segs = []
    for s in range(4):
        if ins[s] and not ins[s - 1]:                    # a run of inside corners starts at ring[s]
            entry = edge_between(ring[s - 1], ring[s])
            t = s
            while ins[(t + 1) % 4]:
                t += 1
            exit_ = edge_between(ring[t % 4], ring[(t + 1) % 4])
            segs.append((entry, exit_))
    return segs


def case_loops(case):
    nxt = {}
    for ring in faces():
        for a, b in face_segments(case, ring):
            assert a not in nxt, (case, "edge is the tail of two segments")
            nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values()), (case, "segments do not close")
    loops, seen = [], set()
    for e0 in sorted(nxt):
        if e0 in seen:
            continue
        loop, e = [], e0
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == e0
        loops.append(loop)
    return loops


def edge_faces(e):
    """the two cube faces (as sets of corners) an edge lies on"""
    a, b = edge_corners(e)
    return [i for i, ring in enumerate(faces()) if a in ring and b in ring]


def diagonal_ok(e0, e1):
    """a triangulation diagonal may not lie on a cube face: the neighbouring cell could build the same edge"""
    return not set(edge_faces(e0)) & set(edge_faces(e1))


def triangulate(poly):
    """triangles of polygon `poly` (orientation kept) whose diagonals all pass through the cell's interior; None if none
    exists.  Fans are tried first, from each start vertex in turn, then any triangulation."""
    n = len(poly)
    for s in range(n):
        p = poly[s:] + poly[:s]
        if all(diagonal_ok(p[0], p[i]) for i in range(2, n - 1)):
            return [(p[0], p[i], p[i + 1]) for i in range(1, n - 1)]

    def rec(p):
        if len(p) < 3:
            return []
        for k in range(1, len(p) - 1):
            if (k > 1 and not diagonal_ok(p[0], p[k])) or (k < len(p) - 2 and not diagonal_ok(p[k], p[-1])):
                continue
            left, right = rec(p[:k + 1]), rec(p[k:])
            if left is not None and right is not None:
                return left + [(p[0], p[k], p[-1])] + right
        return None
    return rec(poly)


def case_triangles(case):
    tris = []
    for loop in case_loops(case):
        t = triangulate(loop)
        assert t is not None, (case, loop, "no triangulation keeps its diagonals off the cube faces")
        tris += t
    return tris


def generate():
    tables = [case_triangles(c) for c in range(256)]
    max_t = max(len(t) for t in tables)
    lines = ["// mc_tables.h - marching-cubes case table.  GENERATED by tools/gen_mc_tables.py: do not edit; regenerate and run",
             "// `python tools/gen_mc_tables.py --check`.  Corner c sits at (c & 1, c >> 1 & 1, c >> 2 & 1) from the cell's min corner;",
             "// case bit c = corner c inside (f > level).  Edge e runs along axis e >> 2 from the corner offset (e & 1, e >> 1 & 1) in",
             "// the two other axes (ascending).  Ambiguous faces separate their inside corners; triangles wind outward from the",
             "// dense region.",
             "#pragma once",
             "#include <stdint.h>",
             "",
             "// a device translation unit defines SW_MC_TABLE_QUAL as `static __constant__ const` before including this header",
             "#ifndef SW_MC_TABLE_QUAL",
             "#define SW_MC_TABLE_QUAL static const",
             "#endif",
             "",
             f"#define SW_MC_MAX_TRIS {max_t}",
             "",
             "SW_MC_TABLE_QUAL int8_t sw_mc_ntri[256] = {"]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(t)) for t in tables[r:r + 32]) + ",")
    lines.append("};")
    lines.append("")
    lines.append(f"SW_MC_TABLE_QUAL int8_t sw_mc_tri[256][{3 * max_t}] = {{")
    for c, t in enumerate(tables):
        flat = [e for tri in t for e in tri] + [-1] * (3 * (max_t - len(t)))
        lines.append("    {" + ", ".join(str(e) for e in flat) + "},  // " + str(c))
    lines.append("};")
    return "\n".join(lines) + "\n", max_t


def main():
    text, max_t = generate()
    if "--check" in sys.argv:
        with open(OUT) as f:
            if f.read() != text:
                print(f"{OUT} differs from a fresh generation: run tools/gen_mc_tables.py", file=sys.stderr)
                return 1
        print(f"ok: {OUT} matches (max {max_t} triangles per case)")
        return 0
    with open(OUT, "w") as f:
        f.write(text)
    print(f"wrote {OUT}: max {max_t} triangles per case")
    return 0


if __name__ == "__main__":
    sys.exit(main())
