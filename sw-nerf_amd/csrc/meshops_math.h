// meshops_math.h - the per-vertex, per-face and per-cluster arithmetic of mesh clean-up, measurement, welding and decimation,
// written once for the device kernels (meshops_kernels.hip, meshsimp_kernels.hip, meshfill_kernels.hip) and for plain host C++ (g++ compiles this header;
// tests/meshops_host_main.cpp, tests/meshsimp_host_main.cpp, tests/meshfill_host_main.cpp).  DESIGN.md 6b "Clean-up and measurement",
// "Welding and decimation" and "Hole filling"
// state the definitions; tests/meshops_ref.py, tests/meshsimp_ref.py and tests/meshfill_ref.py replay them in numpy.
// Everything is fp64 on float32 inputs, one rounding per operation (both builds use -ffp-contract=off) and a fixed order of
// additions, so every result is a pure function of the inputs: the same bits on the device, on the host and in the replay.
// A corner id is c = 3 f + k: vertex k of face f.  An incidence slice lists the corners at one vertex in ascending order.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MESHOPS_HD __host__ __device__ __forceinline__
#else
#define MESHOPS_HD static inline
#endif

#define MESHOPS_FACE_TERMS 5           // area, volume, three first moments

MESHOPS_HD bool meshops_index_ok(int32_t i, int64_t n) { return i >= 0 && (int64_t)i < n; }

// cross(p1 - p0, p2 - p0) of float32 points widened to fp64
MESHOPS_HD void meshops_face_cross(const float* p0, const float* p1, const float* p2, double c[3]) {
    const double ux = (double)p1[0] - (double)p0[0], uy = (double)p1[1] - (double)p0[1], uz = (double)p1[2] - (double)p0[2];
    const double vx = (double)p2[0] - (double)p0[0], vy = (double)p2[1] - (double)p0[1], vz = (double)p2[2] - (double)p0[2];
    c[0] = uy * vz - uz * vy;
    c[1] = uz * vx - ux * vz;
    c[2] = ux * vy - uy * vx;
}

// t[0] = area, t[1] = signed volume about the stored origin, t[2..4] = volume term times the tetrahedron's centroid (p0 + p1 + p2) / 4
MESHOPS_HD void meshops_face_terms(const float* p0, const float* p1, const float* p2, double t[MESHOPS_FACE_TERMS]) {
    double c[3];
    meshops_face_cross(p0, p1, p2, c);
    t[0] = 0.5 * sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    const double ax = p0[0], ay = p0[1], az = p0[2], bx = p1[0], by = p1[1], bz = p1[2], cx = p2[0], cy = p2[1], cz = p2[2];
    const double kx = by * cz - bz * cy, ky = bz * cx - bx * cz, kz = bx * cy - by * cx;     // cross(p1, p2)
    const double vol = ((ax * kx + ay * ky) + az * kz) / 6.0;
    t[1] = vol;
    t[2] = vol * (((ax + bx) + cx) / 4.0);
    t[3] = vol * (((ay + by) + cy) / 4.0);
    t[4] = vol * (((az + bz) + cz) / 4.0);
}

// One umbrella step at vertex v (slice items[lo .. hi)): out = p + s (mean of the slice's neighbours - p).  A corner or a neighbour
// index outside the mesh is skipped, never dereferenced (the callers refuse such meshes before they get here).
MESHOPS_HD void meshops_smooth_vertex(const float* P, const int32_t* faces, const int32_t* items, int32_t lo, int32_t hi, int64_t v,
                                      int64_t V, int64_t F, float s, float out[3]) {
    const double px = P[3 * v], py = P[3 * v + 1], pz = P[3 * v + 2];
    double Sx = 0.0, Sy = 0.0, Sz = 0.0;
    int64_t n = 0;
    for (int32_t q = lo; q < hi; ++q) {
        const int32_t c = items[q];
        if (!meshops_index_ok(c, 3 * F)) continue;
        const int32_t f = c / 3, k = c - 3 * f;
        const int32_t a = faces[3 * f + (k + 1) % 3], b = faces[3 * f + (k + 2) % 3];
        if (!meshops_index_ok(a, V) || !meshops_index_ok(b, V)) continue;
        Sx += (double)P[3 * (int64_t)a];
        Sy += (double)P[3 * (int64_t)a + 1];
        Sz += (double)P[3 * (int64_t)a + 2];
        Sx += (double)P[3 * (int64_t)b];
        Sy += (double)P[3 * (int64_t)b + 1];
        Sz += (double)P[3 * (int64_t)b + 2];
        ++n;
    }
    if (n == 0) {
        out[0] = P[3 * v]; out[1] = P[3 * v + 1]; out[2] = P[3 * v + 2];
        return;
    }
    const double d = (double)(2 * n), sd = (double)s;
    out[0] = (float)(px + sd * (Sx / d - px));
    out[1] = (float)(py + sd * (Sy / d - py));
    out[2] = (float)(pz + sd * (Sz / d - pz));
}

// Area-weighted vertex normal: the slice's face crosses added in order, normalised in fp64; zero or non-finite -> (0, 0, 0)
MESHOPS_HD void meshops_vertex_normal(const float* P, const int32_t* faces, const int32_t* items, int32_t lo, int32_t hi, int64_t V,
                                      int64_t F, float out[3]) {
    double nx = 0.0, ny = 0.0, nz = 0.0;
    for (int32_t q = lo; q < hi; ++q) {
        const int32_t c = items[q];
        if (!meshops_index_ok(c, 3 * F)) continue;
        const int32_t f = c / 3;
        const int32_t a = faces[3 * f], b = faces[3 * f + 1], d = faces[3 * f + 2];
        if (!meshops_index_ok(a, V) || !meshops_index_ok(b, V) || !meshops_index_ok(d, V)) continue;
        double cr[3];
        meshops_face_cross(P + 3 * (int64_t)a, P + 3 * (int64_t)b, P + 3 * (int64_t)d, cr);
        nx += cr[0];
        ny += cr[1];
        nz += cr[2];
    }
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    const double rx = nx / len, ry = ny / len, rz = nz / len;
    const bool ok = len > 0.0 && isfinite(rx) && isfinite(ry) && isfinite(rz);
    out[0] = ok ? (float)rx : 0.f;
    out[1] = ok ? (float)ry : 0.f;
    out[2] = ok ? (float)rz : 0.f;
}

// ---- edges -------------------------------------------------------------------------------------------------------------
// The corner c = 3 f + k carries the directed edge faces[f][k] -> faces[f][(k+1)%3].  For the undirected edge {x, y}, scan x's
// slice: a corner there whose next vertex is y carries x -> y; one whose previous vertex is y means the corner before it (at y)
// carries y -> x.  An edge x == y (a face that repeats an index) has one direction only.
struct MeshopsEdge { int32_t n_xy, n_yx, first; };    // occurrences in each direction, the smallest carrying corner id

MESHOPS_HD MeshopsEdge meshops_edge_scan(const int32_t* faces, const int32_t* items, int32_t lo, int32_t hi, int32_t x, int32_t y,
                                         int64_t F) {
    MeshopsEdge e = {0, 0, INT32_MAX};
    for (int32_t q = lo; q < hi; ++q) {
        const int32_t c = items[q];
        if (!meshops_index_ok(c, 3 * F)) continue;
        const int32_t f = c / 3, k = c - 3 * f;
        if (faces[3 * f + (k + 1) % 3] == y) {
            ++e.n_xy;
            e.first = c < e.first ? c : e.first;
        }
        if (x != y && faces[3 * f + (k + 2) % 3] == y) {
            const int32_t cp = 3 * f + (k + 2) % 3;
            ++e.n_yx;
            e.first = cp < e.first ? cp : e.first;
        }
    }
    return e;
}

// ---- order-preserving float <-> uint32 keys: integer atomicMin / atomicMax on them give the exact float minimum / maximum -------
MESHOPS_HD uint32_t meshops_float_key(float x) {
    union { float f; uint32_t u; } b;
    b.f = x;
    return (b.u & 0x80000000u) ? ~b.u : (b.u | 0x80000000u);
}

MESHOPS_HD float meshops_key_float(uint32_t k) {
    union { float f; uint32_t u; } b;
    b.u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    return b.f;
}

// ---- vertex clustering: welding and decimation (DESIGN.md 6b "Welding and decimation"; tests/meshsimp_ref.py replays it) --------
// Only + - * / and floor in fp64, one rounding each; "finite" is x - x == 0.
#define MESHOPS_CELL_BITS 21
#define MESHOPS_CELL_LIMIT 2097152.0   // 2^21 cells an axis
#define MESHOPS_NO_CELL 0xFFFFFFFFFFFFFFFFull
#define MESHOPS_PLACE_WELD 0
#define MESHOPS_PLACE_MEAN 1
#define MESHOPS_PLACE_QUADRIC 2

MESHOPS_HD bool meshops_finite(double x) { return x - x == 0.0; }

// i_k = floor((p_k - o_k) / h) in fp64; the key i_x | i_y << 21 | i_z << 42, or MESHOPS_NO_CELL when an index is not in [0, 2^21)
// (a NaN or an infinity fails both comparisons).  idx (may be NULL) receives the three indices of a valid vertex.
MESHOPS_HD uint64_t meshops_cell_key(const float* p, const float* o, float h, double* idx) {
    uint64_t key = 0;
    for (int k = 0; k < 3; ++k) {
        const double t = floor(((double)p[k] - (double)o[k]) / (double)h);
        if (!(t >= 0.0 && t < MESHOPS_CELL_LIMIT)) return MESHOPS_NO_CELL;
        key |= (uint64_t)t << (MESHOPS_CELL_BITS * k);
        if (idx) idx[k] = t;
    }
    return key;
}

// the table slot a key starts probing at (splitmix64's finaliser); nothing but the probe sequence depends on it
MESHOPS_HD uint64_t meshops_key_hash(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// A face through the clustering: false when two labels agree (degenerate); else r = g rotated so that the smallest label leads
// (the orientation is kept: the reversed triple is another face).
MESHOPS_HD bool meshops_collapsed_face(const int32_t g[3], int32_t r[3]) {
    if (g[0] == g[1] || g[1] == g[2] || g[0] == g[2]) return false;
    const int s = (g[0] < g[1] && g[0] < g[2]) ? 0 : (g[1] < g[2] ? 1 : 2);
    r[0] = g[s]; r[1] = g[(s + 1) % 3]; r[2] = g[(s + 2) % 3];
    return true;
}

// Face f (labels gl[3 f ..], not degenerate) is a duplicate when an earlier face carries the same rotated triple.  Every such face
// has a corner in the slice items[lo .. hi) of any one of f's three labels; the answer does not depend on the slice's order.
MESHOPS_HD bool meshops_face_is_duplicate(const int32_t* gl, const int32_t* items, int32_t lo, int32_t hi, int32_t f, const int32_t r[3], int64_t F) {
    for (int32_t q = lo; q < hi; ++q) {
        const int32_t c = items[q];
        if (!meshops_index_ok(c, 3 * F)) continue;
        const int32_t e = c / 3;
        if (e >= f) continue;
        int32_t s[3];
        if (meshops_collapsed_face(gl + 3 * (int64_t)e, s) && s[0] == r[0] && s[1] == r[1] && s[2] == r[2]) return true;
    }
    return false;
}

// fp64 mean of the rows A[members[lo .. hi)] (ascending vertex ids), added in that order and divided by the count (hi > lo)
MESHOPS_HD void meshops_member_mean(const float* A, const int32_t* members, int32_t lo, int32_t hi, int64_t V, double m[3]) {
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int64_t n = 0;
    for (int32_t q = lo; q < hi; ++q) {
        const int32_t v = members[q];
        if (!meshops_index_ok(v, V)) continue;
        sx += (double)A[3 * (int64_t)v];
        sy += (double)A[3 * (int64_t)v + 1];
        sz += (double)A[3 * (int64_t)v + 2];
        ++n;
    }
    const double d = (double)n;
    m[0] = sx / d; m[1] = sy / d; m[2] = sz / d;
}

// Lindstrom's representative of one cluster.  items[lo .. hi) are the corners 3 f + k whose vertex carries the cluster's label,
// ascending, so a face's corners are adjacent: it is taken once, at its first corner.  Per face, n = cross(p1 - p0, p2 - p0)
// (unnormalised: the weight is area squared) and d = -((n0 p0x + n1 p0y) + n2 p0z); then, in this order,
//   Axx += n0 n0, Axy += n0 n1, Axz += n0 n2, Ayy += n1 n1, Ayz += n1 n2, Azz += n2 n2, bx += n0 d, by += n1 d, bz += n2 d.
// tr = (Axx + Ayy) + Azz; R = A + (eps tr) I; r = -(((A m)_k) + b_k) with (A m)_x = (Axx mx + Axy my) + Axz mz (and so on);
// y = adj(R) r / det(R) with the cofactors and the determinant exactly as written below; x = m + y.
// x = m when tr or det is not a finite positive number, an x_k is not finite, or x leaves the closed cell [lo_k, lo_k + h],
// lo_k = o_k + i_k h in fp64 (cell[k] = i_k).
MESHOPS_HD void meshops_quadric_point(const float* P, const int32_t* faces, const int32_t* items, int32_t lo, int32_t hi, int64_t V, int64_t F,
                                      const double m[3], const float* o, float h, const double cell[3], double eps, double x[3]) {
    double Axx = 0.0, Axy = 0.0, Axz = 0.0, Ayy = 0.0, Ayz = 0.0, Azz = 0.0, bx = 0.0, by = 0.0, bz = 0.0;
    int32_t last = -1;
    for (int32_t q = lo; q < hi; ++q) {
        const int32_t c = items[q];
        if (!meshops_index_ok(c, 3 * F)) continue;
        const int32_t f = c / 3;
        if (f == last) continue;
        last = f;
        const int32_t i0 = faces[3 * (int64_t)f], i1 = faces[3 * (int64_t)f + 1], i2 = faces[3 * (int64_t)f + 2];
        if (!meshops_index_ok(i0, V) || !meshops_index_ok(i1, V) || !meshops_index_ok(i2, V)) continue;
        const float* p0 = P + 3 * (int64_t)i0;
        double n[3];
        meshops_face_cross(p0, P + 3 * (int64_t)i1, P + 3 * (int64_t)i2, n);
        const double d = -((n[0] * (double)p0[0] + n[1] * (double)p0[1]) + n[2] * (double)p0[2]);
        Axx += n[0] * n[0]; Axy += n[0] * n[1]; Axz += n[0] * n[2];
        Ayy += n[1] * n[1]; Ayz += n[1] * n[2]; Azz += n[2] * n[2];
        bx += n[0] * d; by += n[1] * d; bz += n[2] * d;
    }
    x[0] = m[0]; x[1] = m[1]; x[2] = m[2];
    const double tr = (Axx + Ayy) + Azz;
    if (!(tr > 0.0 && meshops_finite(tr))) return;
    const double lam = eps * tr;
    const double Rxx = Axx + lam, Ryy = Ayy + lam, Rzz = Azz + lam, Rxy = Axy, Rxz = Axz, Ryz = Ayz;
    const double rx = -(((Axx * m[0] + Axy * m[1]) + Axz * m[2]) + bx);
    const double ry = -(((Axy * m[0] + Ayy * m[1]) + Ayz * m[2]) + by);
    const double rz = -(((Axz * m[0] + Ayz * m[1]) + Azz * m[2]) + bz);
    const double c00 = Ryy * Rzz - Ryz * Ryz, c01 = Rxz * Ryz - Rxy * Rzz, c02 = Rxy * Ryz - Rxz * Ryy;
    const double c11 = Rxx * Rzz - Rxz * Rxz, c12 = Rxy * Rxz - Rxx * Ryz, c22 = Rxx * Ryy - Rxy * Rxy;
    const double det = (Rxx * c00 + Rxy * c01) + Rxz * c02;
    if (!(det > 0.0 && meshops_finite(det))) return;
    const double y[3] = {((c00 * rx + c01 * ry) + c02 * rz) / det, ((c01 * rx + c11 * ry) + c12 * rz) / det, ((c02 * rx + c12 * ry) + c22 * rz) / det};
    double t[3];
    for (int k = 0; k < 3; ++k) {
        t[k] = m[k] + y[k];
        const double lo_k = (double)o[k] + cell[k] * (double)h, hi_k = lo_k + (double)h;
        if (!(meshops_finite(t[k]) && t[k] >= lo_k && t[k] <= hi_k)) return;
    }
    x[0] = t[0]; x[1] = t[1]; x[2] = t[2];
}

// One output vertex for label l (a valid vertex index whose cell is valid): WELD copies the rows of l; MEAN and QUADRIC place the
// position as above and average the colours; normals are copied by WELD only (the others recompute them on the new mesh).
// members / corners are the label's slices of the member list and of the corner list (corners are read by QUADRIC only).
MESHOPS_HD void meshops_place_vertex(int placement, const float* P, const float* colors, const int32_t* faces, const int32_t* members, int32_t mlo,
                                     int32_t mhi, const int32_t* corners, int32_t clo, int32_t chi, int64_t l, int64_t V, int64_t F, const float* o,
                                     float h, double eps, float pos[3], float col[3]) {
    if (placement == MESHOPS_PLACE_WELD) {
        for (int k = 0; k < 3; ++k) {
            pos[k] = P[3 * l + k];
            if (colors) col[k] = colors[3 * l + k];
        }
        return;
    }
    double m[3], x[3];
    meshops_member_mean(P, members, mlo, mhi, V, m);
    x[0] = m[0]; x[1] = m[1]; x[2] = m[2];
    if (placement == MESHOPS_PLACE_QUADRIC) {
        double cell[3];
        if (meshops_cell_key(P + 3 * l, o, h, cell) != MESHOPS_NO_CELL) meshops_quadric_point(P, faces, corners, clo, chi, V, F, m, o, h, cell, eps, x);
    }
    for (int k = 0; k < 3; ++k) pos[k] = (float)x[k];
    if (colors) {
        meshops_member_mean(colors, members, mlo, mhi, V, m);
        for (int k = 0; k < 3; ++k) col[k] = (float)m[k];
    }
}

// ---- hole filling (DESIGN.md 6b "Hole filling"; tests/meshfill_ref.py replays it) ------------------------------------------------
#define MESHOPS_FILL_RUN 64            // ranks per partial sum of a new vertex

// Is the half-edge c = 3 f + k (faces[f][k] -> faces[f][(k+1)%3]) a boundary half-edge: tail != head and its undirected edge occurs
// exactly once over all faces (measure's boundary edge).  The shorter of the two incidence slices is scanned.  false when an end
// point is outside 0..V-1: it is compared, never followed.
MESHOPS_HD bool meshops_boundary_halfedge(const int32_t* faces, const int32_t* offsets, const int32_t* items, int32_t c, int64_t V, int64_t F) {
    const int32_t f = c / 3, k = c - 3 * f;
    const int32_t a = faces[c], b = faces[3 * f + (k + 1) % 3];
    if (a == b || !meshops_index_ok(a, V) || !meshops_index_ok(b, V)) return false;
    const bool from_a = offsets[a + 1] - offsets[a] <= offsets[b + 1] - offsets[b];
    const int32_t x = from_a ? a : b, y = from_a ? b : a;
    const MeshopsEdge e = meshops_edge_scan(faces, items, offsets[x], offsets[x + 1], x, y, F);
    return e.n_xy + e.n_yx == 1;
}

// The new face of rank r of a loop p[0 .. n) (n >= 3): n == 3 has the single face (p1, p0, p2) at r == 0; n >= 4 has the fan faces
// (p[(r+1)%n], p[r], newv).  Each holds the reverse of a boundary half-edge, so the winding continues the surface.
MESHOPS_HD void meshops_fill_face(const int32_t* p, int32_t n, int32_t r, int32_t newv, int32_t out[3]) {
    out[0] = p[r + 1 < n ? r + 1 : 0];
    out[1] = p[r];
    out[2] = n == 3 ? p[2] : newv;
}

// fp64 sum of the rows A[p[lo .. hi)] added in that order from 0.0 (one run of a blocked mean); an index outside 0..V-1 is skipped
MESHOPS_HD void meshops_run_sum(const float* A, const int32_t* p, int32_t lo, int32_t hi, int64_t V, double s[3]) {
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int32_t q = lo; q < hi; ++q) {
        const int32_t v = p[q];
        if (!meshops_index_ok(v, V)) continue;
        sx += (double)A[3 * (int64_t)v];
        sy += (double)A[3 * (int64_t)v + 1];
        sz += (double)A[3 * (int64_t)v + 2];
    }
    s[0] = sx; s[1] = sy; s[2] = sz;
}

// The blocked mean of n rows from the sums of its ceil(n / 64) runs (part[3 q ..], run order): added in that order from 0.0, divided
// by n, rounded once to float32
MESHOPS_HD void meshops_blocked_mean(const double* part, int32_t nruns, int32_t n, float out[3]) {
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int32_t q = 0; q < nruns; ++q) {
        sx += part[3 * (int64_t)q];
        sy += part[3 * (int64_t)q + 1];
        sz += part[3 * (int64_t)q + 2];
    }
    const double d = (double)n;
    out[0] = (float)(sx / d); out[1] = (float)(sy / d); out[2] = (float)(sz / d);
}

// The slot of run k of loop li (its vertices start at offset off of the loop-ordered list) in a partial-sum array: strictly
// increasing over (li, k), below M / 64 + L + 1 for M listed vertices in L loops
MESHOPS_HD int64_t meshops_fill_slot(int64_t off, int64_t li, int64_t k) { return off / MESHOPS_FILL_RUN + li + k; }
