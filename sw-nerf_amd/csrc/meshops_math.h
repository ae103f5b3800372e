// meshops_math.h - the per-vertex and per-face arithmetic of mesh clean-up and measurement, written once for the device kernels
// (meshops_kernels.hip) and for plain host C++ (g++ compiles this header; tests/meshops_host_main.cpp).  DESIGN.md 6b "Clean-up and
// measurement" states the definitions; tests/meshops_ref.py replays them in numpy.
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
