// meshrender_math.h - the per-ray, per-face and per-pixel arithmetic of the mesh renderer, written once for the device kernels
// (meshrender_kernels.hip) and for plain host C++ (g++ compiles this header; tests/meshrender_host_main.cpp).  DESIGN.md 6b "Mesh
// rendering" states the definitions and the argument for the pixel boxes; tests/meshrender_ref.py replays them in numpy.
// As in meshops_math.h everything is fp64 on float32 inputs, one rounding per operation (both builds use -ffp-contract=off) and a
// written order of additions, so every result is a pure function of the inputs: the same bits on the device, on the host and in
// the replay.  The one float32 part is the ray direction, which is get_rays' (ray_dir of ray_rows.h), instruction for instruction.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MESHRENDER_HD __host__ __device__ __forceinline__
#else
#define MESHRENDER_HD static inline
#endif

#define MESHRENDER_EMPTY 0xFFFFFFFFFFFFFFFFull     // a z-buffer word no hit has reached
#define MESHRENDER_NARROW_PIXELS 64                // a (face, view) pair whose box holds more pixels goes to the wave tier
#define MESHRENDER_CULL_NONE 0
#define MESHRENDER_CULL_BACK 1                     // drop det > 0
#define MESHRENDER_CULL_FRONT 2                    // drop det < 0
#define MESHRENDER_SHADE_COLORS 0
#define MESHRENDER_SHADE_NORMALS 1
#define MESHRENDER_SHADE_HEADLIGHT 2
#define MESHRENDER_BOX_SKIP 0                      // every vertex behind the camera plane: no ray of the view reaches the face
#define MESHRENDER_BOX_PROJECTED 1
#define MESHRENDER_BOX_IMAGE 2                     // the whole image (the hit rule works on rays: nothing is clipped)
#define MESHRENDER_ROT_TOL 9.5367431640625e-07     // 2^-20: the largest |R^T R - I| entry a view may have and still use projected boxes
#define MESHRENDER_FOV_LIMIT 131072.0              // 2^17 >= (f + side)^2 / f on both axes, likewise
#define MESHRENDER_DZ_GUARD 0.000244140625         // 2^-12: a vertex is in front / behind iff |dz| >= this times |p - o|_1

// float32, the instructions of ray_dir (ray_rows.h): a = (px - cx) / fx, b = -(py - cy) / fy, d = a r_0 + b r_1 - r_2 per row,
// products rounded, added left to right.  r = c2w[:3,:3] row-major.
MESHRENDER_HD void meshrender_ray_dir(float fx, float fy, float cx, float cy, const float r[9], float px, float py, float d[3]) {
    const float a = (px - cx) / fx, b = -(py - cy) / fy, m = -1.f;
    d[0] = a * r[0] + b * r[1] + m * r[2];
    d[1] = a * r[3] + b * r[4] + m * r[5];
    d[2] = a * r[6] + b * r[7] + m * r[8];
}

// E(p, q) = d . (p x q), added left to right.  E(q, p) = -E(p, q) exactly: every product commutes and a - b = -(b - a) in rounded
// arithmetic, so the two faces at an edge get opposite values for it whatever their vertex order.
MESHRENDER_HD double meshrender_edge(const double d[3], const double p[3], const double q[3]) {
    return (d[0] * (p[1] * q[2] - p[2] * q[1]) + d[1] * (p[2] * q[0] - p[0] * q[2])) + d[2] * (p[0] * q[1] - p[1] * q[0]);
}

MESHRENDER_HD double meshrender_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

struct MeshrenderHit { double U, V, W, det, t; float tf; };

// The ray o + t d against the face (p0, p1, p2).  true iff det != 0, U, V, W are all >= 0 or all <= 0, the facing passes `cull`,
// and t_f = (float)t is finite with near < t_f <= far.  h is filled whenever the function is called (the resolve pass reads it).
MESHRENDER_HD bool meshrender_hit(const float* p0, const float* p1, const float* p2, const float o[3], const float df[3], float near, float far,
                                  int cull, MeshrenderHit& h) {
    const double d[3] = {(double)df[0], (double)df[1], (double)df[2]};
    const double A[3] = {(double)p0[0] - (double)o[0], (double)p0[1] - (double)o[1], (double)p0[2] - (double)o[2]};
    const double B[3] = {(double)p1[0] - (double)o[0], (double)p1[1] - (double)o[1], (double)p1[2] - (double)o[2]};
    const double C[3] = {(double)p2[0] - (double)o[0], (double)p2[1] - (double)o[1], (double)p2[2] - (double)o[2]};
    h.U = meshrender_edge(d, B, C);
    h.V = meshrender_edge(d, C, A);
    h.W = meshrender_edge(d, A, B);
    h.det = (h.U + h.V) + h.W;
    h.t = ((h.U * meshrender_dot(A, d) + h.V * meshrender_dot(B, d)) + h.W * meshrender_dot(C, d)) / h.det / meshrender_dot(d, d);
    h.tf = (float)h.t;
    const bool inside = (h.U >= 0.0 && h.V >= 0.0 && h.W >= 0.0) || (h.U <= 0.0 && h.V <= 0.0 && h.W <= 0.0);
    if (!(h.det != 0.0) || !inside) return false;                 // a NaN fails `inside`
    if ((cull == MESHRENDER_CULL_BACK && h.det > 0.0) || (cull == MESHRENDER_CULL_FRONT && h.det < 0.0)) return false;
    return h.tf - h.tf == 0.f && h.tf > near && h.tf <= far;
}

// t_f > near >= 0: its bits order like the value, so an integer minimum of the words is the nearest hit, the smallest face id on
// equal depth bits
MESHRENDER_HD uint64_t meshrender_key(float tf, uint32_t face) {
    union { float f; uint32_t u; } b;
    b.f = tf;
    return ((uint64_t)b.u << 32) | (uint64_t)face;
}

// A face that is never followed: an index outside 0..V-1, a repeated index, a coordinate that is not finite
MESHRENDER_HD bool meshrender_face_ok(const float* verts, const int32_t* faces, int64_t f, int64_t V) {
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (a < 0 || b < 0 || c < 0 || (int64_t)a >= V || (int64_t)b >= V || (int64_t)c >= V || a == b || b == c || a == c) return false;
    const int32_t i[3] = {a, b, c};
    for (int k = 0; k < 3; ++k)
        for (int q = 0; q < 3; ++q) {
            const float x = verts[3 * (int64_t)i[k] + q];
            if (!(x - x == 0.f)) return false;
        }
    return true;
}

// May the faces of this view use projected boxes: the rotation is orthonormal to 2^-20 (a float32 rounding of an orthonormal
// matrix is within 2^-21), the focal lengths are positive and the field of view is bounded.  Anything else - a NaN among them -
// renders through whole-image boxes, which need no assumption.
MESHRENDER_HD bool meshrender_view_boxes(const float r[9], float fx, float fy, int H, int W) {
    double dev = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double e = (((double)r[i] * (double)r[j] + (double)r[3 + i] * (double)r[3 + j]) + (double)r[6 + i] * (double)r[6 + j]) - (i == j ? 1.0 : 0.0);
            const double m = fabs(e);
            if (!(m <= dev)) dev = m;                              // a NaN sticks
        }
    const double sx = (double)fx + (double)W, sy = (double)fy + (double)H;
    return dev <= MESHRENDER_ROT_TOL && fx > 0.f && fy > 0.f && sx * sx / (double)fx <= MESHRENDER_FOV_LIMIT && sy * sy / (double)fy <= MESHRENDER_FOV_LIMIT;
}

// The pixel box of a face in a view: box = {x0, x1, y0, y1}, inclusive, inside the image; x1 < x0 or y1 < y0 is an empty box.
// Per vertex q = p - o, camera coordinates through the transpose of the rotation, dz = -z_c, s = 2^-12 ((|q0| + |q1|) + |q2|);
// the vertex is behind iff dz < 0 and dz <= -s, in front iff dz > 0 and dz >= s.  All behind: SKIP.  `boxes` and all in front:
// px = cx + fx x_c / dz, py = cy - fy y_c / dz, the box is floor(min) - 1 .. ceil(max) + 1 clamped to the image.  Else the image.
MESHRENDER_HD int meshrender_box(const float* p0, const float* p1, const float* p2, const float o[3], const float r[9], float fx, float fy, float cx,
                                 float cy, int H, int W, bool boxes, int box[4]) {
    const float* p[3] = {p0, p1, p2};
    double xlo = 0.0, xhi = 0.0, ylo = 0.0, yhi = 0.0;
    int nfront = 0, nbehind = 0;
    for (int k = 0; k < 3; ++k) {
        const double q0 = (double)p[k][0] - (double)o[0], q1 = (double)p[k][1] - (double)o[1], q2 = (double)p[k][2] - (double)o[2];
        const double xc = ((double)r[0] * q0 + (double)r[3] * q1) + (double)r[6] * q2;
        const double yc = ((double)r[1] * q0 + (double)r[4] * q1) + (double)r[7] * q2;
        const double zc = ((double)r[2] * q0 + (double)r[5] * q1) + (double)r[8] * q2;
        const double dz = -zc, s = MESHRENDER_DZ_GUARD * ((fabs(q0) + fabs(q1)) + fabs(q2));
        const bool front = dz > 0.0 && dz >= s;
        nbehind += dz < 0.0 && dz <= -s;
        if (!front) continue;
        const double px = (double)cx + (double)fx * xc / dz, py = (double)cy - (double)fy * yc / dz;
        if (nfront == 0) { xlo = xhi = px; ylo = yhi = py; }
        else {
            xlo = px < xlo ? px : xlo; xhi = px > xhi ? px : xhi;
            ylo = py < ylo ? py : ylo; yhi = py > yhi ? py : yhi;
        }
        ++nfront;
    }
    if (nbehind == 3) return MESHRENDER_BOX_SKIP;
    box[0] = 0; box[1] = W - 1; box[2] = 0; box[3] = H - 1;
    if (!boxes || nfront != 3 || !(xlo - xlo == 0.0 && xhi - xhi == 0.0 && ylo - ylo == 0.0 && yhi - yhi == 0.0)) return MESHRENDER_BOX_IMAGE;
    const double x0 = floor(xlo) - 1.0, x1 = ceil(xhi) + 1.0, y0 = floor(ylo) - 1.0, y1 = ceil(yhi) + 1.0;
    const double wm = (double)(W - 1), hm = (double)(H - 1);
    // an end beyond the image on its own side leaves an empty box: -1 / W and -1 / H are exact in int
    box[0] = (int)(x0 < 0.0 ? 0.0 : (x0 > wm ? wm + 1.0 : x0));
    box[1] = (int)(x1 > wm ? wm : (x1 < 0.0 ? -1.0 : x1));
    box[2] = (int)(y0 < 0.0 ? 0.0 : (y0 > hm ? hm + 1.0 : y0));
    box[3] = (int)(y1 > hm ? hm : (y1 < 0.0 ? -1.0 : y1));
    return MESHRENDER_BOX_PROJECTED;
}

MESHRENDER_HD int64_t meshrender_box_pixels(const int box[4]) {
    return box[1] < box[0] || box[3] < box[2] ? 0 : (int64_t)(box[1] - box[0] + 1) * (int64_t)(box[3] - box[2] + 1);
}

MESHRENDER_HD double meshrender_clip01(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }

// The colour of a hit.  b = (U, V, W) / det in fp64.  c0..c2 / n0..n2: the face's vertex colours / normals (either may be NULL
// where the mode does not read it).
//   COLORS     clip01((b0 c0 + b1 c1) + b2 c2), rounded once
//   NORMALS    n = (b0 n0 + b1 n1) + b2 n2, nh = n / sqrt((nx nx + ny ny) + nz nz) (0 when that is not finite), 0.5 nh + 0.5
//   HEADLIGHT  the COLORS value before its rounding (0.8 without colours) times |nh . dh|, dh = d / sqrt(d . d)
MESHRENDER_HD void meshrender_shade(int mode, const MeshrenderHit& h, const float* c0, const float* c1, const float* c2, const float* n0,
                                    const float* n1, const float* n2, const float df[3], float rgb[3]) {
    const double b0 = h.U / h.det, b1 = h.V / h.det, b2 = h.W / h.det;
    double col[3] = {0.8, 0.8, 0.8}, nh[3] = {0.0, 0.0, 0.0};
    if (c0)
        for (int k = 0; k < 3; ++k) col[k] = meshrender_clip01((b0 * (double)c0[k] + b1 * (double)c1[k]) + b2 * (double)c2[k]);
    if (mode != MESHRENDER_SHADE_COLORS && n0) {
        double n[3];
        for (int k = 0; k < 3; ++k) n[k] = (b0 * (double)n0[k] + b1 * (double)n1[k]) + b2 * (double)n2[k];
        const double len = sqrt(meshrender_dot(n, n));
        const double x = n[0] / len, y = n[1] / len, z = n[2] / len;
        if (x - x == 0.0 && y - y == 0.0 && z - z == 0.0) { nh[0] = x; nh[1] = y; nh[2] = z; }
    }
    if (mode == MESHRENDER_SHADE_COLORS) {
        for (int k = 0; k < 3; ++k) rgb[k] = (float)col[k];
    } else if (mode == MESHRENDER_SHADE_NORMALS) {
        for (int k = 0; k < 3; ++k) rgb[k] = (float)(0.5 * nh[k] + 0.5);
    } else {
        const double d[3] = {(double)df[0], (double)df[1], (double)df[2]};
        const double dl = sqrt(meshrender_dot(d, d));
        const double dh[3] = {d[0] / dl, d[1] / dl, d[2] / dl};
        const double w = fabs(meshrender_dot(nh, dh));
        for (int k = 0; k < 3; ++k) rgb[k] = (float)(col[k] * w);
    }
}

// ---- view comparison: the written order of the fp64 sums -------------------------------------------------------------------
// One group of MESHRENDER_CMP_LANES lanes per view.  Lane l adds the terms of the pixels l, l + LANES, l + 2 LANES, ... in that order
// from 0.0; the lane sums are then folded in halves: for w = LANES / 2, LANES / 4, .., 1: s[l] += s[l + w] for l < w.  s[0] is the sum.
#define MESHRENDER_CMP_LANES 1024
