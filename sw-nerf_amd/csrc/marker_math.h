// marker_math.h - the arithmetic of the square-marker detector, written once for the device kernels (marker_kernels.hip) and for
// plain host C++ (g++ compiles this header).  DESIGN.md 6k "Markers" describes the stages; tests/marker_ref.py restates them in
// numpy.
// Pixel (i, j) covers [j, j + 1) x [i, i + 1); its centre is (j + 0.5, i + 0.5).  Every stage up to the coarse corners is integer
// arithmetic, so its result is a pure function of the input bytes; refinement and decoding are templated on the real type (the
// device uses float, built with -ffp-contract=off: one rounding per operation).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MARKER_HD __host__ __device__ __forceinline__
#else
#define MARKER_HD static inline
#endif

#define MARKER_MAX_RADIUS 64           // 255 * 129^2 fits int32, a row sum of 129 bytes fits uint16
#define MARKER_MAX_RADII 4
#define MARKER_MIN_AREA 16             // smallest min_area: bounds the components kept per frame by H W / 16
#define MARKER_MAX_SIDE 16384          // squared distances in half pixels stay below 2^31
#define MARKER_FLAG_BORDER 1           // the component touches the image border
#define MARKER_FLAG_ONE_SIDED 2        // no pixel on one side of the diagonal P1P2
#define MARKER_FLAG_SMALL_QUAD 4       // integer quad area below min_area
#define MARKER_SIDE_POINTS 24
#define MARKER_PROFILE 17              // offsets -4 .. 4 in steps of 0.5
#define MARKER_MIN_CONTRAST 40
#define MARKER_MIN_LINE_POINTS 8
#define MARKER_MERGE_DIST 4

// ---- integer stages ---------------------------------------------------------------------------------------------------
MARKER_HD int marker_luma(int r, int g, int b) { return (4899 * r + 9617 * g + 1868 * b + 8192) >> 14; }

// s: sum of the grey values over the window clipped to the image, cnt: its pixel count
MARKER_HD bool marker_dark(int g, int s, int cnt, int C) { return g * cnt < s - C * cnt; }

MARKER_HD int marker_window(int i, int r, int n) { return (i + r < n - 1 ? i + r : n - 1) - (i - r > 0 ? i - r : 0) + 1; }

// twice the centroid coordinate, rounded to the nearest integer: sum over area pixels
MARKER_HD int marker_centre2(int64_t sum, int64_t area) { return (int)((4 * sum + area) / (2 * area)); }

// atomicMax keys: the largest value wins, the smallest linear index among equal values.  value >= 1 for every real entry, so
// key 0 means "none".
MARKER_HD uint64_t marker_key(uint32_t value, uint32_t idx) { return ((uint64_t)value << 32) | (uint64_t)(0xFFFFFFFFu - idx); }
MARKER_HD uint32_t marker_key_index(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFu); }
MARKER_HD uint32_t marker_key_value(uint64_t key) { return (uint32_t)(key >> 32); }

// ---- refinement and decoding ------------------------------------------------------------------------------------------
// grey value at the continuous point (x, y): bilinear between pixel centres, clamped to the image.  No index leaves the image
// for any x, y (a NaN clamps to 0).
template <typename T>
MARKER_HD T marker_bilinear(const uint8_t* g, int H, int W, T x, T y) {
    T fx = x - (T)0.5, fy = y - (T)0.5;
    fx = fx > (T)0 ? fx : (T)0;
    fy = fy > (T)0 ? fy : (T)0;
    fx = fx < (T)(W - 1) ? fx : (T)(W - 1);
    fy = fy < (T)(H - 1) ? fy : (T)(H - 1);
    const int x0 = (int)fx, y0 = (int)fy;                      // fx, fy >= 0: truncation is floor
    const int x1 = x0 + 1 < W ? x0 + 1 : W - 1, y1 = y0 + 1 < H ? y0 + 1 : H - 1;
    const T wx = fx - (T)x0, wy = fy - (T)y0;
    const uint8_t* r0 = g + (int64_t)y0 * W;
    const uint8_t* r1 = g + (int64_t)y1 * W;
    const T top = (T)r0[x0] * ((T)1 - wx) + (T)r0[x1] * wx;
    const T bot = (T)r1[x0] * ((T)1 - wx) + (T)r1[x1] * wx;
    return top * ((T)1 - wy) + bot * wy;
}

// The grey profile through (px, py) along the unit normal (nx, ny) at offsets -4 .. 4 in steps of 0.5; *offset = the crossing of
// its mid level (min + max) / 2 nearest 0 (the first one on a tie).  false when the contrast is below MARKER_MIN_CONTRAST.
template <typename T>
MARKER_HD bool marker_edge_crossing(const uint8_t* g, int H, int W, T px, T py, T nx, T ny, T* offset) {
    T prof[MARKER_PROFILE];
    T lo = (T)1e30, hi = (T)-1e30;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int m = 0; m < MARKER_PROFILE; ++m) {
        const T o = (T)0.5 * (T)m - (T)4;
        prof[m] = marker_bilinear<T>(g, H, W, px + o * nx, py + o * ny);
        lo = prof[m] < lo ? prof[m] : lo;
        hi = prof[m] > hi ? prof[m] : hi;
    }
    if (hi - lo < (T)MARKER_MIN_CONTRAST) return false;
    const T mid = (T)0.5 * (lo + hi);
    bool have = false;
    T best = (T)0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int m = 0; m + 1 < MARKER_PROFILE; ++m) {
        const T v0 = prof[m] - mid, v1 = prof[m + 1] - mid;
        if ((v0 < (T)0) != (v1 < (T)0)) {
            const T o = ((T)0.5 * (T)m - (T)4) + (T)0.5 * v0 / (v0 - v1);
            if (!have || fabs(o) < fabs(best)) {
                best = o;
                have = true;
            }
        }
    }
    *offset = best;
    return have;
}

// Total-least-squares line through the valid ones of n points, summed in index order: line[0..1] = the mean, line[2..3] = the unit
// direction.  Returns the number of points used.
template <typename T>
MARKER_HD int marker_fit_line(const T* px, const T* py, const int* valid, int n, T* line) {
    int cnt = 0;
    T mx = (T)0, my = (T)0;
    for (int i = 0; i < n; ++i)
        if (valid[i]) {
            mx += px[i];
            my += py[i];
            ++cnt;
        }
    if (cnt == 0) return 0;
    mx = mx / (T)cnt;
    my = my / (T)cnt;
    T sxx = (T)0, sxy = (T)0, syy = (T)0;
    for (int i = 0; i < n; ++i)
        if (valid[i]) {
            const T dx = px[i] - mx, dy = py[i] - my;
            sxx += dx * dx;
            sxy += dx * dy;
            syy += dy * dy;
        }
    const T th = (T)0.5 * (T)atan2((T)2 * sxy, sxx - syy);
    line[0] = mx;
    line[1] = my;
    line[2] = (T)cos(th);
    line[3] = (T)sin(th);
    return cnt;
}

// the point where lines a and b (mean, direction) meet; false when they are parallel
template <typename T>
MARKER_HD bool marker_intersect(const T* a, const T* b, T* x, T* y) {
    const T det = a[2] * b[3] - a[3] * b[2];
    if (!(fabs(det) >= (T)1e-6)) return false;
    const T s = ((b[0] - a[0]) * b[3] - (b[1] - a[1]) * b[2]) / det;
    *x = a[0] + s * a[2];
    *y = a[1] + s * a[3];
    return true;
}

// h[8]: x = (h0 u + h1 v + h2) / (h6 u + h7 v + 1), y = (h3 u + h4 v + h5) / (same) takes the unit square's corners (0,0) (1,0)
// (1,1) (0,1) to q[0..3] (x, y pairs)
template <typename T>
MARKER_HD void marker_square_to_quad(const T* q, T* h) {
    const T dx1 = q[2] - q[4], dx2 = q[6] - q[4], sx = q[0] - q[2] + q[4] - q[6];
    const T dy1 = q[3] - q[5], dy2 = q[7] - q[5], sy = q[1] - q[3] + q[5] - q[7];
    const T den = dx1 * dy2 - dy1 * dx2;
    const T gg = (sx * dy2 - sy * dx2) / den, hh = (dx1 * sy - dy1 * sx) / den;
    h[0] = q[2] - q[0] + gg * q[2];
    h[1] = q[6] - q[0] + hh * q[6];
    h[2] = q[0];
    h[3] = q[3] - q[1] + gg * q[3];
    h[4] = q[7] - q[1] + hh * q[7];
    h[5] = q[1];
    h[6] = gg;
    h[7] = hh;
}

template <typename T>
MARKER_HD void marker_map(const T* h, T u, T v, T* x, T* y) {
    const T w = h[6] * u + h[7] * v + (T)1;
    *x = (h[0] * u + h[1] * v + h[2]) / w;
    *y = (h[3] * u + h[4] * v + h[5]) / w;
}

// Edge point pt = 24 side + i of the quad with corners (cx[k], cy[k]): the point at t = 0.15 + 0.7 i / 23 of side k -> k + 1, moved
// along the side's normal to the edge crossing.  false: a degenerate side or too little contrast.
template <typename T>
MARKER_HD bool marker_side_point(const uint8_t* g, int H, int W, const T* cx, const T* cy, int pt, T* x, T* y) {
    const int side = pt / MARKER_SIDE_POINTS, i = pt - side * MARKER_SIDE_POINTS;
    const T ax = cx[side], ay = cy[side], dx = cx[(side + 1) & 3] - ax, dy = cy[(side + 1) & 3] - ay;
    const T len = (T)sqrt(dx * dx + dy * dy);
    if (!(len >= (T)1e-6)) return false;
    const T nx = dy / len, ny = -dx / len;
    const T t = (T)0.15 + (T)0.7 * (T)i / (T)(MARKER_SIDE_POINTS - 1);
    const T bx = ax + t * dx, by = ay + t * dy;
    T o;
    if (!marker_edge_crossing<T>(g, H, W, bx, by, nx, ny, &o)) return false;
    *x = bx + o * nx;
    *y = by + o * ny;
    return true;
}

// centre of cell k = 6 row + column of the 6 x 6 grid, through the homography h
template <typename T>
MARKER_HD void marker_cell_point(const T* h, int k, T* x, T* y) {
    const int b = k / 6, a = k - 6 * b;
    marker_map<T>(h, ((T)a + (T)0.5) / (T)6, ((T)b + (T)0.5) / (T)6, x, y);
}

// the 36 sampled cells -> the payload (inner 4 x 4 row-major, first cell in bit 15, white = 1), or -1: contrast below
// MARKER_MIN_CONTRAST (a NaN among the cells ends here too) or a border cell that is not dark
template <typename T>
MARKER_HD int marker_decode(const T* cell) {
    T lo = cell[0], hi = cell[0];
    for (int k = 1; k < 36; ++k) {
        lo = cell[k] < lo ? cell[k] : lo;
        hi = cell[k] > hi ? cell[k] : hi;
    }
    if (!(hi - lo >= (T)MARKER_MIN_CONTRAST)) return -1;
    const T thr = (T)0.5 * (lo + hi);
    int payload = 0;
    for (int k = 0; k < 36; ++k) {
        const int b = k / 6, a = k - 6 * b;
        const bool white = cell[k] >= thr;
        if (a == 0 || a == 5 || b == 0 || b == 5) {
            if (white) return -1;
        } else if (white) {
            payload |= 1 << (15 - (4 * (b - 1) + (a - 1)));
        }
    }
    return payload;
}
