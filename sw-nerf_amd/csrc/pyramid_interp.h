// pyramid_interp.h - the bilinear upsample of the Laplacian pyramid (align_corners=False) and its transpose, written once: the
// image kernels of pyramid_kernels.hip and the patch loss of patch_kernels.hip are the same instructions.
// Source coordinate per axis, as torch forms it in fp32: s = max(scale * (d + 0.5) - 0.5, 0), scale = (float)n_in / n_out,
// i0 = (int)s, i1 = min(i0 + 1, n_in - 1), lambda = s - i0.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

struct PyAxis { int i0, i1; float l0, l1; };

__device__ __forceinline__ PyAxis py_axis(int d, float scale, int n_in) {
    float s = scale * ((float)d + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    PyAxis a;
    a.i0 = (int)s;
    if (a.i0 > n_in - 1) a.i0 = n_in - 1;                    // never taken for n_in <= 2^20 (s < n_in); keeps every index inside
    a.i1 = a.i0 + (a.i0 < n_in - 1 ? 1 : 0);
    a.l1 = s - (float)a.i0;
    a.l0 = 1.f - a.l1;
    return a;
}

// up at output row axis `ay`, output column x, channel c of ONE image P [h, w, C] (any address space)
template <int C>
__device__ __forceinline__ float py_up_pixel(const float* P, int w, const PyAxis& ay, int x, int c, float sx) {
    const PyAxis ax = py_axis(x, sx, w);
    const float* r0 = P + (int64_t)ay.i0 * w * C + c;
    const float* r1 = P + (int64_t)ay.i1 * w * C + c;
    const float top = ax.l0 * r0[(int64_t)ax.i0 * C] + ax.l1 * r0[(int64_t)ax.i1 * C];
    const float bot = ax.l0 * r1[(int64_t)ax.i0 * C] + ax.l1 * r1[(int64_t)ax.i1 * C];
    return ay.l0 * top + ay.l1 * bot;
}

// the fine indices d whose i0 or i1 can be coarse index i: s(d) in (i - 1, i + 1), widened by 2 against fp32 rounding of the
// estimate; every candidate is then tested with py_axis itself
__device__ __forceinline__ void py_range(int i, float scale, int n_out, int& lo, int& hi) {
    const float a = ((float)i - 0.5f) / scale - 0.5f, b = ((float)i + 1.5f) / scale - 0.5f;
    const float fl = floorf(a) - 2.f, fh = ceilf(b) + 2.f;
    lo = fl < 0.f ? 0 : (fl > (float)(n_out - 1) ? n_out - 1 : (int)fl);
    hi = fh < 0.f ? 0 : (fh > (float)(n_out - 1) ? n_out - 1 : (int)fh);
}

__device__ __forceinline__ float py_weight(const PyAxis& a, int i) {
    return (a.i0 == i ? a.l0 : 0.f) + (a.i1 == i ? a.l1 : 0.f);
}

// up^T at coarse pixel (i, j), channel c, of ONE fine image G [H, W, C] (G points at channel c of its first pixel): the fine pixels
// whose i0 or i1 it is, rows ascending and columns ascending inside a row
template <int C>
__device__ __forceinline__ float py_adjoint_pixel(const float* G, int H, int W, int h, int w, int i, int j, float sy, float sx) {
    int ylo, yhi, xlo, xhi;
    py_range(i, sy, H, ylo, yhi);
    py_range(j, sx, W, xlo, xhi);
    float acc = 0.f;
    for (int y = ylo; y <= yhi; ++y) {
        const float wy = py_weight(py_axis(y, sy, h), i);
        if (wy == 0.f) continue;
        const float* gr = G + (int64_t)y * W * C;
        float rs = 0.f;
        for (int x = xlo; x <= xhi; ++x) {
            const float wx = py_weight(py_axis(x, sx, w), j);
            if (wx != 0.f) rs += wx * gr[(int64_t)x * C];
        }
        acc += wy * rs;
    }
    return acc;
}
