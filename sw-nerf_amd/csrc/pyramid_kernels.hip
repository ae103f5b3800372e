// pyramid_kernels.hip - the Laplacian pyramid of multires_dnerf/pyramid.py on [N, H, W, C] fp32 NHWC frames, C in 1..4
// (DESIGN.md 6g).  Three entry points, one launch each on the caller's stream, no workspace, no atomics:
//   down        dst[N,H/2,W/2,C] = box2x2(blur_k(src)): the k x k cross-correlation with zero padding k/2 (F.conv2d,
//               groups = C) and the 2x2 mean that F.interpolate(scale_factor=0.5, bilinear, align_corners=False)
//               computes, fused - the blurred image is never stored.  One thread per output float: it gathers the
//               (k+1) x (k+1) input footprint of its channel into registers (a tap outside the image is zero) and forms
//               the four blurred pixels from it; the 4x re-read of every input float is served by the caches.
//   up_axpy     out[N,H,W,C] = base + alpha * up(coarse[N,h,w,C]): bilinear, align_corners=False, any (H, W); base may be
//               NULL.  A row is a flat run of C*W floats and the tensor a flat run of rows: a thread owns 4 consecutive
//               floats (one 16-byte load of base, one 16-byte store) when base and out are 16-byte aligned, else 1.
//               (h, w) == (H, W) is base + alpha * coarse with no interpolation arithmetic at all.
//   up_adjoint  g_coarse[N,h,w,C] = up^T(g_out[N,H,W,C]) as a gather: a coarse pixel sums, rows ascending and columns
//               ascending inside a row, the fine pixels whose i0 or i1 it is - the same fp32 source coordinate as up, so
//               the two are exact transposes - and is therefore bit-identical from run to run.
// The source coordinate, the four-tap blend and the gather of the transpose are pyramid_interp.h (shared with patch_kernels.hip).
// All element offsets are 64-bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/swnerf.h"
#include "host_util.h"
#include "pyramid_interp.h"

#define PY_THREADS 256
#define PY_MAX_BLOCKS (1 << 22)        // above this many blocks a kernel strides over its work
#define PY_MAX_SIDE (1 << 20)
#define PY_MAX_K 7

// ---- down ------------------------------------------------------------------------------------------------------------
template <int K, int C>
__global__ __launch_bounds__(PY_THREADS) void py_down_kernel(const float* __restrict__ src, int64_t n, int h, int w,
                                                             const float* __restrict__ wt, float* __restrict__ dst) {
    constexpr int R = K / 2, F = K + 1;
    const int ho = h >> 1, wo = w >> 1;
    const int rowlen = wo * C;
    const int64_t total = n * (int64_t)ho * rowlen;
    float wk[K * K];
#pragma unroll
    for (int q = 0; q < K * K; ++q) wk[q] = wt[q];
    for (int64_t e = (int64_t)blockIdx.x * PY_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * PY_THREADS) {
        const int64_t row = e / rowlen;
        const int f = (int)(e - row * rowlen);
        const int64_t img = row / ho;
        const int i = (int)(row - img * ho);
        const int j = f / C, c = f - j * C;
        const float* S = src + img * (int64_t)h * w * C + c;
        const int y0 = 2 * i - R, x0 = 2 * j - R;
        float v[F][F];
#pragma unroll
        for (int a = 0; a < F; ++a) {
            const int y = y0 + a;
            const bool yin = y >= 0 && y < h;
#pragma unroll
            for (int b = 0; b < F; ++b) {
                const int x = x0 + b;
                v[a][b] = (yin && x >= 0 && x < w) ? S[((int64_t)y * w + x) * C] : 0.f;
            }
        }
        float blur[2][2];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                float s = 0.f;
#pragma unroll
                for (int a = 0; a < K; ++a)
#pragma unroll
                    for (int b = 0; b < K; ++b) s += wk[a * K + b] * v[dy + a][dx + b];
                blur[dy][dx] = s;
            }
        // lambda = 0.5 on both axes: 0.5 * (0.5 * a + 0.5 * b) + 0.5 * (0.5 * c + 0.5 * d); the halvings are exact
        dst[e] = 0.5f * (0.5f * blur[0][0] + 0.5f * blur[0][1]) + 0.5f * (0.5f * blur[1][0] + 0.5f * blur[1][1]);
    }
}

// ---- up_axpy ---------------------------------------------------------------------------------------------------------
template <int C>
__device__ __forceinline__ float py_up_one(const float* __restrict__ coarse, int64_t img, int h, int w, const PyAxis& ay,
                                           int f, float sx) {
    const int x = f / C, c = f - x * C;
    return py_up_pixel<C>(coarse + img * (int64_t)h * w * C, w, ay, x, c, sx);
}

template <int C, int VEC, int SAME>
__global__ __launch_bounds__(PY_THREADS) void py_up_axpy_kernel(const float* __restrict__ coarse, int64_t n, int h, int w,
                                                                const float* base, float alpha, int H, int W, float* out) {
    const int rowlen = W * C;
    const int64_t total = n * (int64_t)H * rowlen;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    const int64_t nvec = (total + VEC - 1) / VEC;
    for (int64_t t = (int64_t)blockIdx.x * PY_THREADS + threadIdx.x; t < nvec; t += (int64_t)gridDim.x * PY_THREADS) {
        const int64_t e = t * VEC;
        float u[VEC], b[VEC];
        const bool whole = e + VEC <= total;
        if (SAME) {
            if (VEC == 4 && whole) {
                const float4 c4 = *reinterpret_cast<const float4*>(coarse + e);
                u[0] = c4.x; u[1 % VEC] = c4.y; u[2 % VEC] = c4.z; u[3 % VEC] = c4.w;
            } else {
#pragma unroll
                for (int q = 0; q < VEC; ++q) u[q] = e + q < total ? coarse[e + q] : 0.f;
            }
        } else {
            int64_t row = e / rowlen;
            int f = (int)(e - row * rowlen);
            int64_t img = row / H;
            int y = (int)(row - img * H);
            PyAxis ay = py_axis(y, sy, h);
#pragma unroll
            for (int q = 0; q < VEC; ++q) {
                u[q] = e + q < total ? py_up_one<C>(coarse, img, h, w, ay, f, sx) : 0.f;
                if (++f == rowlen) {                          // the run of VEC floats crosses into the next row
                    f = 0;
                    if (++y == H) { y = 0; ++img; }
                    ay = py_axis(y, sy, h);
                }
            }
        }
        if (base) {
            if (VEC == 4 && whole) {
                const float4 b4 = *reinterpret_cast<const float4*>(base + e);
                b[0] = b4.x; b[1 % VEC] = b4.y; b[2 % VEC] = b4.z; b[3 % VEC] = b4.w;
            } else {
#pragma unroll
                for (int q = 0; q < VEC; ++q) b[q] = e + q < total ? base[e + q] : 0.f;
            }
#pragma unroll
            for (int q = 0; q < VEC; ++q) u[q] = b[q] + alpha * u[q];
        } else {
#pragma unroll
            for (int q = 0; q < VEC; ++q) u[q] = alpha * u[q];
        }
        if (VEC == 4 && whole) {
            *reinterpret_cast<float4*>(out + e) = make_float4(u[0], u[1 % VEC], u[2 % VEC], u[3 % VEC]);
        } else {
#pragma unroll
            for (int q = 0; q < VEC; ++q)
                if (e + q < total) out[e + q] = u[q];
        }
    }
}

// ---- up_adjoint ------------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(PY_THREADS) void py_up_adjoint_kernel(const float* __restrict__ g_out, int64_t n, int H, int W,
                                                                   int h, int w, float* __restrict__ g_coarse) {
    const int rowlen = w * C;
    const int64_t total = n * (int64_t)h * rowlen;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    for (int64_t e = (int64_t)blockIdx.x * PY_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * PY_THREADS) {
        const int64_t row = e / rowlen;
        const int f = (int)(e - row * rowlen);
        const int64_t img = row / h;
        const int i = (int)(row - img * h);
        const int j = f / C, c = f - j * C;
        const float* G = g_out + img * (int64_t)H * W * C + c;
        g_coarse[e] = py_adjoint_pixel<C>(G, H, W, h, w, i, j, sy, sx);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------
static int py_check_image(const char* who, int64_t n, int64_t h, int64_t w, int c) {
    if (n < 0) return sw_fail(SWNERF_E_ARG, "%s: negative image count %lld", who, (long long)n);
    if (c < 1 || c > 4) return sw_fail(SWNERF_E_ARG, "%s: %d channels; 1..4 are built", who, c);
    if (h < 1 || w < 1 || h > PY_MAX_SIDE || w > PY_MAX_SIDE)
        return sw_fail(SWNERF_E_ARG, "%s: image size %lld x %lld outside 1..2^20", who, (long long)h, (long long)w);
    return 0;
}

static unsigned py_blocks(int64_t items) {
    const int64_t b = (items + PY_THREADS - 1) / PY_THREADS;
    return (unsigned)(b < 1 ? 1 : (b > PY_MAX_BLOCKS ? PY_MAX_BLOCKS : b));
}

template <int K>
static void py_launch_down(int c, unsigned blocks, hipStream_t st, const float* src, int64_t n, int h, int w, const float* wt,
                           float* dst) {
    switch (c) {
    case 1: hipLaunchKernelGGL((py_down_kernel<K, 1>), dim3(blocks), dim3(PY_THREADS), 0, st, src, n, h, w, wt, dst); break;
    case 2: hipLaunchKernelGGL((py_down_kernel<K, 2>), dim3(blocks), dim3(PY_THREADS), 0, st, src, n, h, w, wt, dst); break;
    case 3: hipLaunchKernelGGL((py_down_kernel<K, 3>), dim3(blocks), dim3(PY_THREADS), 0, st, src, n, h, w, wt, dst); break;
    default: hipLaunchKernelGGL((py_down_kernel<K, 4>), dim3(blocks), dim3(PY_THREADS), 0, st, src, n, h, w, wt, dst); break;
    }
}

extern "C" int swnerf_pyramid_down(const float* src, int64_t n, int64_t h, int64_t w, int c, const float* weights, int k,
                                   float* dst, void* stream) {
    int rc = py_check_image("pyramid_down", n, h, w, c);
    if (rc) return rc;
    if (k < 1 || k > PY_MAX_K || (k & 1) == 0) return sw_fail(SWNERF_E_ARG, "pyramid_down: kernel size %d; odd sizes up to %d are built", k, PY_MAX_K);
    if (h < 2 || w < 2) return sw_fail(SWNERF_E_ARG, "pyramid_down: a %lld x %lld image has no half-size level", (long long)h, (long long)w);
    if (n == 0) return 0;
    if (!src || !weights || !dst) return sw_fail(SWNERF_E_ARG, "pyramid_down: NULL pointer");
    if (((uintptr_t)src & 3) || ((uintptr_t)dst & 3) || ((uintptr_t)weights & 3)) return sw_fail(SWNERF_E_ARG, "pyramid_down: operands must be 4-byte aligned");
    const unsigned blocks = py_blocks(n * (h / 2) * (w / 2) * c);
    hipStream_t st = (hipStream_t)stream;
    switch (k) {
    case 1: py_launch_down<1>(c, blocks, st, src, n, (int)h, (int)w, weights, dst); break;
    case 3: py_launch_down<3>(c, blocks, st, src, n, (int)h, (int)w, weights, dst); break;
    case 5: py_launch_down<5>(c, blocks, st, src, n, (int)h, (int)w, weights, dst); break;
    default: py_launch_down<7>(c, blocks, st, src, n, (int)h, (int)w, weights, dst); break;
    }
    return sw_check(hipGetLastError(), "py_down launch");
}

template <int VEC, int SAME>
static void py_launch_up(int c, unsigned blocks, hipStream_t st, const float* coarse, int64_t n, int h, int w, const float* base,
                         float alpha, int H, int W, float* out) {
    switch (c) {
    case 1: hipLaunchKernelGGL((py_up_axpy_kernel<1, VEC, SAME>), dim3(blocks), dim3(PY_THREADS), 0, st, coarse, n, h, w, base, alpha, H, W, out); break;
    case 2: hipLaunchKernelGGL((py_up_axpy_kernel<2, VEC, SAME>), dim3(blocks), dim3(PY_THREADS), 0, st, coarse, n, h, w, base, alpha, H, W, out); break;
    case 3: hipLaunchKernelGGL((py_up_axpy_kernel<3, VEC, SAME>), dim3(blocks), dim3(PY_THREADS), 0, st, coarse, n, h, w, base, alpha, H, W, out); break;
    default: hipLaunchKernelGGL((py_up_axpy_kernel<4, VEC, SAME>), dim3(blocks), dim3(PY_THREADS), 0, st, coarse, n, h, w, base, alpha, H, W, out); break;
    }
}

extern "C" int swnerf_pyramid_up_axpy(const float* coarse, int64_t n, int64_t h, int64_t w, int c, const float* base, float alpha,
                                      int64_t H, int64_t W, float* out, void* stream) {
    int rc = py_check_image("pyramid_up_axpy", n, h, w, c);
    if (rc) return rc;
    rc = py_check_image("pyramid_up_axpy (output)", n, H, W, c);
    if (rc) return rc;
    if (n == 0) return 0;
    if (!coarse || !out) return sw_fail(SWNERF_E_ARG, "pyramid_up_axpy: NULL pointer");
    if (((uintptr_t)coarse & 3) || ((uintptr_t)out & 3) || ((uintptr_t)base & 3)) return sw_fail(SWNERF_E_ARG, "pyramid_up_axpy: operands must be 4-byte aligned");
    const bool same = h == H && w == W;
    const bool vec = !(((uintptr_t)out & 15) || ((uintptr_t)base & 15) || (same && ((uintptr_t)coarse & 15)));
    const int64_t total = n * H * W * c;
    const unsigned blocks = py_blocks(vec ? (total + 3) / 4 : total);
    hipStream_t st = (hipStream_t)stream;
    if (same) {
        if (vec) py_launch_up<4, 1>(c, blocks, st, coarse, n, (int)h, (int)w, base, alpha, (int)H, (int)W, out);
        else     py_launch_up<1, 1>(c, blocks, st, coarse, n, (int)h, (int)w, base, alpha, (int)H, (int)W, out);
    } else {
        if (vec) py_launch_up<4, 0>(c, blocks, st, coarse, n, (int)h, (int)w, base, alpha, (int)H, (int)W, out);
        else     py_launch_up<1, 0>(c, blocks, st, coarse, n, (int)h, (int)w, base, alpha, (int)H, (int)W, out);
    }
    return sw_check(hipGetLastError(), "py_up_axpy launch");
}

extern "C" int swnerf_pyramid_up_adjoint(const float* g_out, int64_t n, int64_t H, int64_t W, int c, int64_t h, int64_t w,
                                         float* g_coarse, void* stream) {
    int rc = py_check_image("pyramid_up_adjoint", n, H, W, c);
    if (rc) return rc;
    rc = py_check_image("pyramid_up_adjoint (coarse)", n, h, w, c);
    if (rc) return rc;
    if (n == 0) return 0;
    if (!g_out || !g_coarse) return sw_fail(SWNERF_E_ARG, "pyramid_up_adjoint: NULL pointer");
    if (((uintptr_t)g_out & 3) || ((uintptr_t)g_coarse & 3)) return sw_fail(SWNERF_E_ARG, "pyramid_up_adjoint: operands must be 4-byte aligned");
    const unsigned blocks = py_blocks(n * h * w * c);
    hipStream_t st = (hipStream_t)stream;
    switch (c) {
    case 1: hipLaunchKernelGGL((py_up_adjoint_kernel<1>), dim3(blocks), dim3(PY_THREADS), 0, st, g_out, n, (int)H, (int)W, (int)h, (int)w, g_coarse); break;
    case 2: hipLaunchKernelGGL((py_up_adjoint_kernel<2>), dim3(blocks), dim3(PY_THREADS), 0, st, g_out, n, (int)H, (int)W, (int)h, (int)w, g_coarse); break;
    case 3: hipLaunchKernelGGL((py_up_adjoint_kernel<3>), dim3(blocks), dim3(PY_THREADS), 0, st, g_out, n, (int)H, (int)W, (int)h, (int)w, g_coarse); break;
    default: hipLaunchKernelGGL((py_up_adjoint_kernel<4>), dim3(blocks), dim3(PY_THREADS), 0, st, g_out, n, (int)H, (int)W, (int)h, (int)w, g_coarse); break;
    }
    return sw_check(hipGetLastError(), "py_up_adjoint launch");
}
