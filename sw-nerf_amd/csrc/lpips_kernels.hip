// lpips_kernels.hip - the three kernels of LPIPS (Learned Perceptual Image Patch Similarity, v0.1, AlexNet / VGG16 trunks;
// nerf/run.py:49-61 and d_nerf/metrics.ipynb build it from the `lpips` package), DESIGN.md 6f "LPIPS".  All activations are
// NHWC fp32, every element offset is 64-bit, no atomics, fixed summation orders: equal bits on every run.
//   conv2d   an implicit GEMM on v_mfma_f32_32x32x2_f32: M = N Ho Wo output pixels, K = k k Cin in (ky, kx, ci) order, N = Cout.
//            A 128 x (64 | 128) block of the output per workgroup of four waves, wave w the 64 x (32 | 64) part (w&1, w>>1) as
//            2 x (1 | 2) accumulator tiles.  K is walked in chunks of 32 through two LDS buffers: the next chunk is on its way from
//            global memory (registers) while this one feeds the matrix pipe, one barrier per chunk.  There is no im2col
//            buffer: the A tile is gathered from the input as it is staged - the (image, iy0, ix0) of the block's 128 pixels
//            sit in LDS, a chunk's k gives (ky, kx, ci), anything outside the image is a zero.  16-byte loads along Cin when
//            Cin % 4 == 0 (four consecutive k share a tap), 4-byte loads otherwise (Cin = 3: K = 27 or 363); the weights,
//            packed [K, Cout], by 16-byte loads when Cout % 4 == 0.  Operand tiles sit K-major in LDS ([k][row]): an MFMA operand
//            read is 32 consecutive floats, the pitches (129, Cout tile + 4) keep the staging writes conflict free.
//            An MFMA accumulates as a k-ordered fp32 fma chain, whose rounding error grows with its length; the chain is cut
//            every CV_FLUSH chunks (128 k): a segment accumulator is added to the running total and cleared, so the error at
//            K = 4608 is that of blocked summation, not of one 4608-long chain.
//   maxpool  window 2 or 3, stride 2, floor mode, no padding; NaN propagates as torch.max_pool2d does (a NaN replaces the
//            maximum and nothing replaces a NaN).  One thread per output pixel and 4 channels (16-byte accesses) when C % 4 == 0.
//   layer    one tap of LPIPS: per pixel sum_c lin_c (f0_c / (|f0| + 1e-10) - f1_c / (|f1| + 1e-10))^2 in fp32 by 16 lanes
//            (two passes over the pixel's channels, the second from cache), then the spatial mean in fp64: block partials in a
//            fixed order and one finishing pass, like the SSIM kernels.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/swnerf.h"
#include "host_util.h"

typedef float cv_f32x16 __attribute__((ext_vector_type(16)));
typedef float cv_f32x4 __attribute__((ext_vector_type(4)));

#define CV_BM 128                      // output pixels per workgroup
#define CV_KC 32                       // k per chunk
#define CV_PA 129                      // LDS pitch of the A tile ([k][pixel])
#define CV_FLUSH 4                     // chunks per accumulation segment
#define CV_MAX_SIDE (1 << 20)
#define CV_ROW_OUT (-(1 << 30))        // iy0 of a pixel row past M: every tap falls outside the image

struct CvArgs {
    const float* in; const float* w; const float* bias; float* out;
    int64_t M, HoWo;                   // N Ho Wo, Ho Wo
    int H, W, Cin, Cout, Wo, ksz, stride, pad, K, relu;
};

struct __attribute__((aligned(16))) CvRow { int64_t base; int iy0, ix0; };   // image offset, top-left tap of one output pixel

static inline size_t cv_lds_bytes(int bn) { return sizeof(CvRow) * CV_BM + 2 * CV_KC * (CV_PA + bn + 4) * sizeof(float); }

template <int TN, bool VECA, bool VECB>
__global__ void __launch_bounds__(256, 2) cv_conv_kernel(CvArgs P) {
    constexpr int BN = 64 * TN, PB = BN + 4, BUF = CV_KC * (CV_PA + PB);
    constexpr int NA = 16, NB = 8 * TN;                                      // staged floats per thread and chunk
    extern __shared__ __attribute__((aligned(16))) unsigned char cv_lds_raw[];
    CvRow* rows = reinterpret_cast<CvRow*>(cv_lds_raw);
    float* lds = reinterpret_cast<float*>(cv_lds_raw + sizeof(CvRow) * CV_BM);
    const int t = threadIdx.x, lane = t & 63, i = lane & 31, h = lane >> 5, wv = t >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * CV_BM;
    const int n0 = blockIdx.y * BN;
    const int wm = 64 * (wv & 1), wn = 32 * TN * (wv >> 1);
    if (t < CV_BM) {
        const int64_t m = m0 + t;
        CvRow r{0, CV_ROW_OUT, 0};
        if (m < P.M) {
            const int64_t n = m / P.HoWo, rem = m - n * P.HoWo;
            const int oy = (int)(rem / P.Wo), ox = (int)(rem - (int64_t)oy * P.Wo);
            r.base = n * P.H * P.W * P.Cin;
            r.iy0 = oy * P.stride - P.pad;
            r.ix0 = ox * P.stride - P.pad;
        }
        rows[t] = r;
    }
    __syncthreads();
    cv_f32x16 tot[2 * TN], seg[2 * TN];
#pragma unroll
    for (int k = 0; k < 2 * TN; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) { tot[k][r] = 0.f; seg[k][r] = 0.f; }
    float ra[NA], rb[NB];                                                    // the next chunk, on its way from global memory
    auto load = [&](int k0) {
        // A: the k of this thread is the same for all its rows, so (ky, kx, ci) is taken apart once per chunk
        const int k = k0 + (VECA ? 4 * (t & 7) : (t & 31));
        const unsigned tap = (unsigned)k / (unsigned)P.Cin;
        const int ci = k - (int)tap * P.Cin;
        const int ky = (int)(tap / (unsigned)P.ksz), kx = (int)tap - ky * P.ksz;
        const bool kin = k < P.K;
        if (VECA) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const CvRow r = rows[(t >> 3) + 32 * q];
                const int iy = r.iy0 + ky, ix = r.ix0 + kx;
                cv_f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (kin && (unsigned)iy < (unsigned)P.H && (unsigned)ix < (unsigned)P.W)      // Cin % 4 == 0: the 4 k share the tap
                    v = *reinterpret_cast<const cv_f32x4*>(P.in + r.base + ((int64_t)iy * P.W + ix) * P.Cin + ci);
                ra[4 * q] = v[0]; ra[4 * q + 1] = v[1]; ra[4 * q + 2] = v[2]; ra[4 * q + 3] = v[3];
            }
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const CvRow r = rows[(t >> 5) + 8 * q];
                const int iy = r.iy0 + ky, ix = r.ix0 + kx;
                ra[q] = (kin && (unsigned)iy < (unsigned)P.H && (unsigned)ix < (unsigned)P.W)
                            ? P.in[r.base + ((int64_t)iy * P.W + ix) * P.Cin + ci] : 0.f;
            }
        }
        if (VECB) {
            // thread -> (k = t / (BN/4) + (1024/BN) q, column 4 (t % (BN/4)) ..+3): BN/4 threads read one k row of the tile
#pragma unroll
            for (int q = 0; q < NB / 4; ++q) {
                const int kk = t / (BN / 4) + (1024 / BN) * q, col = 4 * (t % (BN / 4));
                cv_f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (k0 + kk < P.K && n0 + col < P.Cout)                                          // Cout % 4 == 0 on this path
                    v = *reinterpret_cast<const cv_f32x4*>(P.w + (int64_t)(k0 + kk) * P.Cout + n0 + col);
                rb[4 * q] = v[0]; rb[4 * q + 1] = v[1]; rb[4 * q + 2] = v[2]; rb[4 * q + 3] = v[3];
            }
        } else {
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const int e = t + 256 * q, kk = e / BN, col = e % BN;
                rb[q] = (k0 + kk < P.K && n0 + col < P.Cout) ? P.w[(int64_t)(k0 + kk) * P.Cout + n0 + col] : 0.f;
            }
        }
    };
    auto stage = [&](int buf) {
        float* As = lds + buf * BUF;
        float* Bs = As + CV_KC * CV_PA;
        if (VECA) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = (t >> 3) + 32 * q, kk = 4 * (t & 7);
#pragma unroll
                for (int e = 0; e < 4; ++e) As[(kk + e) * CV_PA + row] = ra[4 * q + e];
            }
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) As[(t & 31) * CV_PA + (t >> 5) + 8 * q] = ra[q];
        }
        if (VECB) {
#pragma unroll
            for (int q = 0; q < NB / 4; ++q) {
                const int kk = t / (BN / 4) + (1024 / BN) * q, col = 4 * (t % (BN / 4));
                const cv_f32x4 v = {rb[4 * q], rb[4 * q + 1], rb[4 * q + 2], rb[4 * q + 3]};
                *reinterpret_cast<cv_f32x4*>(Bs + kk * PB + col) = v;
            }
        } else {
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const int e = t + 256 * q;
                Bs[(e / BN) * PB + e % BN] = rb[q];
            }
        }
    };
    const int nch = (P.K + CV_KC - 1) / CV_KC;
    load(0);
    stage(0);
    __syncthreads();
#pragma nounroll
    for (int c = 0; c < nch; ++c) {
        if (c + 1 < nch) load((c + 1) * CV_KC);
        const float* As = lds + (c & 1) * BUF + wm + i;
        const float* Bs = lds + (c & 1) * BUF + CV_KC * CV_PA + wn + i;
#pragma unroll
        for (int s = 0; s < CV_KC / 2; ++s) {
            const float a0 = As[(2 * s + h) * CV_PA], a1 = As[(2 * s + h) * CV_PA + 32];
            const float b0 = Bs[(2 * s + h) * PB];
            seg[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, seg[0], 0, 0, 0);
            seg[TN] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, seg[TN], 0, 0, 0);
            if (TN == 2) {
                const float b1 = Bs[(2 * s + h) * PB + 32];
                seg[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, seg[1], 0, 0, 0);
                seg[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, seg[3], 0, 0, 0);
            }
        }
        if ((c & (CV_FLUSH - 1)) == CV_FLUSH - 1) {
#pragma unroll
            for (int k = 0; k < 2 * TN; ++k)
#pragma unroll
                for (int r = 0; r < 16; ++r) { tot[k][r] += seg[k][r]; seg[k][r] = 0.f; }
        }
        if (c + 1 < nch) stage((c + 1) & 1);                                 // the buffer nobody reads in this iteration
        __syncthreads();
    }
    // C/D map: register r of lane (i, h) of tile (x, y) is pixel wm + 32 x + (r&3) + 8 (r>>2) + 4 h, channel wn + 32 y + i
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < TN; ++y) {
            const int n = n0 + wn + 32 * y + i;
            if (n >= P.Cout) continue;
            const float bv = P.bias ? P.bias[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t m = m0 + wm + 32 * x + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (m < P.M) {
                    float v = (tot[x * TN + y][r] + seg[x * TN + y][r]) + bv;
                    if (P.relu) v = v < 0.f ? 0.f : v;                       // a NaN stays a NaN, as torch.relu keeps it
                    P.out[m * P.Cout + n] = v;
                }
            }
        }
}

// torch's [Cout, Cin, k, k] -> the [K, Cout] stream of the kernel, K in (ky, kx, ci) order
__global__ void __launch_bounds__(256) cv_pack_kernel(const float* __restrict__ w, int cout, int cin, int ksz, float* __restrict__ packed) {
    const int64_t total = (int64_t)ksz * ksz * cin * cout;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int co = (int)(e % cout);
        const int64_t k = e / cout;
        const int ci = (int)(k % cin), tap = (int)(k / cin);
        packed[e] = w[((int64_t)co * cin + ci) * ksz * ksz + tap];
    }
}

static int cv_shape(const char* what, int cin, int cout, int ksz) {
    if (ksz < 1 || ksz > 11) return sw_fail(SWNERF_E_ARG, "%s: kernel size %d outside 1..11", what, ksz);
    if (cin < 1 || cin > (1 << 20) || cout < 1 || cout > (1 << 20))
        return sw_fail(SWNERF_E_ARG, "%s: channel counts %d -> %d outside 1..2^20", what, cin, cout);
    return 0;
}

extern "C" int swnerf_conv2d_pack(const float* weight, int cout, int cin, int ksz, float* packed, void* stream) {
    int rc = cv_shape("conv2d_pack", cin, cout, ksz);
    if (rc) return rc;
    if (!weight || !packed) return sw_fail(SWNERF_E_ARG, "conv2d_pack: NULL pointer");
    const int64_t total = (int64_t)ksz * ksz * cin * cout;
    const unsigned gb = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(cv_pack_kernel, dim3(gb), dim3(256), 0, (hipStream_t)stream, weight, cout, cin, ksz, packed);
    return sw_check(hipGetLastError(), "conv2d_pack launch");
}

template <int TN>
static void cv_launch(const CvArgs& P, bool veca, bool vecb, dim3 grid, hipStream_t st) {
    const size_t lds = cv_lds_bytes(64 * TN);
    if (veca && vecb) hipLaunchKernelGGL((cv_conv_kernel<TN, true, true>), grid, dim3(256), lds, st, P);
    else if (veca) hipLaunchKernelGGL((cv_conv_kernel<TN, true, false>), grid, dim3(256), lds, st, P);
    else if (vecb) hipLaunchKernelGGL((cv_conv_kernel<TN, false, true>), grid, dim3(256), lds, st, P);
    else hipLaunchKernelGGL((cv_conv_kernel<TN, false, false>), grid, dim3(256), lds, st, P);
}

extern "C" int swnerf_conv2d_nhwc(const float* in, int64_t n, int64_t h, int64_t w, int cin, const float* packed,
                                  const float* bias, int cout, int ksz, int stride, int pad, int act, float* out, void* stream) {
    int rc = cv_shape("conv2d_nhwc", cin, cout, ksz);
    if (rc) return rc;
    if (stride < 1 || stride > 4) return sw_fail(SWNERF_E_ARG, "conv2d_nhwc: stride %d outside 1..4", stride);
    if (pad < 0 || pad > 5) return sw_fail(SWNERF_E_ARG, "conv2d_nhwc: padding %d outside 0..5", pad);
    if (act != SWNERF_ACT_NONE && act != SWNERF_ACT_RELU) return sw_fail(SWNERF_E_ARG, "conv2d_nhwc: activation %d is neither none nor ReLU", act);
    if (n < 0) return sw_fail(SWNERF_E_ARG, "conv2d_nhwc: negative image count %lld", (long long)n);
    if (h < 1 || w < 1 || h > CV_MAX_SIDE || w > CV_MAX_SIDE) return sw_fail(SWNERF_E_ARG, "conv2d_nhwc: image side outside 1..2^20");
    if (h + 2 * pad < ksz || w + 2 * pad < ksz)
        return sw_fail(SWNERF_E_ARG, "conv2d_nhwc: a %lld x %lld image with padding %d has no %d x %d window", (long long)h, (long long)w, pad, ksz, ksz);
    if (n == 0) return 0;
    if (!in || !packed || !out) return sw_fail(SWNERF_E_ARG, "conv2d_nhwc: NULL pointer");
    if (((uintptr_t)in | (uintptr_t)packed | (uintptr_t)bias | (uintptr_t)out) & 3) return sw_fail(SWNERF_E_ARG, "conv2d_nhwc: operands must be 4-byte aligned");
    const int64_t ho = (h + 2 * pad - ksz) / stride + 1, wo = (w + 2 * pad - ksz) / stride + 1;
    CvArgs P{};
    P.in = in; P.w = packed; P.bias = bias; P.out = out;
    P.HoWo = ho * wo; P.M = n * P.HoWo;
    P.H = (int)h; P.W = (int)w; P.Cin = cin; P.Cout = cout; P.Wo = (int)wo; P.ksz = ksz; P.stride = stride; P.pad = pad;
    P.K = ksz * ksz * cin; P.relu = act == SWNERF_ACT_RELU;
    const int bn = cout > 64 ? 128 : 64;
    const int64_t gx = (P.M + CV_BM - 1) / CV_BM, gy = (cout + bn - 1) / bn;
    if (gx > 0x7fffffffLL || gy > 65535) return sw_fail(SWNERF_E_ARG, "conv2d_nhwc: %lld output pixels x %d channels are too many for one launch", (long long)P.M, cout);
    const bool veca = cin % 4 == 0 && ((uintptr_t)in & 15) == 0, vecb = cout % 4 == 0 && ((uintptr_t)packed & 15) == 0;
    const dim3 grid((unsigned)gx, (unsigned)gy);
    if (bn == 128) cv_launch<2>(P, veca, vecb, grid, (hipStream_t)stream);
    else cv_launch<1>(P, veca, vecb, grid, (hipStream_t)stream);
    return sw_check(hipGetLastError(), "conv2d_nhwc launch");
}

// ---- max pooling ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float mp_max(float m, float v) { return (v > m || v != v) ? v : m; }   // torch: a NaN replaces, nothing replaces a NaN

template <int WIN, int VEC>
__global__ void __launch_bounds__(256) mp_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t total,
                                                      int64_t H, int64_t W, int C, int64_t Ho, int64_t Wo) {
    const int cv = C / VEC;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int c = (int)(e % cv) * VEC;
        int64_t p = e / cv;
        const int64_t ox = p % Wo; p /= Wo;
        const int64_t oy = p % Ho, n = p / Ho;
        const float* src = in + ((n * H + 2 * oy) * W + 2 * ox) * C + c;
        float m[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) m[j] = -INFINITY;
#pragma unroll
        for (int dy = 0; dy < WIN; ++dy)
#pragma unroll
            for (int dx = 0; dx < WIN; ++dx) {
                const float* q = src + ((int64_t)dy * W + dx) * C;
                if (VEC == 4) {
                    const cv_f32x4 v = *reinterpret_cast<const cv_f32x4*>(q);
#pragma unroll
                    for (int j = 0; j < 4; ++j) m[j] = mp_max(m[j], v[j]);
                } else {
                    m[0] = mp_max(m[0], q[0]);
                }
            }
        float* dst = out + ((n * Ho + oy) * Wo + ox) * C + c;
        if (VEC == 4) {
            const cv_f32x4 v = {m[0], m[1], m[2], m[3]};
            *reinterpret_cast<cv_f32x4*>(dst) = v;
        } else {
            dst[0] = m[0];
        }
    }
}

extern "C" int swnerf_maxpool2d_nhwc(const float* in, int64_t n, int64_t h, int64_t w, int c, int window, float* out, void* stream) {
    if (window != 2 && window != 3) return sw_fail(SWNERF_E_ARG, "maxpool2d_nhwc: window %d is neither 2 nor 3 (stride 2, floor mode, no padding)", window);
    if (n < 0) return sw_fail(SWNERF_E_ARG, "maxpool2d_nhwc: negative image count %lld", (long long)n);
    if (c < 1 || c > (1 << 20)) return sw_fail(SWNERF_E_ARG, "maxpool2d_nhwc: %d channels outside 1..2^20", c);
    if (h < window || w < window || h > CV_MAX_SIDE || w > CV_MAX_SIDE)
        return sw_fail(SWNERF_E_ARG, "maxpool2d_nhwc: a %lld x %lld image has no %d x %d window (or a side above 2^20)", (long long)h, (long long)w, window, window);
    if (n == 0) return 0;
    if (!in || !out) return sw_fail(SWNERF_E_ARG, "maxpool2d_nhwc: NULL pointer");
    if (((uintptr_t)in | (uintptr_t)out) & 3) return sw_fail(SWNERF_E_ARG, "maxpool2d_nhwc: operands must be 4-byte aligned");
    const int64_t ho = (h - window) / 2 + 1, wo = (w - window) / 2 + 1;
    const bool vec = c % 4 == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
    const int64_t total = n * ho * wo * (vec ? c / 4 : c);
    const unsigned gb = (unsigned)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
    hipStream_t st = (hipStream_t)stream;
    if (window == 2 && vec) hipLaunchKernelGGL((mp_pool_kernel<2, 4>), dim3(gb), dim3(256), 0, st, in, out, total, h, w, c, ho, wo);
    else if (window == 2) hipLaunchKernelGGL((mp_pool_kernel<2, 1>), dim3(gb), dim3(256), 0, st, in, out, total, h, w, c, ho, wo);
    else if (vec) hipLaunchKernelGGL((mp_pool_kernel<3, 4>), dim3(gb), dim3(256), 0, st, in, out, total, h, w, c, ho, wo);
    else hipLaunchKernelGGL((mp_pool_kernel<3, 1>), dim3(gb), dim3(256), 0, st, in, out, total, h, w, c, ho, wo);
    return sw_check(hipGetLastError(), "maxpool2d_nhwc launch");
}

// ---- one LPIPS tap --------------------------------------------------------------------------------------------------
#define LP_THREADS 256
#define LP_GROUP 16                    // lanes per pixel
#define LP_PIX (LP_THREADS / LP_GROUP) // pixels per block and step
#define LP_MAX_PB 256                  // blocks per image at most
#define LP_MAX_GRID_Y 65535
#define LP_EPS 1.0e-10f                // the eps of the package's normalize_tensor: f / (sqrt(sum f^2) + eps)

static inline int lp_blocks(int64_t hw) {
    const int64_t pb = (hw + 4 * LP_PIX - 1) / (4 * LP_PIX);
    return (int)(pb < 1 ? 1 : (pb > LP_MAX_PB ? LP_MAX_PB : pb));
}

__device__ __forceinline__ float lp_group_sum(float v) {
#pragma unroll
    for (int o = LP_GROUP / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <bool VEC>
__global__ void __launch_bounds__(LP_THREADS) lp_layer_kernel(const float* __restrict__ f0, const float* __restrict__ f1,
                                                              const float* __restrict__ lin, int64_t n_img, int64_t hw, int C,
                                                              int pb, double* __restrict__ part, float* __restrict__ map) {
    __shared__ double red[LP_THREADS / 64];
    const int t = threadIdx.x, g = t & (LP_GROUP - 1), grp = t / LP_GROUP;
    for (int64_t n = blockIdx.y; n < n_img; n += gridDim.y) {
        double sum = 0.0;
        for (int64_t p = (int64_t)blockIdx.x * LP_PIX + grp; p < hw; p += (int64_t)pb * LP_PIX) {
            const float* a = f0 + (n * hw + p) * C;
            const float* b = f1 + (n * hw + p) * C;
            float sa = 0.f, sb = 0.f;
            if (VEC) {
                for (int c = 4 * g; c < C; c += 4 * LP_GROUP) {
                    const cv_f32x4 va = *reinterpret_cast<const cv_f32x4*>(a + c), vb = *reinterpret_cast<const cv_f32x4*>(b + c);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { sa += va[j] * va[j]; sb += vb[j] * vb[j]; }
                }
            } else {
                for (int c = g; c < C; c += LP_GROUP) { sa += a[c] * a[c]; sb += b[c] * b[c]; }
            }
            const float na = sqrtf(lp_group_sum(sa)) + LP_EPS, nb = sqrtf(lp_group_sum(sb)) + LP_EPS;
            float d = 0.f;
            if (VEC) {
                for (int c = 4 * g; c < C; c += 4 * LP_GROUP) {
                    const cv_f32x4 va = *reinterpret_cast<const cv_f32x4*>(a + c), vb = *reinterpret_cast<const cv_f32x4*>(b + c);
                    const cv_f32x4 wl = *reinterpret_cast<const cv_f32x4*>(lin + c);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { const float x = va[j] / na - vb[j] / nb; d += wl[j] * (x * x); }
                }
            } else {
                for (int c = g; c < C; c += LP_GROUP) { const float x = a[c] / na - b[c] / nb; d += lin[c] * (x * x); }
            }
            d = lp_group_sum(d);
            if (g == 0) {
                sum += (double)d;
                if (map) map[n * hw + p] = d;
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if ((t & 63) == 0) red[t >> 6] = sum;
        __syncthreads();
        if (t == 0) part[n * pb + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) lp_finish_kernel(const double* __restrict__ part, int64_t n_img, int64_t hw, int pb,
                                                        int accumulate, double* __restrict__ out) {
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < n_img; n += (int64_t)gridDim.x * 256) {
        double s = 0.0;
        for (int b = 0; b < pb; ++b) s += part[n * pb + b];
        s /= (double)hw;
        out[n] = accumulate ? out[n] + s : s;
    }
}

extern "C" size_t swnerf_lpips_layer_workspace_bytes(int64_t n, int64_t h, int64_t w) {
    if (n <= 0 || h < 1 || w < 1 || h > CV_MAX_SIDE || w > CV_MAX_SIDE) return 0;
    return (size_t)(8 * n * lp_blocks(h * w));
}

extern "C" int swnerf_lpips_layer(const float* f0, const float* f1, const float* lin, int64_t n, int64_t h, int64_t w, int c,
                                  int accumulate, void* workspace, double* out, float* map, void* stream) {
    if (n < 0) return sw_fail(SWNERF_E_ARG, "lpips_layer: negative image count %lld", (long long)n);
    if (c < 1 || c > (1 << 20)) return sw_fail(SWNERF_E_ARG, "lpips_layer: %d channels outside 1..2^20", c);
    if (h < 1 || w < 1 || h > CV_MAX_SIDE || w > CV_MAX_SIDE) return sw_fail(SWNERF_E_ARG, "lpips_layer: feature-map side outside 1..2^20");
    if (n == 0) return 0;
    if (!f0 || !f1 || !lin || !workspace || !out) return sw_fail(SWNERF_E_ARG, "lpips_layer: NULL pointer");
    if (((uintptr_t)f0 | (uintptr_t)f1 | (uintptr_t)lin | (uintptr_t)map) & 3) return sw_fail(SWNERF_E_ARG, "lpips_layer: operands must be 4-byte aligned");
    if (((uintptr_t)workspace | (uintptr_t)out) & 7) return sw_fail(SWNERF_E_ARG, "lpips_layer: workspace and out must be 8-byte aligned");
    const int64_t hw = h * w;
    const int pb = lp_blocks(hw);
    const bool vec = c % 4 == 0 && (((uintptr_t)f0 | (uintptr_t)f1 | (uintptr_t)lin) & 15) == 0;
    const unsigned gy = (unsigned)(n < LP_MAX_GRID_Y ? n : LP_MAX_GRID_Y);
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)workspace;
    if (vec) hipLaunchKernelGGL(lp_layer_kernel<true>, dim3(pb, gy), dim3(LP_THREADS), 0, st, f0, f1, lin, n, hw, c, pb, part, map);
    else hipLaunchKernelGGL(lp_layer_kernel<false>, dim3(pb, gy), dim3(LP_THREADS), 0, st, f0, f1, lin, n, hw, c, pb, part, map);
    int rc = sw_check(hipGetLastError(), "lpips_layer launch");
    if (rc) return rc;
    const unsigned fb = (unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(lp_finish_kernel, dim3(fb), dim3(256), 0, st, (const double*)part, n, hw, pb, accumulate ? 1 : 0, out);
    return sw_check(hipGetLastError(), "lpips_layer finish launch");
}
