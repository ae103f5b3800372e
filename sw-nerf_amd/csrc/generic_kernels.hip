// generic_kernels.hip - the NeRF MLPs at ANY shape (model.py:10-62, 93-151, 227-296 with D, W, skips, input sizes and
// use_viewdirs as given): one nn.Linear at a time.  The shipped configs (D=8, W=256, skips=[4], use_viewdirs=True) run
// on the register-resident fused kernels (mlp_core.h); everything else - `use_viewdirs=False` (the reference's argparse
// default, utils.py:26-29 / model.py:59-60), other depths / widths / skip sets - runs layer by layer on this tiled
// fp32-MFMA GEMM, which is slower but exact in the same sense (v_mfma_f32_32x32x2_f32, fp32 accumulate).
//
//   linear   : Y[M,N] = act(X[M,K] . W[N,K]^T + b)         (torch.nn.functional.linear [+ relu])
//   gemm_nn  : dX[M,K] = dY[M,N] . W[N,K]                   (its input gradient)
//   relu_mask: dY *= (Y > 0)                                (relu backward, in place)
//   linear_act / elu_grad: the same GEMM with an ELU epilogue (elu.h) and its backward from the output (TNeRF, model.py:152-210)
// The weight gradient dW = dY^T . X and db = column sums are swnerf_gemm_tn (wgrad_kernels.hip).
//
// One workgroup (4 waves) owns a 64 x 64 block of the output, wave w the 32 x 32 tile (w&1, w>>1); the K dimension
// is walked in chunks of 32 staged through LDS with bounds-checked 4-byte loads (any leading dimension, any K: 63, 90,
// 319 ...; consecutive lanes read consecutive k of one row, so the loads coalesce).  In the MFMA both operands use
// the same (lane half, step) -> k map, so any k order is a valid contraction order.
#include <hip/hip_runtime.h>
#include "../../include/swnerf.h"
#include "host_util.h"
#include "elu.h"
#include <cstdint>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define GK_CH 32                 // k per chunk
#define GK_LD (GK_CH + 1)        // LDS row pitch (floats): odd, so the 32 rows of a tile hit 32 different banks

struct GenericGemm {
    const float* A; int lda;     // [M, K] row-major
    const float* B; int ldb;     // BT: [N, K] row-major (C = A.B^T);  else [K, N] row-major (C = A.B)
    const float* bias;           // [N] or NULL
    float* C; int ldc;           // [M, N]
    int64_t M; int N, K; int act;    // epilogue: SWNERF_ACT_NONE / _RELU / _ELU
};

template <bool BT>
__global__ void __launch_bounds__(256) generic_gemm_kernel(GenericGemm P) {
    __shared__ float As[64][GK_LD];
    __shared__ float Bs[64][GK_LD];
    const int t = threadIdx.x, lane = t & 63, i = lane & 31, h = lane >> 5;
    const int wv = t >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * 64;     // rows on grid.x (2^31-1 blocks); grid.y is capped at 65535
    const int n0 = blockIdx.y * 64;
    const int wm = 32 * (wv & 1), wn = 32 * (wv >> 1);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < P.K; k0 += GK_CH) {
        // stage A[m0..+64][k0..+32] and op(B)[n0..+64][k0..+32]: 2048 floats each, 8 per thread
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = t + 256 * q, row = e >> 5, kk = e & 31;
            const int64_t m = m0 + row;
            const int k = k0 + kk;
            As[row][kk] = (m < P.M && k < P.K) ? P.A[m * P.lda + k] : 0.f;
        }
        if (BT) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int e = t + 256 * q, row = e >> 5, kk = e & 31;
                const int n = n0 + row, k = k0 + kk;
                Bs[row][kk] = (n < P.N && k < P.K) ? P.B[(int64_t)n * P.ldb + k] : 0.f;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int e = t + 256 * q, kk = e >> 6, col = e & 63;       // consecutive lanes: consecutive n of one k row
                const int n = n0 + col, k = k0 + kk;
                Bs[col][kk] = (n < P.N && k < P.K) ? P.B[(int64_t)k * P.ldb + n] : 0.f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < GK_CH / 2; ++s) {
            const float a = As[wm + i][2 * s + h];
            const float b = Bs[wn + i][2 * s + h];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D map: register r of lane (j = i, h) is row (r&3) + 8(r>>2) + 4h of the tile, column j
    const int n = n0 + wn + i;
    if (n >= P.N) return;
    const float bv = P.bias ? P.bias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (m < P.M) {
            float v = acc[r] + bv;
            if (P.act == SWNERF_ACT_RELU) v = fmaxf(v, 0.f);
            else if (P.act == SWNERF_ACT_ELU) v = sw_elu(v);
            P.C[m * P.ldc + n] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The same GEMM for outputs at least 64 wide (round 3): a 128 x 128 block of C per workgroup, wave w the 64 x 64 quadrant
// (w&1, w>>1) as 2 x 2 accumulator tiles - four times the MFMA work per staged float of the 64 x 64 kernel above, which ran
// the 8x256 nets at 29 % of the fp32-MFMA roofline.  K is walked in chunks of 32 through two LDS buffers: the next chunk's
// global loads are in flight (registers) while this chunk feeds the matrix pipe, one barrier per chunk.  Operand tiles sit
// K-MAJOR in LDS ([k][row]), so an MFMA operand read is 32 consecutive floats (conflict free) and the pitch is chosen per
// operand so that the staging writes are conflict free too: 129 floats where a thread writes 4 consecutive k of one row
// (A, and B as [N,K]), 132 where it writes 4 consecutive columns of one k (B as [K,N]: one ds_write_b128).
// VEC: both operands allow 16-byte loads (base, leading dimension); otherwise 4-byte loads with the same coalescing.
#define G2_KC 32
#define G2_PA 129
template <bool BT, bool VEC>
__global__ void __launch_bounds__(256, 2) generic_gemm128_kernel(GenericGemm P) {
    constexpr int PB = BT ? 129 : 132;
    extern __shared__ __attribute__((aligned(16))) float g2_lds[];          // [2][ A: KC x PA | B: KC x PB ]
    constexpr int BUF = G2_KC * (G2_PA + PB);
    const int t = threadIdx.x, lane = t & 63, i = lane & 31, h = lane >> 5;
    const int wv = t >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * 128;
    const int n0 = blockIdx.y * 128;
    const int wm = 64 * (wv & 1), wn = 64 * (wv >> 1);
    f32x16 acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;
    float ra[16], rb[16];                                                     // the next chunk, on its way from global memory
    auto load = [&](int k0) {
        if (VEC) {
            // A (and B^T): thread -> (row = t/8 + 32 q, k = 4 (t%8) ..+3): 8 threads read one 128-byte line of a row
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = (t >> 3) + 32 * q, kk = 4 * (t & 7);
                const int64_t m = m0 + row;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (m < P.M && k0 + kk < P.K) v = *reinterpret_cast<const f32x4*>(P.A + m * P.lda + k0 + kk);   // K % 4 == 0 on this path
                ra[4 * q] = v[0]; ra[4 * q + 1] = v[1]; ra[4 * q + 2] = v[2]; ra[4 * q + 3] = v[3];
            }
            if (BT) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int row = (t >> 3) + 32 * q, kk = 4 * (t & 7);
                    const int n = n0 + row;
                    f32x4 v = {0.f, 0.f, 0.f, 0.f};
                    if (n < P.N && k0 + kk < P.K) v = *reinterpret_cast<const f32x4*>(P.B + (int64_t)n * P.ldb + k0 + kk);
                    rb[4 * q] = v[0]; rb[4 * q + 1] = v[1]; rb[4 * q + 2] = v[2]; rb[4 * q + 3] = v[3];
                }
            } else {
                // B [K,N]: thread -> (k = t/32 + 8 q, n = 4 (t%32) ..+3): 32 threads read 512 consecutive bytes of a k row
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int kk = (t >> 5) + 8 * q, col = 4 * (t & 31);
                    f32x4 v = {0.f, 0.f, 0.f, 0.f};
                    if (k0 + kk < P.K && n0 + col < P.N) v = *reinterpret_cast<const f32x4*>(P.B + (int64_t)(k0 + kk) * P.ldb + n0 + col);   // N % 4 == 0 on this path
                    rb[4 * q] = v[0]; rb[4 * q + 1] = v[1]; rb[4 * q + 2] = v[2]; rb[4 * q + 3] = v[3];
                }
            }
        } else {
            // 4-byte loads: element e = t + 256 q -> (row = e/32, k = e%32) for A and B^T, (k = e/128, n = e%128) for B [K,N]
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int e = t + 256 * q, row = e >> 5, kk = e & 31;
                const int64_t m = m0 + row;
                ra[q] = (m < P.M && k0 + kk < P.K) ? P.A[m * P.lda + k0 + kk] : 0.f;
                if (BT) {
                    const int n = n0 + row;
                    rb[q] = (n < P.N && k0 + kk < P.K) ? P.B[(int64_t)n * P.ldb + k0 + kk] : 0.f;
                } else {
                    const int k2 = e >> 7, col = e & 127;
                    rb[q] = (k0 + k2 < P.K && n0 + col < P.N) ? P.B[(int64_t)(k0 + k2) * P.ldb + n0 + col] : 0.f;
                }
            }
        }
    };
    auto stage = [&](int buf) {
        float* As = g2_lds + buf * BUF;
        float* Bs = As + G2_KC * G2_PA;
        if (VEC) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = (t >> 3) + 32 * q, kk = 4 * (t & 7);
#pragma unroll
                for (int e = 0; e < 4; ++e) As[(kk + e) * G2_PA + row] = ra[4 * q + e];
                if (BT) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) Bs[(kk + e) * PB + row] = rb[4 * q + e];
                }
            }
            if (!BT) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int kk = (t >> 5) + 8 * q, col = 4 * (t & 31);
                    const f32x4 v = {rb[4 * q], rb[4 * q + 1], rb[4 * q + 2], rb[4 * q + 3]};
                    *reinterpret_cast<f32x4*>(Bs + kk * PB + col) = v;
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int e = t + 256 * q, row = e >> 5, kk = e & 31;
                As[kk * G2_PA + row] = ra[q];
                if (BT) Bs[kk * PB + row] = rb[q];
                else Bs[(e >> 7) * PB + (e & 127)] = rb[q];
            }
        }
    };
    const int nch = (P.K + G2_KC - 1) / G2_KC;
    load(0);
    stage(0);
    __syncthreads();
#pragma nounroll
    for (int c = 0; c < nch; ++c) {
        if (c + 1 < nch) load((c + 1) * G2_KC);                               // in flight while this chunk computes
        const float* As = g2_lds + (c & 1) * BUF + wm + i;
        const float* Bs = g2_lds + (c & 1) * BUF + G2_KC * G2_PA + wn + i;
#pragma unroll
        for (int s = 0; s < G2_KC / 2; ++s) {
            const float a0 = As[(2 * s + h) * G2_PA], a1 = As[(2 * s + h) * G2_PA + 32];
            const float b0 = Bs[(2 * s + h) * PB], b1 = Bs[(2 * s + h) * PB + 32];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[3], 0, 0, 0);
        }
        if (c + 1 < nch) stage((c + 1) & 1);                                   // the buffer nobody reads in this iteration
        __syncthreads();
    }
    // C/D map: register r of lane (j = i, h) of tile (x, y) is row wm + 32 x + frow(r,h), column wn + 32 y + j
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int n = n0 + wn + 32 * y + i;
            if (n >= P.N) continue;
            const float bv = P.bias ? P.bias[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t m = m0 + wm + 32 * x + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (m < P.M) {
                    float v = acc[2 * x + y][r] + bv;
                    if (P.act == SWNERF_ACT_RELU) v = fmaxf(v, 0.f);
                    else if (P.act == SWNERF_ACT_ELU) v = sw_elu(v);
                    P.C[m * P.ldc + n] = v;
                }
            }
        }
}

static int generic_launch(const GenericGemm& P, bool bt, void* stream, const char* what) {
    if (P.M == 0) return 0;
    if (!P.A || !P.B || !P.C || P.M < 0 || P.N < 1 || P.K < 1 || P.lda < P.K || P.ldc < P.N || P.ldb < (bt ? P.K : P.N))
        return sw_fail(SWNERF_E_ARG, "%s: bad arguments (M=%lld N=%d K=%d lda=%d ldb=%d ldc=%d)", what, (long long)P.M, P.N, P.K, P.lda, P.ldb, P.ldc);
    if (P.N >= 64 && P.M >= 128) {
        const int64_t gx2 = (P.M + 127) / 128, gy2 = (P.N + 127) / 128;
        if (gx2 > 0x7fffffffLL || gy2 > 65535) return sw_fail(SWNERF_E_UNSUPP, "%s: M %lld or N %d too large for one launch", what, (long long)P.M, P.N);
        const dim3 grid2((unsigned)gx2, (unsigned)gy2), block2(256);
        const bool vec = (P.lda % 4 == 0) && (P.ldb % 4 == 0) && (((uintptr_t)P.A | (uintptr_t)P.B) % 16 == 0) && (P.K % 4 == 0) && (bt || P.N % 4 == 0);
        const size_t lds = 2 * G2_KC * (G2_PA + (bt ? 129 : 132)) * sizeof(float);
        hipStream_t st = (hipStream_t)stream;
        if (bt && vec) hipLaunchKernelGGL((generic_gemm128_kernel<true, true>), grid2, block2, lds, st, P);
        else if (bt) hipLaunchKernelGGL((generic_gemm128_kernel<true, false>), grid2, block2, lds, st, P);
        else if (vec) hipLaunchKernelGGL((generic_gemm128_kernel<false, true>), grid2, block2, lds, st, P);
        else hipLaunchKernelGGL((generic_gemm128_kernel<false, false>), grid2, block2, lds, st, P);
        return sw_check(hipGetLastError(), what);
    }
    const int64_t gx = (P.M + 63) / 64, gy = (P.N + 63) / 64;
    if (gx > 0x7fffffffLL || gy > 65535) return sw_fail(SWNERF_E_UNSUPP, "%s: M %lld or N %d too large for one launch", what, (long long)P.M, P.N);
    const dim3 grid((unsigned)gx, (unsigned)gy), block(256);
    if (bt) hipLaunchKernelGGL(generic_gemm_kernel<true>, grid, block, 0, (hipStream_t)stream, P);
    else hipLaunchKernelGGL(generic_gemm_kernel<false>, grid, block, 0, (hipStream_t)stream, P);
    return sw_check(hipGetLastError(), what);
}

extern "C" int swnerf_linear(const float* x, int ldx, int64_t M, int K, const float* weight, const float* bias, int N,
                             int relu, float* y, int ldy, void* stream) {
    GenericGemm P;
    P.A = x; P.lda = ldx; P.B = weight; P.ldb = K; P.bias = bias; P.C = y; P.ldc = ldy; P.M = M; P.N = N; P.K = K; P.act = relu ? SWNERF_ACT_RELU : SWNERF_ACT_NONE;
    return generic_launch(P, true, stream, "linear");
}

extern "C" int swnerf_gemm_nn(const float* a, int lda, int64_t M, int K, const float* b, int ldb, int N, float* c, int ldc,
                              void* stream) {
    GenericGemm P;
    P.A = a; P.lda = lda; P.B = b; P.ldb = ldb; P.bias = nullptr; P.C = c; P.ldc = ldc; P.M = M; P.N = N; P.K = K; P.act = SWNERF_ACT_NONE;
    return generic_launch(P, false, stream, "gemm_nn");
}

__global__ void __launch_bounds__(256) relu_mask_kernel(float* dy, const float* y, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) dy[e] = (y[e] > 0.f) ? dy[e] : 0.f;
}

extern "C" int swnerf_relu_mask(float* dy, const float* y, int64_t n, void* stream) {
    if (n == 0) return 0;
    if (!dy || !y || n < 0) return sw_fail(SWNERF_E_ARG, "relu_mask: NULL pointer or negative count");
    hipLaunchKernelGGL(relu_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, y, n);
    return sw_check(hipGetLastError(), "relu_mask launch");
}

extern "C" int swnerf_linear_act(const float* x, int ldx, int64_t M, int K, const float* weight, const float* bias, int N,
                                 int act, float* y, int ldy, void* stream) {
    if (act != SWNERF_ACT_NONE && act != SWNERF_ACT_RELU && act != SWNERF_ACT_ELU)
        return sw_fail(SWNERF_E_ARG, "linear_act: unknown activation %d (0 none, 1 relu, 2 elu)", act);
    GenericGemm P;
    P.A = x; P.lda = ldx; P.B = weight; P.ldb = K; P.bias = bias; P.C = y; P.ldc = ldy; P.M = M; P.N = N; P.K = K; P.act = act;
    return generic_launch(P, true, stream, "linear_act");
}

// ELU backward from the output: elu'(x) = 1 for x > 0, exp(x) = y + 1 otherwise
__global__ void __launch_bounds__(256) elu_grad_kernel(float* dy, const float* y, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) {
        const float v = y[e];
        dy[e] = (v > 0.f) ? dy[e] : dy[e] * (v + 1.f);
    }
}

extern "C" int swnerf_elu_grad(float* dy, const float* y, int64_t n, void* stream) {
    if (n == 0) return 0;
    if (!dy || !y || n < 0) return sw_fail(SWNERF_E_ARG, "elu_grad: NULL pointer or negative count");
    hipLaunchKernelGGL(elu_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, y, n);
    return sw_check(hipGetLastError(), "elu_grad launch");
}

// ---------------------------------------------------------------------------------------------
// The weight gradient with a REPRODUCIBLE sum: C[No,ldc] += A[M,lda]^T . B[M,ldb], bias[No] += column sums of A - what
// swnerf_gemm_tn computes, but swnerf_gemm_tn combines its row slices with float atomics, so two identical calls differ
// in the last bits.  Here every row slice writes its own partial product (plain stores, one owner per entry) and a second
// kernel adds the slices in slice order.  The split depends on (M, No, Ni) alone, so equal calls give equal bits.
//   ws: [nslices][No][Ni + 1] - column Ni holds the slice's column sums of A.
// One wave owns a 32 x 32 tile of a slice's partial product (4 waves: 4 neighbouring column tiles, sharing the A rows
// through L1); lane (i, h) supplies A[m + h][o0 + i] and B[m + h][i0 + i] straight from global memory, two contiguous
// 128-byte segments per wave load, bounds checked (any leading dimension, any No / Ni, odd slice lengths).
struct OrderedTN { const float* A; int lda; int No; const float* B; int ldb; int Ni; int64_t M; int64_t rows_per_slice; float* ws; };

__global__ void __launch_bounds__(256) gemm_tn_slice_kernel(OrderedTN P) {
    const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const int it = 4 * blockIdx.z + (threadIdx.x >> 6);       // this wave's column tile
    if (32 * it >= P.Ni) return;                                // (no barrier below)
    const int o = 32 * blockIdx.y + i, col = 32 * it + i;
    const bool ao = o < P.No, bc = col < P.Ni;
    const int64_t m0 = (int64_t)blockIdx.x * P.rows_per_slice;
    const int64_t mend = m0 + P.rows_per_slice < P.M ? m0 + P.rows_per_slice : P.M;
    const float* Ap = P.A + (ao ? o : 0);
    const float* Bp = P.B + (bc ? col : 0);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float bsum = 0.f;
    const int64_t nsteps = (mend - m0 + 1) / 2;               // two rows per MFMA; an odd slice's last step has one
    // a row past the slice (and a column past the operand) is read at a clamped, valid address and replaced by zero
    auto step = [&](int64_t s, float& a, float& b) {
        const int64_t m = m0 + 2 * s + h, mc = m < mend ? m : mend - 1;
        a = Ap[mc * P.lda];
        b = Bp[mc * P.ldb];
        a = (m < mend && ao) ? a : 0.f;
        b = (m < mend && bc) ? b : 0.f;
    };
    int64_t s = 0;
    for (; s + 4 <= nsteps; s += 4) {                          // four steps' loads in flight
        float a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) step(s + q, a[q], b[q]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            bsum += a[q];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], b[q], acc, 0, 0, 0);
        }
    }
    for (; s < nsteps; ++s) {
        float a, b;
        step(s, a, b);
        bsum += a;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    // C/D map: register r of lane (j = i, h) is row (r&3) + 8(r>>2) + 4h of the tile, column j
    float* W = P.ws + (size_t)blockIdx.x * P.No * (P.Ni + 1);
    if (bc) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int orow = 32 * blockIdx.y + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (orow < P.No) W[(size_t)orow * (P.Ni + 1) + col] = acc[r];
        }
    }
    if (it == 0) {
        bsum += __shfl_xor(bsum, 32, 64);
        if (h == 0 && ao) W[(size_t)o * (P.Ni + 1) + P.Ni] = bsum;
    }
}

__global__ void __launch_bounds__(256) gemm_tn_sum_slices_kernel(const float* ws, int nslices, int No, int Ni, float* C, int ldc, float* bias) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, n = (int64_t)No * (Ni + 1);
    if (e >= n) return;
    float s = 0.f;
    for (int k = 0; k < nslices; ++k) s += ws[k * n + e];       // slice order, always
    const int o = (int)(e / (Ni + 1)), col = (int)(e % (Ni + 1));
    if (col < Ni) C[(size_t)o * ldc + col] += s;
    else if (bias) bias[o] += s;
}

// at most 256 slices of at least 512 rows (an even number each), and at most 16 MiB of partial products
static void ordered_split(int64_t M, int No, int Ni, int64_t* rows_per_slice, int64_t* nslices) {
    int64_t ns = (M + 511) / 512;
    const int64_t cap = ((int64_t)4 << 20) / ((int64_t)No * (Ni + 1));
    if (ns > 256) ns = 256;
    if (ns > cap) ns = cap;
    if (ns < 1) ns = 1;
    const int64_t rows = ((M + ns - 1) / ns + 1) / 2 * 2;
    *rows_per_slice = rows;
    *nslices = (M + rows - 1) / rows;
}

// (the tiles of C lie on grid.y and grid.z: 65535 blocks each at most)
static bool ordered_shape_ok(int64_t M, int No, int Ni) { return M >= 0 && No >= 1 && No <= 65536 && Ni >= 1 && Ni <= 65536; }

extern "C" size_t swnerf_gemm_tn_ordered_ws_floats(int64_t M, int No, int Ni) {
    if (!ordered_shape_ok(M, No, Ni) || M == 0) return 0;
    int64_t rows, ns;
    ordered_split(M, No, Ni, &rows, &ns);
    return (size_t)ns * No * (Ni + 1);
}

extern "C" int swnerf_gemm_tn_ordered(const float* A, int lda, int No, const float* B, int ldb, int Ni, int64_t M,
                                      float* C, int ldc, float* bias, float* ws, size_t ws_floats, void* stream) {
    if (M == 0) return 0;
    if (!A || !B || !C || !ws || M < 0 || No < 1 || Ni < 1 || lda < No || ldb < Ni || ldc < Ni)
        return sw_fail(SWNERF_E_ARG, "gemm_tn_ordered: bad arguments (M=%lld No=%d Ni=%d lda=%d ldb=%d ldc=%d)", (long long)M, No, Ni, lda, ldb, ldc);
    if (!ordered_shape_ok(M, No, Ni)) return sw_fail(SWNERF_E_UNSUPP, "gemm_tn_ordered: No and Ni up to 65536 (No=%d Ni=%d)", No, Ni);
    OrderedTN P;
    int64_t ns;
    ordered_split(M, No, Ni, &P.rows_per_slice, &ns);
    if (ws_floats < (size_t)ns * No * (Ni + 1))
        return sw_fail(SWNERF_E_ARG, "gemm_tn_ordered: workspace of %zu floats, needs %zu (swnerf_gemm_tn_ordered_ws_floats)", ws_floats, (size_t)ns * No * (Ni + 1));
    P.A = A; P.lda = lda; P.No = No; P.B = B; P.ldb = ldb; P.Ni = Ni; P.M = M; P.ws = ws;
    const int ti = (Ni + 31) / 32;
    hipLaunchKernelGGL(gemm_tn_slice_kernel, dim3((unsigned)ns, (unsigned)((No + 31) / 32), (unsigned)((ti + 3) / 4)), dim3(256), 0, (hipStream_t)stream, P);
    if (int rc = sw_check(hipGetLastError(), "gemm_tn_ordered launch")) return rc;
    const int64_t n = (int64_t)No * (Ni + 1);
    hipLaunchKernelGGL(gemm_tn_sum_slices_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)ws, (int)ns, No, Ni, C, ldc, bias);
    return sw_check(hipGetLastError(), "gemm_tn_ordered sum launch");
}
