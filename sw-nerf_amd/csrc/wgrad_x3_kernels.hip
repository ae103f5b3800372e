// wgrad_x3_kernels.hip - the 256 x 256 weight-gradient GEMMs of a training step in "bf16x3" arithmetic (opt-in:
// swnerf/wgrad.py set_precision).  C[o][i] += sum_m A[m][o] * B[m][i] with every fp32 operand element split as
// v = hi + lo (bf16x3_split.h) and the product evaluated as A_hi.B_hi + A_hi.B_lo + A_lo.B_hi on v_mfma_f32_32x32x16_bf16 with fp32
// accumulation: 3/16 of the matrix cycles of the fp32 kernel (wgrad_kernels.hip gemm_tn_dma_group_kernel), whose plan it keeps -
// one 16-wave workgroup owns the whole 256 x 256 block for its row slice, 32-row fp32 slabs of A and B arrive by LDS-DMA, double
// buffered, the rows are split by wgrad_host.h split_rows, ONE launch covers up to 16 items, float atomics in the epilogue.
// A translation unit of its own: the fp32 kernels' register counts depend on what shares their unit (wgrad_kernels.hip, top).
//
// Operand layout.  The reduction index of this GEMM is the data ROW, and lane (r, h) of the bf16 MFMA holds eight consecutive
// k = 8h .. 8h+7 of one column r.  The slabs stay fp32 in LDS exactly as the DMA wrote them, and a lane reads its eight rows
// with eight strided 8-byte reads (two adjacent columns each: the wave's tiles are interleaved as in the fp32 kernel) and splits
// them in registers.  The other route - a second, bf16 image written once per slab and read back transposed - would split each
// element once instead of four times (the four waves that share a column block), but costs another pass over LDS, a second
// barrier per slab and a 64-KB image that does not fit a CU's 160 KB next to the 128 KB of double-buffered fp32 slabs.  Here a slab
// costs each wave 32 reads and ~200 vector instructions next to 24 MFMAs of 32 cycles, which four waves per SIMD overlap; per
// 64-KB slab that stays below the time HBM needs to deliver it: the launch runs at 4.1 TB/s on its operands (profiles/wgrad_x3.md).
#include <hip/hip_runtime.h>
#include "../../include/swnerf.h"
#include "swnerf_common.h"
#include "lds_dma.h"
#include "host_util.h"
#include "wgrad_host.h"
#include "bf16x3_split.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#define X3W_SLAB 32                                   // rows per LDS slab = two k-steps of 16
#define X3W_BUF_FLOATS (2 * X3W_SLAB * 256)           // A slab then B slab
#define X3W_MAX 16
#define X3W_WG_TARGET 256                             // one workgroup per CU: each holds 128 KB of LDS

struct X3Item { const float* A; int lda; const float* B; int ldb; float* C; int ldc; float* bias; int64_t rows_per_wg; };
struct X3Group { int n; int64_t M; int wg0[X3W_MAX + 1]; X3Item it[X3W_MAX]; };      // wg0: first workgroup of item k (prefix sums)

// eight rows x two adjacent columns of fp32 -> the (hi, lo) operands of the two interleaved tiles: element j of a fragment is row j
__device__ __forceinline__ void x3w_split8(const f32x2 (&v)[8], u32x4 (&hi)[2], u32x4 (&lo)[2]) {
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned h2, l2;
            x3_split_pair(v[2 * q][c], v[2 * q + 1][c], h2, l2);
            hi[c][q] = h2; lo[c][q] = l2;
        }
}

__global__ void __launch_bounds__(1024) gemm_tn_x3_group_kernel(X3Group G) {
    int k = 0;
    while (k + 1 < G.n && (int)blockIdx.x >= G.wg0[k + 1]) ++k;               // wave-uniform: scalar
    const X3Item& P = G.it[k];
    const int slice = (int)blockIdx.x - G.wg0[k];
    extern __shared__ __attribute__((aligned(16))) float x3w_lds[];          // [2][X3W_BUF_FLOATS]
    const int t = threadIdx.x, lane = t & 63, i = lane & 31, hp = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int o0 = 64 * (w & 3), i0 = 64 * (w >> 2);                          // the wave's 64 x 64 block of C
    const int64_t m0 = (int64_t)slice * P.rows_per_wg;
    const int mlen = (int)(min(G.M, m0 + P.rows_per_wg) - m0);
    const int nslab = (mlen + X3W_SLAB - 1) / X3W_SLAB;
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)x3w_lds);
    const unsigned voff = (unsigned)lane * 16u;
    // slab s -> buffer s&1: 64 rows of 1 KiB (32 of A, 32 of B), 4 per wave; the row pointers advance by one slab per call.
    // Rows past the slice (last slab only) are clamped to its last row - never out of bounds - and zeroed on the A side below.
    const char* cur[4];
    int64_t step[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int id = w * 4 + q, row = id & 31;
        cur[q] = reinterpret_cast<const char*>(id < 32 ? P.A + (m0 + row) * P.lda : P.B + (m0 + row) * P.ldb);
        step[q] = (int64_t)X3W_SLAB * 4 * (id < 32 ? P.lda : P.ldb);
    }
    auto issue = [&](int sl) {
        const bool full = (sl + 1) * X3W_SLAB <= mlen;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int id = w * 4 + q, row = id & 31;
            const char* g = cur[q];
            if (!full) {
                const int64_t r = m0 + min(sl * X3W_SLAB + row, mlen - 1);
                g = reinterpret_cast<const char*>(id < 32 ? P.A + r * P.lda : P.B + r * P.ldb);
            }
            ws_dma(g, voff, lds0 + (unsigned)((sl & 1) * X3W_BUF_FLOATS * 4 + id * 1024));
            cur[q] += step[q];
        }
    };
    f32x16 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
    f32x2 bs01 = {0.f, 0.f};                                 // fp32 column sums of this lane's two (unsplit) A columns
    const bool do_bias = P.bias != nullptr && i0 == 0;       // wave-uniform: the four waves of the first column block
    issue(0);
#pragma nounroll
    for (int sl = 0; sl < nslab; ++sl) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's share of slab sl has landed ...
        __syncthreads();                                      // ... everyone's has; and everyone is done with slab sl-1
        float* Abw = x3w_lds + (sl & 1) * X3W_BUF_FLOATS;
        const int valid = mlen - sl * X3W_SLAB;
        if (valid < X3W_SLAB) {                               // the slice's last, partial slab: zero the clamped copies on the A side
            for (int e = t; e < (X3W_SLAB - valid) * 256; e += 1024) Abw[valid * 256 + e] = 0.f;
            __syncthreads();
        }
        if (sl + 1 < nslab) issue(sl + 1);
        // lane (i, hp) of k-step ks reads rows 16 ks + 8 hp + j, j = 0..7, at columns o0 + 2i, +1 (A) and i0 + 2i, +1 (B): the wave's
        // four tiles are rows o0 + 2m + {0,1} x columns i0 + 2n + {0,1}, so both columns of a row are ONE ds_read_b64 and every read
        // of a slab is base + immediate offset
        const f32x2* Ap = reinterpret_cast<const f32x2*>(Abw + o0 + 2 * i + 8 * hp * 256);
        const f32x2* Bp = reinterpret_cast<const f32x2*>(Abw + X3W_SLAB * 256 + i0 + 2 * i + 8 * hp * 256);
#pragma unroll
        for (int ks = 0; ks < X3W_SLAB / 16; ++ks) {
            f32x2 v[8];
            u32x4 ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = Ap[(16 * ks + j) * 128];
            if (do_bias) {
#pragma unroll
                for (int j = 0; j < 8; ++j) bs01 += v[j];
            }
            x3w_split8(v, ah, al);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = Bp[(16 * ks + j) * 128];
            x3w_split8(v, bh, bl);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const bf16x8 a_hi = __builtin_bit_cast(bf16x8, ah[b >> 1]), b_hi = __builtin_bit_cast(bf16x8, bh[b & 1]);
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, al[b >> 1]), b_hi, acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, __builtin_bit_cast(bf16x8, bl[b & 1]), acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_hi, acc[b], 0, 0, 0);
            }
        }
    }
    // C/D map: register r of lane (j = i, h = hp) of tile (oa, ib) is row o0 + 2 frow(r,h) + oa, column i0 + 2 j + ib (interleaved tiles)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int col = i0 + 2 * i + (b & 1);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = o0 + 2 * sw_frow(r, hp) + (b >> 1);
            atomicAdd(P.C + (size_t)o * P.ldc + col, acc[b][r]);
        }
    }
    if (do_bias) {
        float bs0 = bs01[0], bs1 = bs01[1];
        bs0 += __shfl_xor(bs0, 32, 64); bs1 += __shfl_xor(bs1, 32, 64);
        if (hp == 0) { atomicAdd(P.bias + o0 + 2 * i, bs0); atomicAdd(P.bias + o0 + 2 * i + 1, bs1); }
    }
}

// swnerf_gemm_tn_group in bf16x3 arithmetic.  The main 256 x 256 GEMM of every item the LDS-DMA plan can take (the first 16 of
// them) goes into ONE launch of the kernel above, the ~256 workgroups dealt out evenly (the items are equal work here).  Everything
// else keeps the fp32 route and fp32 results: an item that does not qualify (alignment, M < 4096) or exceeds the 16 runs as
// swnerf_gemm_tn_fused runs it; the B2 rider (<= 64 unaligned columns, ld 90) and the A2 rider are swnerf_gemm_tn launches - a
// fifth accumulator tile for the rider does not fit the 128-register budget next to the split operands.
extern "C" int swnerf_gemm_tn_group_x3(const swnerf_gemm_item* items, int n_items, int64_t M, void* stream) {
    if (M == 0 || n_items == 0) return 0;
    if (!items || n_items < 0 || M < 0) return sw_fail(SWNERF_E_ARG, "gemm_tn_group_x3: NULL items / negative count");
    for (int k = 0; k < n_items; ++k)
        if (const char* bad = fused_item_bad(&items[k])) {
            const swnerf_gemm_item& q = items[k];
            return sw_fail(SWNERF_E_ARG, "gemm_tn_group_x3: item %d: bad %s (lda=%d ldb=%d ldc=%d Ni2=%d No2=%d)", k, bad, q.lda, q.ldb, q.ldc, q.Ni2, q.No2);
        }
    X3Group G;
    G.n = 0;
    G.M = M;
    for (int k = 0; k < n_items; ++k) {
        const swnerf_gemm_item& q = items[k];
        int rc;
        if (!fused_item_takes_dma(&q, M) || G.n == X3W_MAX) {
            rc = swnerf_gemm_tn_fused(q.A, q.lda, q.B, q.ldb, M, q.C, q.ldc, q.bias, q.B2, q.ldb2, q.Ni2, q.C2, q.ldc2,
                                      q.A2, q.lda2, q.No2, q.C3, q.ldc3, q.bias3, stream);
            if (rc) return rc;
            continue;
        }
        if (q.B2 && (rc = swnerf_gemm_tn(q.A, q.lda, 256, q.B2, q.ldb2, q.Ni2, M, q.C2, q.ldc2, nullptr, stream))) return rc;
        if (q.A2 && (rc = swnerf_gemm_tn(q.A2, q.lda2, q.No2, q.B, q.ldb, 256, M, q.C3, q.ldc3, q.bias3, stream))) return rc;
        X3Item& P = G.it[G.n++];
        P.A = q.A; P.lda = q.lda; P.B = q.B; P.ldb = q.ldb; P.C = q.C; P.ldc = q.ldc; P.bias = q.bias;
    }
    if (G.n == 0) return 0;
    int total = 0;
    G.wg0[0] = 0;
    for (int k = 0; k < G.n; ++k) {
        const RowSplit sp = split_rows(M, X3W_WG_TARGET / G.n, X3W_SLAB);
        G.it[k].rows_per_wg = sp.rows_per_wg;
        total += (int)sp.nwg;
        G.wg0[k + 1] = total;
    }
    hipLaunchKernelGGL(gemm_tn_x3_group_kernel, dim3((unsigned)total), dim3(1024), 2 * X3W_BUF_FLOATS * sizeof(float), (hipStream_t)stream, G);
    return sw_check(hipGetLastError(), "gemm_tn_group_x3 launch");
}
