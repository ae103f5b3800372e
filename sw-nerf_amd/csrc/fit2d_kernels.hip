// fit2d_kernels.hip - 2-D image fitting (2d_pos_encoding/) for gfx950 (MI355X): the positional encoder, BatchNorm1d
// (training forward / backward, eval form), the fitting loss, the weight pack and the fused eval pass.
//
// The net (2d_pos_encoding/model.py:6-43) is n_layers x (Linear -> ReLU -> BatchNorm1d) at width 256 and Linear(256, 3) on
// encode(pos, L) (encoding.py:22-40, 4L + 2 columns).  In eval mode BatchNorm1d is the affine map x.s + t behind the ReLU; the
// pack kernel folds it into the NEXT Linear (W.diag(s), b + W.t: fp64 product, one rounding), so the fused pass is a plain ReLU
// trunk: layer 0 on three 32-column k-tiles of the encoding, n_layers - 1 segments of 8 x 8 tiles, the 3-output head on the
// VALU - mlp_core.h's seg_mfma / head_valu with one wave per 32-pixel tile.  DESIGN.md 6h.
//
// A fused TRAINING pass is not built: batch statistics couple all rows of a batch at every layer, so a wave cannot own its rows
// from input to loss.  Training runs layer by layer: swnerf_linear, then swnerf_bn_forward_train with the ReLU in front.
#include <hip/hip_runtime.h>
#include "../../include/swnerf.h"
#include "swnerf_common.h"
#include "host_util.h"
#include "render_pass.h"
#include "fit2d_cols.h"

// ---- the encoder (the slot map sw_fit2d_col and SW_F2_MAX_L: fit2d_cols.h) --------------------------------------------
#define SW_F2_MAX_LAYERS 64                // bias-style tiles of the whole net sit in LDS (1 KiB per layer)
#define SW_F2_L0_STEPS 96                  // 8 n-tiles x 3 k-tiles

// xn = 2 * (p / max) - 1: a correctly rounded division and two more roundings (encoding.py:27; -ffp-contract=off)
__device__ __forceinline__ float fit2d_normalise(float p, float maxv) { return 2.f * (p / maxv) - 1.f; }

// the 47 values of one coordinate in slot order: sin / cos of fl32(2^i pi) * xn as ONE fp32 product (encoding.py:33-38: the
// scalar 2**i * np.pi enters the tensor product as a float), the double-precision reduction for every band, then xn itself
__device__ __forceinline__ void fit2d_encode(float xn, int L, f32x16 (&e)[3]) {
#pragma unroll
    for (int i = 0; i < SW_F2_MAX_L; ++i) {
        float s = 0.f, c = 0.f;
        if (i < L) sw_sincos_pair_wide((3.14159274101257324f * (float)(1 << i)) * xn, &s, &c);     // 2^i * fl32(pi) is exact
        e[(2 * i) >> 4][(2 * i) & 15] = s;
        e[(2 * i + 1) >> 4][(2 * i + 1) & 15] = c;
    }
    e[2][14] = xn;
    e[2][15] = 0.f;
}

__global__ void __launch_bounds__(256) encode2d_kernel(const float* pos, int64_t N, float max_x, float max_y, int L, float* out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;           // (row, coordinate)
    if (idx >= 2 * N) return;
    const int64_t row = idx >> 1;
    const int h = (int)(idx & 1);
    f32x16 e[3];
    fit2d_encode(fit2d_normalise(pos[idx], h ? max_y : max_x), L, e);
    float* o = out + row * (4 * L + 2);
#pragma unroll
    for (int a = 0; a < 48; ++a) {
        const int col = sw_fit2d_col(a, h, L);
        if (col >= 0) o[col] = e[a >> 4][a & 15];
    }
}

extern "C" int swnerf_encode2d(const float* pos, int64_t N, float max_x, float max_y, int L, float* out, void* stream) {
    if (L < 0 || L > SW_F2_MAX_L) return sw_fail(SWNERF_E_ARG, "encode2d: L %d outside 0..%d", L, SW_F2_MAX_L);
    if (!(max_x > 0.f) || !(max_y > 0.f))
        return sw_fail(SWNERF_E_ARG, "encode2d: max_x %g, max_y %g must be > 0 (a 1-pixel-wide picture divides by zero in the reference)", max_x, max_y);
    if (N < 0) return sw_fail(SWNERF_E_ARG, "encode2d: negative N");
    if (N == 0) return 0;
    if (!pos || !out) return sw_fail(SWNERF_E_ARG, "encode2d: NULL pointer");
    hipLaunchKernelGGL(encode2d_kernel, dim3((unsigned)((2 * N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pos, N, max_x, max_y, L, out);
    return sw_check(hipGetLastError(), "encode2d launch");
}

// ---- BatchNorm1d on [M, C] rows -------------------------------------------------------------------------------------
// Column sums in fp64, in a fixed order, no atomics.  A workgroup is CB columns x 256 / CB row phases: thread (ph, c) adds its
// rows r0 + ph, r0 + ph + NPH, ... in order, the phases are added in phase order through LDS.  M <= SW_BN_ONE_M: ONE launch per
// direction (a workgroup owns 16 columns over all rows: sums, finish, then the elementwise part, the rows still in L2);
// above it the rows are split into slabs over the grid's y dimension: partial sums into the workspace, a second stage that adds
// the slabs in slab order, and the elementwise launch.
#define SW_BN_ONE_M 512
#define SW_BN_MAX_SLABS 1024
#define SW_BN_SLAB_ROWS 256

// v0 / v1: this thread's two summands of row r; returns (in every thread of phase 0) the block's column sums
template <int CB, class F>
__device__ __forceinline__ void bn_col_sums(int64_t r0, int64_t r1, int c, bool cok, F f, double (*lds)[2][CB], double& s0, double& s1) {
    constexpr int NPH = 256 / CB;
    const int ph = threadIdx.x / CB, cc = threadIdx.x % CB;
    double a0 = 0.0, a1 = 0.0;
    if (cok)
        for (int64_t r = r0 + ph; r < r1; r += NPH) {
            double v0, v1;
            f(r, c, v0, v1);
            a0 += v0; a1 += v1;
        }
    lds[ph][0][cc] = a0; lds[ph][1][cc] = a1;
    __syncthreads();
    s0 = 0.0; s1 = 0.0;
#pragma unroll
    for (int p = 0; p < NPH; ++p) { s0 += lds[p][0][cc]; s1 += lds[p][1][cc]; }
    __syncthreads();
}

struct BnDev {
    const float* a; const float* dy; int64_t M; int C; int relu;
    const float* gamma; const float* beta; double eps, momentum;
    float* y; float* mean; float* invstd; float* rmean; float* rvar;
    float* dx; float* dgamma; float* dbeta;
    double* ws; int nslab; int64_t slab_rows;
};

__device__ __forceinline__ float bn_in(const BnDev& P, int64_t r, int c) {
    const float v = P.a[r * P.C + c];
    return P.relu ? fmaxf(v, 0.f) : v;
}

// column c's statistics from its sums: saved mean / invstd, running buffers (momentum; the unbiased variance, as torch)
__device__ __forceinline__ void bn_finish_fwd(const BnDev& P, int c, double s, double ss, float& mu, float& is) {
    const double m = s / (double)P.M;
    double var = ss / (double)P.M - m * m;
    var = var > 0.0 ? var : 0.0;
    mu = (float)m;
    is = (float)(1.0 / sqrt(var + P.eps));
    P.mean[c] = mu; P.invstd[c] = is;
    if (P.rmean) {
        const double unb = var * ((double)P.M / (double)(P.M - 1));
        P.rmean[c] = (float)((1.0 - P.momentum) * (double)P.rmean[c] + P.momentum * m);
        P.rvar[c] = (float)((1.0 - P.momentum) * (double)P.rvar[c] + P.momentum * unb);
    }
}

__device__ __forceinline__ float bn_norm(float x, float mu, float is, float g, float b) { return g * ((x - mu) * is) + b; }

__device__ __forceinline__ float bn_dx(const BnDev& P, int64_t r, int c, float mu, float is, float g, float db, float dg) {
    const float a = P.a[r * P.C + c];
    const float xh = ((P.relu ? fmaxf(a, 0.f) : a) - mu) * is;
    const float Mf = (float)P.M;
    const float v = (g * is / Mf) * (Mf * P.dy[r * P.C + c] - db - xh * dg);
    return (P.relu && !(a > 0.f)) ? 0.f : v;
}

template <bool BWD>
__global__ void __launch_bounds__(256) bn_one_kernel(BnDev P) {
    constexpr int CB = 16, NPH = 16;
    __shared__ double lds[NPH][2][CB];
    __shared__ float st[2][CB];
    const int ph = threadIdx.x / CB, cc = threadIdx.x % CB;
    const int c = blockIdx.x * CB + cc;
    const bool cok = c < P.C;
    double s0, s1;
    if (!BWD) {
        bn_col_sums<CB>(0, P.M, c, cok, [&](int64_t r, int c_, double& v0, double& v1) {
            const double x = (double)bn_in(P, r, c_); v0 = x; v1 = x * x; }, lds, s0, s1);
        if (ph == 0 && cok) { float mu, is; bn_finish_fwd(P, c, s0, s1, mu, is); st[0][cc] = mu; st[1][cc] = is; }
        __syncthreads();
        if (!cok) return;
        const float mu = st[0][cc], is = st[1][cc], g = P.gamma[c], b = P.beta[c];
        for (int64_t r = ph; r < P.M; r += NPH) P.y[r * P.C + c] = bn_norm(bn_in(P, r, c), mu, is, g, b);
    } else {
        const float mu = cok ? P.mean[c] : 0.f, is = cok ? P.invstd[c] : 0.f;
        bn_col_sums<CB>(0, P.M, c, cok, [&](int64_t r, int c_, double& v0, double& v1) {
            const float d = P.dy[r * P.C + c_]; v0 = (double)d; v1 = (double)(d * ((bn_in(P, r, c_) - mu) * is)); }, lds, s0, s1);
        if (ph == 0 && cok) { st[0][cc] = (float)s0; st[1][cc] = (float)s1; P.dbeta[c] = (float)s0; P.dgamma[c] = (float)s1; }
        __syncthreads();
        if (!cok) return;
        const float db = st[0][cc], dg = st[1][cc], g = P.gamma[c];
        for (int64_t r = ph; r < P.M; r += NPH) P.dx[r * P.C + c] = bn_dx(P, r, c, mu, is, g, db, dg);
    }
}

// split path, stage 1: slab blockIdx.y, columns 64 * blockIdx.x ..: partial sums -> ws[slab][2][C]
template <bool BWD>
__global__ void __launch_bounds__(256) bn_partial_kernel(BnDev P) {
    constexpr int CB = 64, NPH = 4;
    __shared__ double lds[NPH][2][CB];
    const int ph = threadIdx.x / CB, cc = threadIdx.x % CB;
    const int c = blockIdx.x * CB + cc;
    const bool cok = c < P.C;
    const int64_t r0 = (int64_t)blockIdx.y * P.slab_rows, r1 = r0 + P.slab_rows < P.M ? r0 + P.slab_rows : P.M;
    double s0, s1;
    if (!BWD) {
        bn_col_sums<CB>(r0, r1, c, cok, [&](int64_t r, int c_, double& v0, double& v1) {
            const double x = (double)bn_in(P, r, c_); v0 = x; v1 = x * x; }, lds, s0, s1);
    } else {
        const float mu = cok ? P.mean[c] : 0.f, is = cok ? P.invstd[c] : 0.f;
        bn_col_sums<CB>(r0, r1, c, cok, [&](int64_t r, int c_, double& v0, double& v1) {
            const float d = P.dy[r * P.C + c_]; v0 = (double)d; v1 = (double)(d * ((bn_in(P, r, c_) - mu) * is)); }, lds, s0, s1);
    }
    if (ph == 0 && cok) {
        double* w = P.ws + (size_t)blockIdx.y * 2 * P.C;
        w[c] = s0; w[P.C + c] = s1;
    }
}

// stage 2: one thread per column adds the slabs in slab order
template <bool BWD>
__global__ void __launch_bounds__(256) bn_final_kernel(BnDev P) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= P.C) return;
    double s0 = 0.0, s1 = 0.0;
    for (int s = 0; s < P.nslab; ++s) { s0 += P.ws[(size_t)s * 2 * P.C + c]; s1 += P.ws[(size_t)s * 2 * P.C + P.C + c]; }
    if (!BWD) { float mu, is; bn_finish_fwd(P, c, s0, s1, mu, is); }
    else { P.dbeta[c] = (float)s0; P.dgamma[c] = (float)s1; }
}

// stage 3: the elementwise part
template <bool BWD>
__global__ void __launch_bounds__(256) bn_apply_saved_kernel(BnDev P) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= P.M * P.C) return;
    const int64_t r = idx / P.C;
    const int c = (int)(idx - r * P.C);
    if (!BWD) P.y[idx] = bn_norm(bn_in(P, r, c), P.mean[c], P.invstd[c], P.gamma[c], P.beta[c]);
    else P.dx[idx] = bn_dx(P, r, c, P.mean[c], P.invstd[c], P.gamma[c], P.dbeta[c], P.dgamma[c]);
}

static void bn_split(int64_t M, int* nslab, int64_t* slab_rows) {
    int64_t rows = SW_BN_SLAB_ROWS;
    if ((M + rows - 1) / rows > SW_BN_MAX_SLABS) rows = (M + SW_BN_MAX_SLABS - 1) / SW_BN_MAX_SLABS;
    *slab_rows = rows;
    *nslab = (int)((M + rows - 1) / rows);
}

extern "C" size_t swnerf_bn_workspace_bytes(int64_t M, int C) {
    if (M <= SW_BN_ONE_M || C < 1) return 0;
    int nslab; int64_t rows;
    bn_split(M, &nslab, &rows);
    return (size_t)nslab * 2 * (size_t)C * sizeof(double);
}

template <bool BWD>
static int bn_launch(BnDev& P, const char* what, hipStream_t st) {
    if (P.M <= SW_BN_ONE_M) {
        hipLaunchKernelGGL(bn_one_kernel<BWD>, dim3((unsigned)((P.C + 15) / 16)), dim3(256), 0, st, P);
        return sw_check(hipGetLastError(), what);
    }
    if (!P.ws) return sw_fail(SWNERF_E_ARG, "%s: M %lld > %d needs the workspace of swnerf_bn_workspace_bytes", what, (long long)P.M, SW_BN_ONE_M);
    bn_split(P.M, &P.nslab, &P.slab_rows);
    hipLaunchKernelGGL(bn_partial_kernel<BWD>, dim3((unsigned)((P.C + 63) / 64), (unsigned)P.nslab), dim3(256), 0, st, P);
    hipLaunchKernelGGL(bn_final_kernel<BWD>, dim3((unsigned)((P.C + 255) / 256)), dim3(256), 0, st, P);
    hipLaunchKernelGGL(bn_apply_saved_kernel<BWD>, dim3((unsigned)((P.M * P.C + 255) / 256)), dim3(256), 0, st, P);
    return sw_check(hipGetLastError(), what);
}

static int bn_shape(const char* what, int64_t M, int C) {
    if (C < 1 || M < 0) return sw_fail(SWNERF_E_ARG, "%s: M %lld, C %d", what, (long long)M, C);
    if (M < 2) return sw_fail(SWNERF_E_ARG, "%s: batch statistics need M >= 2 rows (got %lld), as torch's BatchNorm1d", what, (long long)M);
    if (M * (int64_t)C > ((int64_t)1 << 40)) return sw_fail(SWNERF_E_ARG, "%s: M * C too large", what);
    return 0;
}

extern "C" int swnerf_bn_forward_train(const float* a, int64_t M, int C, int relu, const float* gamma, const float* beta, double eps,
                                       double momentum, float* y, float* save_mean, float* save_invstd, float* running_mean,
                                       float* running_var, void* ws, void* stream) {
    int rc = bn_shape("bn_forward_train", M, C);
    if (rc) return rc;
    if (!a || !gamma || !beta || !y || !save_mean || !save_invstd || (!running_mean) != (!running_var))
        return sw_fail(SWNERF_E_ARG, "bn_forward_train: NULL pointer");
    if (!(eps >= 0.0) || !(momentum >= 0.0 && momentum <= 1.0)) return sw_fail(SWNERF_E_ARG, "bn_forward_train: eps %g, momentum %g", eps, momentum);
    BnDev P = {};
    P.a = a; P.M = M; P.C = C; P.relu = relu ? 1 : 0; P.gamma = gamma; P.beta = beta; P.eps = eps; P.momentum = momentum;
    P.y = y; P.mean = save_mean; P.invstd = save_invstd; P.rmean = running_mean; P.rvar = running_var; P.ws = (double*)ws;
    return bn_launch<false>(P, "bn_forward_train", (hipStream_t)stream);
}

extern "C" int swnerf_bn_backward(const float* dy, const float* a, int64_t M, int C, int relu, const float* gamma, const float* save_mean,
                                  const float* save_invstd, float* dx, float* dgamma, float* dbeta, void* ws, void* stream) {
    int rc = bn_shape("bn_backward", M, C);
    if (rc) return rc;
    if (!dy || !a || !gamma || !save_mean || !save_invstd || !dx || !dgamma || !dbeta) return sw_fail(SWNERF_E_ARG, "bn_backward: NULL pointer");
    BnDev P = {};
    P.a = a; P.dy = dy; P.M = M; P.C = C; P.relu = relu ? 1 : 0; P.gamma = gamma;
    P.mean = const_cast<float*>(save_mean); P.invstd = const_cast<float*>(save_invstd);
    P.dx = dx; P.dgamma = dgamma; P.dbeta = dbeta; P.ws = (double*)ws;
    return bn_launch<true>(P, "bn_backward", (hipStream_t)stream);
}

// eval form: y = x . s + t with s = gamma / sqrt(running_var + eps), t = beta - running_mean . s (s, t formed in fp64, rounded once)
__global__ void __launch_bounds__(256) bn_apply_kernel(const float* x, int64_t M, int C, int relu, const float* gamma, const float* beta,
                                                       const float* rmean, const float* rvar, double eps, float* y) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= M * C) return;
    const int c = (int)(idx % C);
    const double s = (double)gamma[c] / sqrt((double)rvar[c] + eps);
    const float sf = (float)s, tf = (float)((double)beta[c] - (double)rmean[c] * s);
    const float v = x[idx];
    y[idx] = fmaf(relu ? fmaxf(v, 0.f) : v, sf, tf);
}

extern "C" int swnerf_bn_apply(const float* x, int64_t M, int C, int relu, const float* gamma, const float* beta, const float* running_mean,
                               const float* running_var, double eps, float* y, void* stream) {
    if (C < 1 || M < 0 || M * (int64_t)C > ((int64_t)1 << 40)) return sw_fail(SWNERF_E_ARG, "bn_apply: M %lld, C %d", (long long)M, C);
    if (!(eps >= 0.0)) return sw_fail(SWNERF_E_ARG, "bn_apply: eps %g", eps);
    if (M == 0) return 0;
    if (!x || !gamma || !beta || !running_mean || !running_var || !y) return sw_fail(SWNERF_E_ARG, "bn_apply: NULL pointer");
    hipLaunchKernelGGL(bn_apply_kernel, dim3((unsigned)((M * C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, M, C, relu ? 1 : 0,
                       gamma, beta, running_mean, running_var, eps, y);
    return sw_check(hipGetLastError(), "bn_apply launch");
}

// ---- the fitting loss (2d_pos_encoding/utils.py:13,56,62-64) --------------------------------------------------------
// sums[0] = mse(out, target) + reg * mean(max(max(0, x - 1), max(-x, 0))), sums[1] = the grey-scale mse; grad = d sums[0] / d out.
// ONE workgroup (the batches are 512 rows): thread t adds elements t, t + 1024, ... in fp64, then the 1024 partial sums are
// added in a fixed tree.  At the ties x == 0 and x == 1 the clip term's subgradient is 0 here (torch: 0.25 reg / (3M)).
__global__ void __launch_bounds__(1024) fit2d_loss_kernel(const float* out, const float* tgt, int64_t M, float reg, double* sums, float* grad) {
    __shared__ double red[3][1024];
    const int t = threadIdx.x;
    const int64_t n = 3 * M;
    const float inv = 1.f / (float)n;
    double sq = 0.0, cl = 0.0, gr = 0.0;
    for (int64_t e = t; e < n; e += 1024) {
        const float x = out[e], d = x - tgt[e];
        sq += (double)d * (double)d;
        cl += (double)fmaxf(fmaxf(0.f, x - 1.f), fmaxf(-x, 0.f));
        if (grad) grad[e] = (2.f * d) * inv + (x > 1.f ? reg * inv : (x < 0.f ? -reg * inv : 0.f));
    }
    for (int64_t r = t; r < M; r += 1024) {
        const float go = 0.2989f * out[3 * r] + 0.5870f * out[3 * r + 1] + 0.1140f * out[3 * r + 2];
        const float gt = 0.2989f * tgt[3 * r] + 0.5870f * tgt[3 * r + 1] + 0.1140f * tgt[3 * r + 2];
        const float d = go - gt;
        gr += (double)d * (double)d;
    }
    red[0][t] = sq; red[1][t] = cl; red[2][t] = gr;
    __syncthreads();
    for (int w = 512; w >= 1; w >>= 1) {
        if (t < w) { red[0][t] += red[0][t + w]; red[1][t] += red[1][t + w]; red[2][t] += red[2][t + w]; }
        __syncthreads();
    }
    if (t == 0) {
        sums[0] = red[0][0] / (double)n + (double)reg * (red[1][0] / (double)n);
        sums[1] = red[2][0] / (double)M;
    }
}

extern "C" int swnerf_fit2d_loss(const float* out, const float* target, int64_t M, float reg, double* sums, float* grad, void* stream) {
    if (M < 1 || M > ((int64_t)1 << 32)) return sw_fail(SWNERF_E_ARG, "fit2d_loss: M %lld", (long long)M);
    if (!out || !target || !sums) return sw_fail(SWNERF_E_ARG, "fit2d_loss: NULL pointer");
    hipLaunchKernelGGL(fit2d_loss_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, out, target, M, reg, sums, grad);
    return sw_check(hipGetLastError(), "fit2d_loss launch");
}

// ---- pack: BatchNorm folded into the next Linear, MFMA-fragment order (pack_kernels.hip) -------------------------------
// blob: [L0: 8 x 3 tiles][n_layers - 1 blocks of 8 x 8][ring tail = L0's first SW_TAIL steps] then the bias-style tiles:
// 8 per layer | head weight 3 x 8 | 1 head-bias tile.  params (HOST array of DEVICE pointers): per hidden layer l
// [6l..6l+5] = Linear weight, bias, BatchNorm weight, bias, running_mean, running_var; then [6n], [6n+1] = head weight, bias.
#define SW_F2_STEPS(n) (SW_F2_L0_STEPS + ((n) - 1) * SW_STEPS_TRUNK)
#define SW_F2_W_FLOATS(n) ((size_t)(SW_F2_STEPS(n) + SW_TAIL) * SW_STEP_FLOATS)
#define SW_F2_BIAS_TILES(n) (8 * (n) + 24 + 1)
struct F2Layer { const float* W; const float* b; const float* g; const float* be; const float* rm; const float* rv; };
struct F2PackDev { int n_layers, L, K0; double eps; float* packed; F2Layer layers[SW_F2_MAX_LAYERS + 1]; };
static_assert(sizeof(F2PackDev) <= 3800, "the tensor table must fit the kernel-argument segment");

// s_k, t_k of the BatchNorm behind layer l (fp64)
__device__ __forceinline__ void f2_st(const F2Layer& y, int k, double eps, double& s, double& t) {
    s = (double)y.g[k] / sqrt((double)y.rv[k] + eps);
    t = (double)y.be[k] - (double)y.rm[k] * s;
}

__global__ void __launch_bounds__(256) pack_fit2d_w_kernel(F2PackDev P) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)SW_F2_W_FLOATS(P.n_layers);
    if (e >= total) return;
    int64_t step = e / SW_STEP_FLOATS;
    const int rem = (int)(e % SW_STEP_FLOATS);
    if (step >= SW_F2_STEPS(P.n_layers)) step -= SW_F2_STEPS(P.n_layers);        // the ring tail: the head of L0 once more
    const int lane = rem >> 2, i4 = rem & 3, i = lane & 31, h = lane >> 5;
    float v = 0.f;
    if (step < SW_F2_L0_STEPS) {
        const int s = (int)step, n = s / 12, kt = (s >> 2) % 3, q = s & 3;
        const int col = sw_fit2d_col(16 * kt + 4 * q + i4, h, P.L);
        if (col >= 0) v = P.layers[0].W[(size_t)(32 * n + i) * P.K0 + col];
    } else {
        const int l = 1 + (int)((step - SW_F2_L0_STEPS) / SW_STEPS_TRUNK), s = (int)((step - SW_F2_L0_STEPS) % SW_STEPS_TRUNK);
        const int n = s / 32, kt = (s >> 2) & 7, q = s & 3;
        const int col = 32 * kt + sw_frow(4 * q + i4, h);
        double sc, t;
        f2_st(P.layers[l - 1], col, P.eps, sc, t);
        v = (float)((double)P.layers[l].W[(size_t)(32 * n + i) * 256 + col] * sc);
    }
    P.packed[e] = v;
}

// bias-style tiles.  Block = one output row (64 lanes): b'[o] = b[o] + sum_k W[o][k] t[k] in fp64 (lane: 4 terms in order, then a
// fixed xor tree), one rounding; the head's block also writes its folded weight row as 8 tiles.
__global__ void __launch_bounds__(64) pack_fit2d_b_kernel(F2PackDev P) {
    const int l = blockIdx.x / 256, o = blockIdx.x % 256, lane = threadIdx.x;
    const bool head = l == P.n_layers;
    if (head && o >= 3) return;
    const F2Layer& y = P.layers[l];
    float* tiles = P.packed + SW_F2_W_FLOATS(P.n_layers);
    double acc = 0.0;
    if (l > 0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = lane + 64 * u;
            double s, t;
            f2_st(P.layers[l - 1], k, P.eps, s, t);
            const double w = (double)y.W[(size_t)o * 256 + k];
            acc += w * t;
            if (head) {                                   // tile (o, n): [h][r] = W'[o][32n + frow(r, h)]
                const int n = k >> 5, f = k & 31, hh = (f >> 2) & 1, r = (f & 3) + 4 * (f >> 3);
                tiles[(8 * P.n_layers + o * 8 + n) * SW_BIAS_TILE_FLOATS + hh * 16 + r] = (float)(w * s);
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    }
    if (lane != 0) return;
    const float bv = (float)((double)y.b[o] + acc);
    if (head) {
        float* hb = tiles + (8 * P.n_layers + 24) * SW_BIAS_TILE_FLOATS;
        hb[o] = bv; hb[16 + o] = bv;
        if (o == 0) for (int r = 3; r < 16; ++r) { hb[r] = 0.f; hb[16 + r] = 0.f; }
    } else {
        const int n = o >> 5, f = o & 31, hh = (f >> 2) & 1, r = (f & 3) + 4 * (f >> 3);
        tiles[(8 * l + n) * SW_BIAS_TILE_FLOATS + hh * 16 + r] = bv;
    }
}

static int f2_shape(const char* what, int L, int n_layers) {
    if (L < 0 || L > SW_F2_MAX_L) return sw_fail(SWNERF_E_ARG, "%s: L %d outside 0..%d (the encoding is held in three 32-column k-tiles)", what, L, SW_F2_MAX_L);
    if (n_layers < 1) return sw_fail(SWNERF_E_ARG, "%s: n_layers %d < 1", what, n_layers);
    if (n_layers > SW_F2_MAX_LAYERS) return sw_fail(SWNERF_E_UNSUPP, "%s: n_layers %d > %d (bias tiles exceed the LDS)", what, n_layers, SW_F2_MAX_LAYERS);
    return 0;
}

extern "C" size_t swnerf_fit2d_packed_floats(int n_layers) {
    if (n_layers < 1 || n_layers > SW_F2_MAX_LAYERS) return 0;
    return SW_F2_W_FLOATS(n_layers) + (size_t)SW_F2_BIAS_TILES(n_layers) * SW_BIAS_TILE_FLOATS;
}

extern "C" int swnerf_pack_fit2d(const float* const* params /*HOST*/, int n_layers, int L, double eps, float* packed, void* stream) {
    int rc = f2_shape("pack_fit2d", L, n_layers);
    if (rc) return rc;
    if (!(eps >= 0.0)) return sw_fail(SWNERF_E_ARG, "pack_fit2d: eps %g", eps);
    if (!params || !packed) return sw_fail(SWNERF_E_ARG, "pack_fit2d: NULL pointer");
    for (int i = 0; i < 6 * n_layers + 2; ++i) if (!params[i]) return sw_fail(SWNERF_E_ARG, "pack_fit2d: params[%d] is NULL", i);
    hipStream_t st = (hipStream_t)stream;
    F2PackDev P = {};
    F2Layer* host = P.layers;
    for (int l = 0; l <= n_layers; ++l) {
        const float* const* p = params + 6 * l;
        host[l].W = p[0]; host[l].b = p[1];
        host[l].g = l < n_layers ? p[2] : nullptr; host[l].be = l < n_layers ? p[3] : nullptr;
        host[l].rm = l < n_layers ? p[4] : nullptr; host[l].rv = l < n_layers ? p[5] : nullptr;
    }
    P.n_layers = n_layers; P.L = L; P.K0 = 4 * L + 2; P.eps = eps; P.packed = packed;
    const size_t total = SW_F2_W_FLOATS(n_layers);
    hipLaunchKernelGGL(pack_fit2d_w_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, P);
    hipLaunchKernelGGL(pack_fit2d_b_kernel, dim3((unsigned)(256 * n_layers + 3)), dim3(64), 0, st, P);
    return sw_check(hipGetLastError(), "pack_fit2d launch");
}

// ---- the fused eval pass: one wave per 32-pixel tile, four waves per workgroup ---------------------------------------
struct Fit2dDev {
    PassDev S;                      // only the start-up shaping fields are used (render_pass.h pass_startup)
    const float* w0; const float* b0; int nbias;
    const float* x; int ldx; int64_t M; int L, n_layers;
    int64_t W; float max_x, max_y;  // PICTURE: row length, W - 1, H - 1
    float* out; unsigned char* out_u8;
};

// LDS: bias-style tiles | per wave: weight ring + 1 KiB junk slot of the L2 warm-up
#define SW_F2_WAVE_FLOATS ((SW_RING + 1) * SW_STEP_FLOATS)

template <bool PICTURE>
__global__ void __launch_bounds__(256, 1) fit2d_kernel(Fit2dDev P) {
    extern __shared__ __attribute__((aligned(16))) float lds_all[];
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* lds_ring = lds_all + P.nbias + wv * SW_F2_WAVE_FLOATS;
    const int64_t tile = (int64_t)blockIdx.x * 4 + wv;
    pass_startup(P.S, P.w0, lds_ring + SW_RING * SW_STEP_FLOATS, lane, wv);
    bias_to_lds(lds_all, P.b0, P.nbias);         // the only block barrier
    if (tile * 32 >= P.M) return;                // wave-uniform
    const int64_t row = tile * 32 + j;
    const bool live = row < P.M;
    const int64_t rr = live ? row : P.M - 1;

    WStream ws;
    ws_start(ws, P.w0, lds_all, lds_ring, lane);
    f32x16 emb[3], in[8], out[8];
    if constexpr (PICTURE) {
        // pixel rr = (x, y) = (rr % W, rr / W); this lane half encodes its coordinate (get_picture, utils.py:110-114)
        const int64_t py = rr / P.W, px = rr - py * P.W;
        fit2d_encode(fit2d_normalise(h ? (float)py : (float)px, h ? P.max_y : P.max_x), P.L, emb);
    } else {
        const float* xr = P.x + rr * P.ldx;
#pragma unroll
        for (int a = 0; a < 48; ++a) {
            const int col = sw_fit2d_col(a, h, P.L);
            emb[a >> 4][a & 15] = (col >= 0) ? xr[col] : 0.f;
        }
    }
    seg_mfma<8, 3, SEG_BIAS>(out, emb, ws);
#pragma unroll
    for (int n = 0; n < 8; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) in[n][r] = relu1(out[n][r]);
#pragma nounroll
    for (int l = 1; l < P.n_layers; ++l) {
        seg_mfma<8, 8, SEG_BIAS>(out, in, ws);
#pragma unroll
        for (int n = 0; n < 8; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) in[n][r] = relu1(out[n][r]);
    }
    float c3[3];
    head_valu<3, 8>(in, ws, c3);
    c3[0] += ws.bias[0]; c3[1] += ws.bias[1]; c3[2] += ws.bias[2];
    if (!live || h != 0) return;
    if constexpr (PICTURE) {
        // np.clip(picture, 0, 1) (utils.py:124); bytes = to8b: (255 * clip).astype(uint8)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = fminf(fmaxf(c3[c], 0.f), 1.f);
            if (P.out) P.out[row * 3 + c] = v;
            if (P.out_u8) P.out_u8[row * 3 + c] = (unsigned char)(255.f * v);
        }
    } else {
        P.out[row * 3 + 0] = c3[0]; P.out[row * 3 + 1] = c3[1]; P.out[row * 3 + 2] = c3[2];
    }
}

template <bool PICTURE>
static int fit2d_launch(Fit2dDev& P, const float* packed, const char* what, hipStream_t st) {
    P.S = pass_dev(swnerf_pass_args{});
    P.w0 = packed;
    P.b0 = packed + SW_F2_W_FLOATS(P.n_layers);
    P.nbias = SW_F2_BIAS_TILES(P.n_layers) * SW_BIAS_TILE_FLOATS;
    const dim3 grid((unsigned)((P.M + 127) / 128)), block(256);
    pass_startup_args(P.S, grid.x, SW_F2_STEPS(P.n_layers));
    const size_t lds = ((size_t)P.nbias + 4 * SW_F2_WAVE_FLOATS) * sizeof(float);
    hipLaunchKernelGGL(fit2d_kernel<PICTURE>, grid, block, lds, st, P);
    return sw_check(hipGetLastError(), what);
}

extern "C" int swnerf_fit2d_forward(const float* packed, const float* x, int64_t M, int ldx, int L, int n_layers, float* out, void* stream) {
    int rc = f2_shape("fit2d_forward", L, n_layers);
    if (rc) return rc;
    if (M < 0 || M > ((int64_t)1 << 36)) return sw_fail(SWNERF_E_ARG, "fit2d_forward: M %lld", (long long)M);
    if (ldx < 4 * L + 2) return sw_fail(SWNERF_E_ARG, "fit2d_forward: rows of %d floats cannot hold %d encoded columns", ldx, 4 * L + 2);
    if (M == 0) return 0;
    if (!packed || !x || !out) return sw_fail(SWNERF_E_ARG, "fit2d_forward: NULL pointer");
    Fit2dDev P = {};
    P.x = x; P.ldx = ldx; P.M = M; P.L = L; P.n_layers = n_layers; P.out = out;
    return fit2d_launch<false>(P, packed, "fit2d_forward launch", (hipStream_t)stream);
}

extern "C" int swnerf_fit2d_picture(const float* packed, int64_t H, int64_t W, int L, int n_layers, float* out_f32, unsigned char* out_u8,
                                    void* stream) {
    int rc = f2_shape("fit2d_picture", L, n_layers);
    if (rc) return rc;
    if (H < 2 || W < 2 || H > (1 << 20) || W > (1 << 20))
        return sw_fail(SWNERF_E_ARG, "fit2d_picture: %lld x %lld (both sides 2..2^20: the reference divides by zero for a 1-pixel-wide picture)", (long long)H, (long long)W);
    if (!out_f32 && !out_u8) return sw_fail(SWNERF_E_ARG, "fit2d_picture: out_f32 and out_u8 are both NULL");
    if (!packed) return sw_fail(SWNERF_E_ARG, "fit2d_picture: NULL pointer");
    Fit2dDev P = {};
    P.M = H * W; P.L = L; P.n_layers = n_layers; P.W = W; P.max_x = (float)(W - 1); P.max_y = (float)(H - 1);
    P.out = out_f32; P.out_u8 = out_u8;
    return fit2d_launch<true>(P, packed, "fit2d_picture launch", (hipStream_t)stream);
}
