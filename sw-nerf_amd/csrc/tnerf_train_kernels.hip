// tnerf_train_kernels.hip - the fused T-NeRF training pass for gfx950 (MI355X): ONE wavefront owns ONE ray, forward and backward.
//
// Forward: tnerf_pass.h with TRAIN = true - the inference pass, bit for bit, that also saves per padded row
// (swnerf_train_rows) act [rows, SW_TN_ACT_LD] = post-ELU h0..h7 and the layer_9 hidden, and xs [rows, SW_TN_XS_LD] = the
// encodings in operand slot order (swnerf_common.h SW_TN_*).
//
// Backward (tnerf_backward_kernel): per ray
//   1. the compositing backward (render_pass.h: bwd_ray_enter / bwd_ray_load, comp_bwd_ray and, per tile, bwd_tile are shared with
//      train_kernels.hip render_pass_backward_kernel): T and w recomputed from the saved raw and depths, suffix sums of G.w in
//      double, d raw of every sample -> the wave's LDS slice;
//   2. per 32-sample tile the dX chain: d raw -> colour head (ReLU mask from raw; 3 x 64 on the VALU from bias-style tiles) -> ELU'
//      -> the folded layer_9 transposed (W9f^T, 4 x 2) + density.weight . d sigma (SEG_BIAS_SCALED) -> layers.7 .. layers.1
//      transposed (4 x 4; layer 5: its h4 columns - gamma(x), gamma(t) are data) with ELU' from the saved activations.
//      d(pre-activation) of every layer goes to grad [rows, SW_TN_ACT_LD] (the layout of act) as side stores.  (The chain of the
//      8 x 256 ReLU nets is mlp_bwd.h; this 8 x 128 ELU one shares none of it: no bit masks, activations fetched instead.)
// ELU' needs y itself (1 for y > 0, y + 1 otherwise: the rule of swnerf_elu_grad), not a bit: layer l-1's activations of the tile
// (16 KiB = 16 LDS-DMA steps) come into a slot of the wave while layer l's segment runs, ONE step every third weight step (every
// step in the 32-step W9f^T segment), each right behind that step's weight DMA (mlp_core.h SideFetch) - a burst of 16 in front of the
// segment would sit in front of its first counted waits (vmcnt retires in order).  Nothing the compiler sees is ever pending.
// Only the 64-wide hidden layer at the head of a tile has no segment in front of it: a burst of 8 and one vmcnt(0) per tile.
//
// Weight gradients: TN GEMMs of wgrad_kernels.hip over grad / act / xs (swnerf/wgrad.py, kind "tnerf"); `feature` is folded into
// layer_9, its two weight gradients come back from G = sum d pre_9 (x) h7 in swnerf_tnerf_feature_finish below.
#include "tnerf_pass.h"

// ---- forward, TRAIN ----------------------------------------------------------------------------------------------------------
extern "C" size_t swnerf_tnerf_act_floats_per_row(void) { return (size_t)SW_TN_ACT_LD; }
extern "C" size_t swnerf_tnerf_xs_floats_per_row(void) { return (size_t)SW_TN_XS_LD; }

static int sw_tnerf_train_launch(const swnerf_pass_args& a, float* act, float* xs, hipStream_t st) {
    PassDev P = pass_dev(a);
    P.w0 = a.packed;
    P.b0 = a.packed + SW_TN_W_FLOATS;
    P.nbias = SW_TN_BIAS_TILES * SW_BIAS_TILE_FLOATS;
    P.act = act; P.xs = xs;
    const dim3 grid((unsigned)((a.n_rays + 3) / 4)), block(256);
    pass_startup_args(P, grid.x, SW_TN_STEPS);
    hipLaunchKernelGGL(tnerf_render_kernel<true>, grid, block, SW_TN_LDS_FLOATS * sizeof(float), st, P);
    return sw_check(hipGetLastError(), "render_pass_train_tnerf launch");
}

extern "C" int swnerf_render_pass_train_tnerf(const swnerf_pass_args* args, float* act, float* xs, void* stream) {
    static const PassAccepts accepts = {"render_pass_train_tnerf", {0, 0, 0, SW_COLS(12)}, SWNERF_E_UNSUPP,
        "%s: T-NeRF (SWNERF_NET_TNERF) with the 12-column ray batch [o, d, near, far, t, viewdirs]", true, SW_BWD_SMAX};
    if (!args) return sw_fail(SWNERF_E_ARG, "render_pass_train_tnerf: NULL args");
    const swnerf_pass_args& a = *args;
    if (a.n_rays == 0 && a.packed) return 0;
    if (!act || !xs) return sw_fail(SWNERF_E_ARG, "render_pass_train_tnerf: NULL pointer");
    if (int rc = pass_check(accepts, a)) return rc;
    if (a.n_importance > 0)
        return sw_fail(SWNERF_E_ARG, "render_pass_train_tnerf: T-NeRF has no hierarchical resampling (run_tnerf.py forces N_importance = 0), got n_importance %d", a.n_importance);
    if (a.L_dir == 0) return sw_fail(SWNERF_E_UNSUPP, "render_pass_train_tnerf: T-NeRF needs view directions (L_dir >= 1; TNeRF.forward reads vdir)");
    if (a.dx) return sw_fail(SWNERF_E_ARG, "render_pass_train_tnerf: T-NeRF has no position_delta output");
    if (!a.raw || !(a.z_vals || a.z_out)) return sw_fail(SWNERF_E_ARG, "render_pass_train_tnerf: the backward needs raw and the depths (z_vals given or z_out)");
    if (((uintptr_t)act | (uintptr_t)xs | (uintptr_t)a.raw) % 16) return sw_fail(SWNERF_E_ARG, "render_pass_train_tnerf: act, xs and raw must be 16-byte aligned");
    return sw_tnerf_train_launch(a, act, xs, (hipStream_t)stream);
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
// One layer's saved activations of a 32-row tile, through LDS: chunk c = 4n + g (16 bytes per lane: features 32n + 8g + 4h ..+3
// of row j) is one LDS-DMA step into 1 KiB of the wave's slot; lane (j, h) reads back exactly what it fetched.
struct ActRing {
    const char* base;        // wave-uniform: the tile's first row of act
    unsigned voff, lds_addr; // (j * SW_TN_ACT_LD + 4h) * 4; LDS byte address of the slot
    const float* slot;       // the slot + lane * 4 floats
};
#define TB_ACT_SLOT_FLOATS (16 * SW_STEP_FLOATS)
__device__ __forceinline__ void act_start(ActRing& ar, const float* act_tile, float* lds_slot, int lane) {
    ar.base = reinterpret_cast<const char*>(act_tile);
    ar.voff = (unsigned)(((lane & 31) * SW_TN_ACT_LD + 4 * (lane >> 5)) * 4);
    ar.lds_addr = __builtin_amdgcn_readfirstlane((unsigned)(size_t)lds_slot);
    ar.slot = lds_slot + lane * 4;
}
// fetch the NT tiles at column `col` as ONE burst (the head of a tile, where no segment runs yet); the previous contents must have
// been read (act_take ends with lgkmcnt(0))
template <int NT>
__device__ __forceinline__ void act_fetch(const ActRing& ar, int col) {
#pragma unroll
    for (int c = 0; c < 4 * NT; ++c) ws_dma(ar.base + (col + 32 * (c >> 2) + 8 * (c & 3)) * 4, ar.voff, ar.lds_addr + c * 1024);
}
// the same fetch spread over the steps of the segment that runs meanwhile (mlp_core.h SideFetch): the 4 tiles at column `col`
__device__ __forceinline__ SideFetch act_side(const ActRing& ar, int col) { return SideFetch{ar.base + col * 4, ar.voff, ar.lds_addr}; }
// d[n][r] *= ELU'(y) from the activations fetched last; legal behind the segment that carried the fetch (its last DMA goes out
// >= SW_RING steps before the segment ends), or after ws_wait<0>()
template <int NT>
__device__ __forceinline__ void act_take_elu_grad(const ActRing& ar, f32x16 (&d)[NT]) {
#pragma unroll
    for (int c = 0; c < 4 * NT; ++c) {
        const f32x4 y = *reinterpret_cast<const f32x4*>(ar.slot + c * SW_STEP_FLOATS);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float v = d[c >> 2][4 * (c & 3) + e];
            d[c >> 2][4 * (c & 3) + e] = y[e] > 0.f ? v : v * (y[e] + 1.f);
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

#define TB_WAVE_FLOATS (SW_RING * SW_STEP_FLOATS + TB_ACT_SLOT_FLOATS + SW_BWD_COMP_FLOATS)    // weight ring | act slot | T[S], w[S], d_raw[S][4]
#define TB_LDS_FLOATS (SW_TN_BWD_BIAS_TILES * SW_BIAS_TILE_FLOATS + 4 * TB_WAVE_FLOATS)

struct TnBwdDev {
    const float* w0; const float* b0;                // backward stream; bias-style tiles: density.weight (4), color.weight (3 x 2)
    const float* act;                                // [rows, SW_TN_ACT_LD]
    const float* raw; const float* z; const float* ray_batch; const float* noise;
    int64_t n_rays; int S; int white;
    const float* g_rgb; const float* g_disp; const float* g_acc; const float* g_raw;
    float* grad; float* d_raw;                       // [rows, SW_TN_ACT_LD], [rows, 4] = d(pre-ReLU colour)(3), d sigma
};

__global__ void __launch_bounds__(256, 1) tnerf_backward_kernel(TnBwdDev P) {
    extern __shared__ __attribute__((aligned(16))) float lds_all[];
    constexpr int BIASF = SW_TN_BWD_BIAS_TILES * SW_BIAS_TILE_FLOATS;
    const int S = P.S;
    BwdRay r;
    bwd_ray_enter(r, lds_all, P.b0, BIASF);
    if (r.ray >= P.n_rays) return;                    // wave-uniform
    bwd_ray_load(r, P.ray_batch, 12, P.raw, 4, P.z, S);
    const int lane = r.lane, h = r.h;
    float* lds_ring = lds_all + BIASF + r.wv * TB_WAVE_FLOATS;
    float* lds_act = lds_ring + SW_RING * SW_STEP_FLOATS;
    WStream ws;
    ws_start(ws, P.w0, lds_all, lds_ring, lane);      // the weight ring fills while the compositing backward runs

    // ---- 1. compositing backward (render_pass.h comp_bwd_ray; no d(depth_map) and no d(weights) reach the fused step)
    float* T_ = lds_act + TB_ACT_SLOT_FLOATS;
    float* W_ = T_ + SW_BWD_SMAX;
    float* dR = W_ + SW_BWD_SMAX;
    const int64_t ray = r.ray;
    comp_bwd_ray<true>(r.raw, 4, r.zv, P.noise ? P.noise + ray * S : nullptr, S, lane, r.dnorm, P.white, P.g_rgb ? P.g_rgb + ray * 3 : nullptr,
                       P.g_disp ? P.g_disp + ray : nullptr, P.g_acc ? P.g_acc + ray : nullptr, T_, W_, dR);

    // ---- 2. the dX chain, tile by tile
    const f32x4 nomask = {0.f, 0.f, 0.f, 0.f};
#pragma nounroll
    for (int tile = 0; tile < r.ntiles; ++tile) {
        ActRing ar;                                                          // (the tile index is bwd_tile's tix, written here too: bwd_tile has to stay behind the fetch)
        act_start(ar, P.act + (r.ray * r.ntiles + tile) * 32 * SW_TN_ACT_LD, lds_act, lane);
        act_fetch<2>(ar, SW_TN_ACT_HV);                                      // the layer_9 hidden; waited for below (once per tile)
        const BwdTile t = bwd_tile(r, tile, S, dR, P.g_raw);                 // (behind the fetch: its loads wait, the DMAs do not)
        f32x4 dr = t.dr;
        {   // the colour head's ReLU (model.py:188-189): raw holds its OUTPUT, so the mask is raw > 0
            const f32x4 r4 = *reinterpret_cast<const f32x4*>(r.raw + t.sc * 4);
            dr[0] = r4[0] > 0.f ? dr[0] : 0.f; dr[1] = r4[1] > 0.f ? dr[1] : 0.f; dr[2] = r4[2] > 0.f ? dr[2] : 0.f;
        }
        if (h == 0) *reinterpret_cast<f32x4*>(P.d_raw + t.prow * 4) = dr;
        float* grad_row = P.grad + t.prow * SW_TN_ACT_LD + 4 * h;
        // d hv = color.weight^T . d pre_color: 3 weight rows as bias-style tiles behind density.weight's four (tile n of channel c: [h][r])
        f32x16 dhv[2], in[4], out[4];
        // (written out ON PURPOSE: as mlp_bwd.h wrows_valu with a tile count of 2 this kernel came out at 204 / 140 registers for 208 / 144 and 291 s_waitcnt for 290)
        const float* wt = lds_all + 4 * SW_BIAS_TILE_FLOATS + h * 16;
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 w0 = *reinterpret_cast<const f32x4*>(wt + (0 * 2 + n) * SW_BIAS_TILE_FLOATS + 4 * q);
                const f32x4 w1 = *reinterpret_cast<const f32x4*>(wt + (1 * 2 + n) * SW_BIAS_TILE_FLOATS + 4 * q);
                const f32x4 w2 = *reinterpret_cast<const f32x4*>(wt + (2 * 2 + n) * SW_BIAS_TILE_FLOATS + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) dhv[n][4 * q + e] = w0[e] * dr[0] + w1[e] * dr[1] + w2[e] * dr[2];
            }
        ws_wait<0>();            // the hidden layer's activations have landed (no segment lies between their fetch and their use: once per tile)
        act_take_elu_grad<2>(ar, dhv);                                       // d pre_9
        // d h7 = W9f^T . d pre_9 + density.weight * d sigma: `feature` folded into layer_9 (SW_TN_BWD_STEPS); h7 comes in meanwhile
        seg_mfma<4, 2, SEG_BIAS_SCALED, 2, 4>(out, dhv, ws, dr[3], SideStore{grad_row + SW_TN_ACT_HV, nullptr, nomask}, act_side(ar, 128 * 7));
#pragma nounroll
        for (int l = 7; l >= 1; --l) {
            // out = d h_l;  d pre_l = out . ELU'(h_l);  d h_{l-1} = W_l[:, -128:]^T . d pre_l
#pragma unroll
            for (int n = 0; n < 4; ++n) in[n] = out[n];
            act_take_elu_grad<4>(ar, in);
            seg_mfma<4, 4, SEG_ZERO, 4, 4>(out, in, ws, 1.f, SideStore{grad_row + 128 * l, nullptr, nomask}, act_side(ar, 128 * (l - 1)));   // ... and h_{l-1}
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) in[n] = out[n];
        act_take_elu_grad<4>(ar, in);                                        // d pre_0 (gamma(x), gamma(t) are data: no further gradient)
        tiles_store<4>(grad_row, in);
        ws_rewind(ws, P.w0, lds_all, lane);
    }
}

extern "C" int swnerf_render_pass_backward_tnerf(const float* packed_bwd, const float* act, const float* raw, const float* z_vals,
                                                 const float* ray_batch, int cols, const float* noise, int64_t n_rays, int n_samples,
                                                 int white_bkgd, const float* g_rgb, const float* g_disp, const float* g_acc,
                                                 const float* g_raw, float* grad, float* d_raw, void* stream) {
    if (n_rays == 0 && packed_bwd) return 0;
    if (int rc = pass_bwd_check("render_pass_backward_tnerf", packed_bwd && act && raw && z_vals && ray_batch && grad && d_raw, n_rays, n_samples)) return rc;
    if (cols != 12) return sw_fail(SWNERF_E_ARG, "render_pass_backward_tnerf: T-NeRF needs the 12-column ray batch [o, d, near, far, t, viewdirs], got %d", cols);
    if (((uintptr_t)act | (uintptr_t)raw | (uintptr_t)g_raw | (uintptr_t)grad | (uintptr_t)d_raw | (uintptr_t)packed_bwd) % 16)
        return sw_fail(SWNERF_E_ARG, "render_pass_backward_tnerf: packed_bwd, act, raw, g_raw, grad and d_raw must be 16-byte aligned");
    TnBwdDev P = {};
    P.w0 = packed_bwd; P.b0 = packed_bwd + SW_TN_BWD_W_FLOATS; P.act = act; P.raw = raw; P.z = z_vals; P.ray_batch = ray_batch;
    P.noise = noise; P.n_rays = n_rays; P.S = n_samples; P.white = white_bkgd;
    P.g_rgb = g_rgb; P.g_disp = g_disp; P.g_acc = g_acc; P.g_raw = g_raw; P.grad = grad; P.d_raw = d_raw;
    hipLaunchKernelGGL(tnerf_backward_kernel, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), TB_LDS_FLOATS * sizeof(float), (hipStream_t)stream, P);
    return sw_check(hipGetLastError(), "render_pass_backward_tnerf launch");
}

// ---- un-fold -----------------------------------------------------------------------------------------------------------------
// `feature` has no activation (model.py:186-187) and every kernel runs it folded into layer_9, so `feature` and d feature do not
// exist.  With G = sum_rows d pre_9 (x) h7 [64, 128] and db9 = sum_rows d pre_9 (W9f = layer_9.weight[:, :128]):
//   d layer_9.weight[:, :128] += G . Wf^T + db9 (x) bf,   d feature.weight += W9f^T . G,   d feature.bias += W9f^T . db9
// and density's gradient is row 3 of the 4-row form (a4w [4,128] = d raw^T . h7, a4b [4]).  The sibling of swnerf_feature_finish
// (wgrad_kernels.hip), whose kernel is written for the 128 x 256 view layer.
__global__ void __launch_bounds__(128) tnerf_feature_finish_kernel(const float* G, const float* db9, const float* W9, int ld9, const float* Wf,
                                                                   const float* bf, const float* a4w, const float* a4b, float* dW9, int ld_dw9,
                                                                   float* dWf, float* dbf, float* dWd, float* dbd) {
    __shared__ float sh[128];
    const int t = threadIdx.x, b = blockIdx.x;
    if (b < 64) {                                            // row u = b of d layer_9.weight[:, :128]; thread = output column o
        sh[t] = G[b * 128 + t];
        __syncthreads();
        const float* w = Wf + (size_t)t * 128;
        float acc = 0.f;
        for (int i = 0; i < 128; ++i) acc = fmaf(sh[i], w[i], acc);
        dW9[(size_t)b * ld_dw9 + t] += acc + db9[b] * bf[t];
    } else if (b < 192) {                                    // row o = b - 64 of d feature.weight; thread = column i
        const int o = b - 64;
        if (t < 64) sh[t] = W9[(size_t)t * ld9 + o];
        __syncthreads();
        float acc = 0.f;
        for (int u = 0; u < 64; ++u) acc = fmaf(sh[u], G[u * 128 + t], acc);
        dWf[(size_t)o * 128 + t] += acc;
        if (t == 0) {
            float bb = 0.f;
            for (int u = 0; u < 64; ++u) bb = fmaf(sh[u], db9[u], bb);
            dbf[o] += bb;
        }
    } else {
        dWd[t] += a4w[3 * 128 + t];
        if (t == 0) dbd[0] += a4b[3];
    }
}

extern "C" int swnerf_tnerf_feature_finish(const float* G, const float* db9, const float* W9, int ld9, const float* Wf, const float* bf,
                                           const float* a4w, const float* a4b, float* dW9, int ld_dw9, float* dWf, float* dbf,
                                           float* dW_density, float* db_density, void* stream) {
    if (!G || !db9 || !W9 || !Wf || !bf || !a4w || !a4b || !dW9 || !dWf || !dbf || !dW_density || !db_density || ld9 < 128 || ld_dw9 < 128)
        return sw_fail(SWNERF_E_ARG, "tnerf_feature_finish: NULL pointer or a leading dimension below 128");
    hipLaunchKernelGGL(tnerf_feature_finish_kernel, dim3(193), dim3(128), 0, (hipStream_t)stream, G, db9, W9, ld9, Wf, bf, a4w, a4b, dW9, ld_dw9,
                       dWf, dbf, dW_density, db_density);
    return sw_check(hipGetLastError(), "tnerf_feature_finish launch");
}
