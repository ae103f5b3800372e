// tnerf_kernels.hip - the fused T-NeRF render pass for gfx950 (MI355X): ONE wavefront owns ONE ray.
//
// TNeRF (model.py:152-210) is 8 layers of width 128 with ELU, a skip input [gamma(x) | gamma(t)] at layer 5, a density head
// and a colour branch feature -> layer_9 (ELU) -> color (ReLU).  One net, no hierarchical resampling (run_tnerf.py:329,
// 479-481 force N_importance to 0).  Per 32-sample tile: depths -> points -> gamma(x) (VALU) -> the 8 x 128 trunk on
// v_mfma_f32_32x32x2_f32 with the activations resident in registers (mlp_core.h at NT = KT = 4) -> density and colour heads
// -> the raw2outputs wave scan (run_tnerf.py:349-393, the arithmetic of ray.py:155-198).  Per RAY, before the first tile:
// the gamma(t) columns of layers 0 and 5 and the gamma(d) columns of the folded layer_9, each with its layer's bias, into
// per-wave LDS tiles that start those layers' accumulators (swnerf_common.h SW_TN_*).
//
// TRAIN (template parameter; swnerf_render_pass_train_tnerf): the same arithmetic - outputs are bit-equal -
// that also saves, per padded row, what tnerf_train_kernels.hip's backward needs: the post-ELU activations h0..h7 and the layer_9
// hidden (act, as side stores of the segments whose B operand they are) and the encodings in operand slot order (xs: gamma(x) as a
// side store of layer 0; the ray's gamma(t) / gamma(d) tiles into every row of the ray, once per ray).
//
// The kernel template lives in tnerf_pass.h; this translation unit instantiates the inference pass (render_kernels.hip's
// swnerf_render_pass forwards kind SWNERF_NET_TNERF to sw_tnerf_render_launch after its argument checks), tnerf_train_kernels.hip
// the TRAIN one behind its own entry point swnerf_render_pass_train_tnerf (swnerf_render_pass_train refuses this kind).
#include "tnerf_pass.h"

// Called by swnerf_render_pass (render_kernels.hip) for kind SWNERF_NET_TNERF after the common checks (render_pass.h pass_check); the T-NeRF ones are here.
int sw_tnerf_render_launch(const swnerf_pass_args& a, hipStream_t st) {
    if (a.n_importance > 0)
        return sw_fail(SWNERF_E_ARG, "render_pass: T-NeRF has no hierarchical resampling (run_tnerf.py forces N_importance = 0), got n_importance %d", a.n_importance);
    if (a.cols != 12) return sw_fail(SWNERF_E_ARG, "render_pass: T-NeRF needs the 12-column ray batch [o, d, near, far, t, viewdirs], got %d", a.cols);
    if (a.L_dir == 0) return sw_fail(SWNERF_E_UNSUPP, "render_pass: T-NeRF needs view directions (L_dir >= 1; TNeRF.forward reads vdir)");
    if (a.dx) return sw_fail(SWNERF_E_ARG, "render_pass: T-NeRF has no position_delta output");
    PassDev P = pass_dev(a);
    P.w0 = a.packed;
    P.b0 = a.packed + SW_TN_W_FLOATS;
    P.nbias = SW_TN_BIAS_TILES * SW_BIAS_TILE_FLOATS;
    if (a.n_rays == 0) return 0;
    const dim3 grid((unsigned)((a.n_rays + 3) / 4)), block(256);
    pass_startup_args(P, grid.x, SW_TN_STEPS);
    hipLaunchKernelGGL(tnerf_render_kernel<false>, grid, block, SW_TN_LDS_FLOATS * sizeof(float), st, P);
    return sw_check(hipGetLastError(), "render_pass (T-NeRF) launch");
}

// ------------------------------------------------------------------------------------------
// TNeRF.forward on bare points at ONE frame time with V view directions shared by every point (the grid query of mesh
// extraction, nerf/extract_mesh.py:27-90, through t_nerf/run_tnerf.py run_network :48-87): one wave per 32 points.  The time is a
// constant of the launch, so the T0 / T5 tiles are evaluated once per wave; the trunk and the density once per point; per
// direction v the DIR tile (a shared direction is constant over the wave's 32 rows: ray_init_tile on gamma(d_v)), the folded layer_9
// (ELU) and `color` (ReLU), summed in direction order.  Direction 0 runs in stream order (its DIR segment sits between T5 and
// MAIN, layer_9 behind layer 7); every further direction leaves the stream twice (ws_restart onto DIR, then onto layer_9: two
// exposed L2 round trips per 160 MFMAs - the stream has no loop form of the colour branch).  Same LDS layout as the pass.
struct TnQueryDev {
    const float* pts; int64_t M; const float* dirs; int64_t V;
    const float* w0; const float* b0; int nbias; float ft; float* out;
};

__global__ void __launch_bounds__(256, SW_TN_WAVES_PER_SIMD) tnerf_query_kernel(TnQueryDev P) {
    extern __shared__ __attribute__((aligned(16))) float lds_all[];
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t tile = (int64_t)blockIdx.x * 4 + wv;
    float* lds_ring = lds_all + SW_TN_BIAS_TILES * SW_BIAS_TILE_FLOATS + wv * SW_TN_WAVE_FLOATS;
    float* lds_emb = lds_ring + SW_RING * SW_STEP_FLOATS;
    float* lds_t0 = lds_emb + 2 * 16 * 64;
    float* lds_t5 = lds_t0 + 4 * SW_BIAS_TILE_FLOATS;
    float* lds_vb = lds_t5 + 4 * SW_BIAS_TILE_FLOATS;
    bias_to_lds(lds_all, P.b0, P.nbias);         // the only block barrier (its own SW_TN_* LDS layout: not mlp_kernels.h row_tile)
    if (tile * 32 >= P.M) return;                // wave-uniform
    const int64_t row = tile * 32 + j;
    const bool live = row < P.M;
    const int64_t rr = live ? row : P.M - 1;

    WStream ws;
    ws_start(ws, P.w0, lds_all, lds_ring, lane);
    {
        f32x16 k;
        pe_time(P.ft, h, k);
        ray_init_tile<4>(k, lds_t0, lane, ws);     // T0: layers.0 bias + its gamma(t) columns
        ray_init_tile<4>(k, lds_t5, lane, ws);     // T5: layers.5 bias + its gamma(t) columns
        pe_dir(P.dirs[0], P.dirs[1], P.dirs[2], h, k);
        ray_init_tile<2>(k, lds_vb, lane, ws);     // DIR of direction 0: b9f + layer_9's gamma(d) columns
    }
    const float* main_b = lds_all + SW_TN_PREFIX_BIAS_TILES * SW_BIAS_TILE_FLOATS;
    const float* dir_w = P.w0 + (SW_TN_STEPS_T0 + SW_TN_STEPS_T5) * SW_STEP_FLOATS;
    const float* l9_w = P.w0 + (SW_TN_STEPS - 32) * SW_STEP_FLOATS;          // layer_9: the last 2 x 4 segment of MAIN

    f32x16 emb[2], in[4], out[4];
    pe_pos(P.pts[rr * 3], P.pts[rr * 3 + 1], P.pts[rr * 3 + 2], h, emb);
    emb_park(lds_emb, lane, emb);
    ws.bias = lds_t0 + h * 16;                   // layer 0 on [gamma(x) | gamma(t)]: the accumulators start from the T0 tile
    seg_mfma<4, 2, SEG_BIAS>(out, emb, ws);
    ws.bias = main_b + h * 16;
    elu_tiles<4>(out, in);
#pragma nounroll
    for (int l = 1; l < 8; ++l) {
        const float* keep = ws.bias;
        if (l == 5) ws.bias = lds_t5 + h * 16;
        seg_mfma<4, 4, SEG_BIAS>(out, in, ws);
        if (l == 5) {
            ws.bias = keep;
            f32x16 e2[2];
            emb_fetch(lds_emb, lane, e2);
            seg_mfma<4, 2, SEG_ACC>(out, e2, ws);
        }
        elu_tiles<4>(out, in);
    }
    float s1[1];
    head_valu<1, 4>(in, ws, s1);
    const float* hb = ws.bias;                   // [b_density, b_r, b_g, b_b]
    const float sg = s1[0] + hb[0];
    const float* color_tiles = ws.bias + SW_BIAS_TILE_FLOATS;                // color.weight as bias-style tiles: re-read on every turn
    float sr = 0.f, sgr = 0.f, sb = 0.f;
#pragma nounroll
    for (int64_t v = 0; v < P.V; ++v) {
        if (v > 0) {
            f32x16 k;
            pe_dir(P.dirs[v * 3], P.dirs[v * 3 + 1], P.dirs[v * 3 + 2], h, k);
            ws_restart(ws, dir_w);
            ws.bias = lds_all + (SW_TN_PREFIX_BIAS_TILES - 2) * SW_BIAS_TILE_FLOATS + h * 16;      // the b9f tiles
            ray_init_tile<2>(k, lds_vb, lane, ws);
            ws_restart(ws, l9_w);
        }
        f32x16 hv[2];
        float c3[3];
        ws.bias = lds_vb + h * 16;               // layer_9 with feature folded in: accumulators from the DIR tile, then W9f . h7; ELU
        seg_mfma<2, 4, SEG_BIAS>(hv, in, ws);
        elu_tiles<2>(hv, hv);
        ws.bias = color_tiles;
        head_valu<3, 2>(hv, ws, c3);
        sr += relu1(c3[0] + hb[1]); sgr += relu1(c3[1] + hb[2]); sb += relu1(c3[2] + hb[3]);
    }
    if (live && h == 0) {
        const float inv = 1.f / (float)P.V;
        f32x4 r4 = {sr * inv, sgr * inv, sb * inv, sg};
        *reinterpret_cast<f32x4*>(P.out + row * 4) = r4;
    }
}

// Called by swnerf_query_points_time (query_kernels.hip) for kind SWNERF_NET_TNERF after its argument checks.
int sw_tnerf_query_launch(const float* packed, const float* pts, int64_t M, const float* dirs, int64_t n_dirs, float ft,
                          float* out, hipStream_t st) {
    TnQueryDev P;
    P.pts = pts; P.M = M; P.dirs = dirs; P.V = n_dirs; P.ft = ft; P.out = out;
    P.w0 = packed; P.b0 = packed + SW_TN_W_FLOATS; P.nbias = SW_TN_BIAS_TILES * SW_BIAS_TILE_FLOATS;
    return sw_launch_rows(tnerf_query_kernel, P, M, SW_TN_LDS_FLOATS * sizeof(float), st, "query_points_time (T-NeRF) launch");
}
