// tnerf_pass.h - the fused T-NeRF render pass (kernel template): see tnerf_kernels.hip for the plan.  Instantiated twice:
// tnerf_kernels.hip <TRAIN = false> (inference) and tnerf_train_kernels.hip <TRAIN = true> (the pass that also saves what the
// backward needs) - one definition of the arithmetic, so the two give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/swnerf.h"
#include "swnerf_common.h"
#include "host_util.h"
#include "render_pass.h"
#include "elu.h"

#define SW_TN_WAVES_PER_SIMD 2          // 4 accumulator tiles per activation: two waves per SIMD fit (DESIGN.md T-NeRF)

// LDS: the bias-style tiles | per wave: weight ring, parked gamma(x) (2 k-tiles), per-ray tiles T0 (4) T5 (4) DIR (2)
#define SW_TN_WAVE_FLOATS (SW_RING * SW_STEP_FLOATS + 2 * 16 * 64 + SW_TN_PREFIX_BIAS_TILES * SW_BIAS_TILE_FLOATS)
#define SW_TN_LDS_FLOATS (SW_TN_BIAS_TILES * SW_BIAS_TILE_FLOATS + 4 * SW_TN_WAVE_FLOATS)

template <int NT>
__device__ __forceinline__ void elu_tiles(const f32x16 (&x)[NT], f32x16 (&y)[NT]) {
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) y[n][r] = sw_elu(x[n][r]);
}

// a ray-constant encoding tile (gamma(t) or gamma(d)) into xs columns col0.. of every padded row of the ray (TRAIN)
__device__ __forceinline__ void tn_xs_ray_tile(const f32x16& k, float* xs_ray, int ntiles, int col0, int j, int h) {
#pragma nounroll
    for (int tile = 0; tile < ntiles; ++tile)
        xs_store_tile(xs_ray + ((int64_t)tile * 32 + j) * SW_TN_XS_LD + col0 + 4 * h, k);
}

template <bool TRAIN>
__global__ void __launch_bounds__(256, SW_TN_WAVES_PER_SIMD) tnerf_render_kernel(PassDev P) {
    extern __shared__ __attribute__((aligned(16))) float lds_all[];
    const swnerf_pass_args& a = P.a;
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t ray = (int64_t)blockIdx.x * 4 + wv;
    float* lds_ring = lds_all + SW_TN_BIAS_TILES * SW_BIAS_TILE_FLOATS + wv * SW_TN_WAVE_FLOATS;
    float* lds_emb = lds_ring + SW_RING * SW_STEP_FLOATS;
    float* lds_t0 = lds_emb + 2 * 16 * 64;
    float* lds_t5 = lds_t0 + 4 * SW_BIAS_TILE_FLOATS;
    float* lds_vb = lds_t5 + 4 * SW_BIAS_TILE_FLOATS;
    pass_startup(P, P.w0, lds_emb, lane, wv);    // junk slot = the parked-encoding region: nothing is parked before ws_start's wait
    bias_to_lds(lds_all, P.b0, P.nbias);         // the only block barrier
    if (ray >= a.n_rays) return;                 // wave-uniform

    const int S = a.n_samples;
    const float* rb = a.ray_batch + ray * 12;    // [o, d, near, far, t, viewdirs] (run_tnerf.py:156-164)
    // (the directions are read where pe_dir needs them, behind T0 / T5: loaded here with the row they merge into one wider load - 228 -> 227 global_*)
    const RayRow r = ray_row_load<false>(rb, 12);

    const int ntiles = (S + 31) >> 5;
    WStream ws;
    ws_start(ws, P.w0, lds_all, lds_ring, lane);
    {
        f32x16 k;
        pe_time(r.ft, h, k);
        if constexpr (TRAIN) tn_xs_ray_tile(k, P.xs + ray * ntiles * 32 * SW_TN_XS_LD, ntiles, 64, j, h);
        ray_init_tile<4>(k, lds_t0, lane, ws);     // T0: layers.0 bias + its gamma(t) columns
        ray_init_tile<4>(k, lds_t5, lane, ws);     // T5: layers.5 bias + its gamma(t) columns
        pe_dir(rb[9], rb[10], rb[11], h, k);
        if constexpr (TRAIN) tn_xs_ray_tile(k, P.xs + ray * ntiles * 32 * SW_TN_XS_LD, ntiles, 96, j, h);
        ray_init_tile<2>(k, lds_vb, lane, ws);     // DIR: b9f + layer_9's gamma(d) columns
    }
    const float* main_w = P.w0 + SW_TN_PREFIX_STEPS * SW_STEP_FLOATS;
    const float* main_b = lds_all + SW_TN_PREFIX_BIAS_TILES * SW_BIAS_TILE_FLOATS;
    ws.bias = main_b + h * 16;

    const float* zrow = a.z_vals ? a.z_vals + ray * S : nullptr;
    float pr = 0.f, pg = 0.f, pb = 0.f, pd = 0.f, pa = 0.f;
    double Tc = 1.0;                              // transmittance carried across tiles
#pragma nounroll
    for (int tile = 0; tile < ntiles; ++tile) {
        const int s = tile * 32 + j;
        const bool live = s < S;
        const int sc = live ? s : S - 1;
        float z, zn;
        if (zrow) {
            z = zrow[sc];
            zn = (s + 1 < S) ? zrow[s + 1] : z;
        } else {
            z = z_sample(a, ray, r.near, r.far, sc);
            zn = (s + 1 < S) ? z_sample(a, ray, r.near, r.far, s + 1) : z;
        }
        // pts = rays_o + rays_d * z  (two roundings, run_tnerf.py:477)
        const float px = r.o[0] + r.d[0] * z, py = r.o[1] + r.d[1] * z, pz = r.o[2] + r.d[2] * z;

        f32x16 emb[2], in[4], out[4], hv[2];
        pe_pos(px, py, pz, h, emb);
        emb_park(lds_emb, lane, emb);
        // TRAIN: this lane's padded row of act / xs (+ 4h: the 16-byte chunk map of mlp_core.h tiles_store)
        const int64_t prow = (ray * ntiles + tile) * 32 + j;
        float* act_row = TRAIN ? P.act + prow * SW_TN_ACT_LD + 4 * h : nullptr;
        const f32x4 nomask = {0.f, 0.f, 0.f, 0.f};
        // layer 0 on [gamma(x) | gamma(t)]: the accumulators start from the per-ray T0 tile
        ws.bias = lds_t0 + h * 16;
        if constexpr (TRAIN) seg_mfma<4, 2, SEG_BIAS, 2>(out, emb, ws, 1.f, SideStore{P.xs + prow * SW_TN_XS_LD + 4 * h, nullptr, nomask});
        else seg_mfma<4, 2, SEG_BIAS>(out, emb, ws);
        ws.bias = main_b + h * 16;
        elu_tiles<4>(out, in);
#pragma nounroll
        for (int l = 1; l < 8; ++l) {
            // layer 5 on cat([gamma(x), gamma(t)], h4) (model.py:200-201): h4 from the per-ray T5 tile, then the gamma(x) columns
            const float* keep = ws.bias;
            if (l == 5) ws.bias = lds_t5 + h * 16;
            if constexpr (TRAIN) seg_mfma<4, 4, SEG_BIAS, 4>(out, in, ws, 1.f, SideStore{act_row + 128 * (l - 1), nullptr, nomask});   // h_{l-1}
            else seg_mfma<4, 4, SEG_BIAS>(out, in, ws);
            if (l == 5) {
                ws.bias = keep;
                f32x16 e2[2];
                emb_fetch(lds_emb, lane, e2);
                seg_mfma<4, 2, SEG_ACC>(out, e2, ws);
            }
            elu_tiles<4>(out, in);
        }
        // density (no activation): a VALU head; then the head-bias tile [b_density, b_r, b_g, b_b]
        float s1[1], c3[3];
        head_valu<1, 4>(in, ws, s1);
        const float* hb = ws.bias;
        float sg = s1[0] + hb[0];
        ws.bias += SW_BIAS_TILE_FLOATS;
        // layer_9 on [feature | gamma(d)] with feature folded in: accumulators from the per-ray DIR tile, then W9f . h7; ELU
        {
            const float* keep = ws.bias;
            ws.bias = lds_vb + h * 16;
            if constexpr (TRAIN) seg_mfma<2, 4, SEG_BIAS, 4>(hv, in, ws, 1.f, SideStore{act_row + 128 * 7, nullptr, nomask});          // h7
            else seg_mfma<2, 4, SEG_BIAS>(hv, in, ws);
            ws.bias = keep;
        }
        elu_tiles<2>(hv, hv);
        if constexpr (TRAIN) tiles_store<2>(act_row + SW_TN_ACT_HV, hv);
        head_valu<3, 2>(hv, ws, c3);
        const float c0 = relu1(c3[0] + hb[1]), c1 = relu1(c3[1] + hb[2]), c2 = relu1(c3[2] + hb[3]);
        ws_rewind(ws, main_w, main_b, lane);     // the ring already holds MAIN's head (the blob's tail copy)

        // ---- raw2outputs on this tile (composite.h; run_tnerf.py:349-393); both lane halves mirror each other
        if (a.raw && live && h == 0) {
            f32x4 r4 = {c0, c1, c2, sg};
            *reinterpret_cast<f32x4*>(a.raw + (ray * S + s) * 4) = r4;
        }
        float alpha;
        const float w = pass_weight(a, ray, s, sc, live, j, sg, z, zn, r.dnorm, Tc, alpha);
        if (live) pass_store_wz(a, ray, s, h, w, z);
        comp_accumulate(w, c0, c1, c2, z, pr, pg, pb, pd, pa);
    }

    pass_write_maps(pr, pg, pb, pd, pa, lane, false, a, ray, a.rgb_map);
}
