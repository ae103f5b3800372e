// train_kernels.hip - the training path of the MLP: the forward that saves activations
// and ReLU bit masks, the kernels that run the dX chain (mlp_bwd.h) on the canonical and the deformation net, per row
// and fused with the compositing backward (its per-ray set-up: render_pass.h).  Same building blocks as the render
// kernels (mlp_core.h) but with a 16-deep weight ring: these kernels also issue stores, `vmcnt` retires in order, and
// a store's write acknowledge takes longer than 6 ring steps often enough to cost 8 % (measured: forward 7.57 ->
// 6.94 ms, dX chain 6.64 -> 6.32 ms at 786 k rows).  The render kernels keep 8: their LDS also holds 28 KB of
// resampling scratch, and depth made no difference there.
#ifndef SW_RING
#define SW_RING 16
#endif
#include "mlp_kernels.h"
#include "render_pass.h"
#include "mlp_bwd.h"

// ------------------------------------------------------------------------------------------
// Backward of the MLP w.r.t. its activations (the "dX chain"), one wave per 32 rows: the chain itself - mask ring, view
// head, trunk - is written once in mlp_bwd.h; the kernels here seed it and finish it.
struct DxDev {
    const float* w0; const float* b0;      // backward stream; its 8 "bias" tiles = alpha_linear.weight
    const float* bits; const float* d_out; // [ceil(M/32), SW_MASK_TILE_FLOATS], [M,4]
    int64_t M; float* grad;
    const float* pts; float* d_pts; int Lp; // INGRAD: the embedded positions [M,3], their gradient [M,3]
};

// INGRAD: also d gamma(x) = pts_linears.5.weight[:, :Cpos]^T . d pre_5 + pts_linears.0.weight^T . d pre_0 in the
// slots pe_pos() fills (pack_kernels.hip rowmap), then d x = J_gamma(x)^T . d gamma(x) on the VALU (embedder.py:33-42).
template <bool INGRAD>
__global__ void __launch_bounds__(256, 1) mlp_backward_dx_kernel(DxDev P) {
    extern __shared__ __attribute__((aligned(16))) float lds_bias[];
    RowTile rt;
    if (!row_tile(rt, lds_bias, P.b0, SW_BWD_BIAS_TILES * SW_BIAS_TILE_FLOATS, P.M)) return;
    const int lane = rt.lane, h = rt.h;
    const int64_t rr = rt.rr;
    const f32x4 dr = *reinterpret_cast<const f32x4*>(P.d_out + rr * 4);     // d rgb(3), d sigma
    float* grad_row = P.grad + rr * SW_ACT_LD + 4 * h;
    const f32x4 nomask = {0.f, 0.f, 0.f, 0.f};
    MaskRing mr;
    mask_start(mr, P.bits, rt.tile, rt.lds_emb + 2 * 16 * 64, lane);
    mask_fetch(mr, 8);                                                   // views hidden; older than every weight step
    WStream ws;
    ws_start(ws, P.w0, lds_bias, rt.lds_ring, lane);
    f32x16 in[8], out[8];
    dx_view_head(dr, h, mr, ws, grad_row, out);                          // d h7
    dx_trunk<INGRAD>(in, out, mr, ws, grad_row, rt.lds_emb, lane);       // d pre_7 .. d pre_1 stored, in = d pre_0
    if (!INGRAD) {
        tiles_store<8>(grad_row, in);
    } else {
        f32x16 ge[2];
        emb_fetch(rt.lds_emb, lane, ge);
        seg_mfma<2, 8, SEG_ACC, 8>(ge, in, ws, 1.f, SideStore{grad_row, nullptr, nomask});
        // slot a of lane half h holds sin (h=0) / cos (h=1) of 2^k x_c, a = 3k + c < 30; slots 30, 31 hold x itself
        // (in line here and in render_pass_backward_kernel<1> ON PURPOSE: as one __forceinline__ function this kernel came out +27 instructions / -1 s_waitcnt, the fused one +96 / +44 or, with reference results, 312 -> 316 registers)
        const float x0 = P.pts[rr * 3], x1 = P.pts[rr * 3 + 1], x2 = P.pts[rr * 3 + 2];
        float g0 = 0.f, g1 = 0.f, g2 = 0.f;
#pragma unroll
        for (int a = 0; a < 30; ++a) {
            const int k = a / 3, c = a % 3;
            const float f = (float)(1 << k);
            const float xc = (c == 0) ? x0 : ((c == 1) ? x1 : x2);
            float d = sw_sin_or_cos(xc * f, 1 - h) * f;                  // d sin = cos, d cos = -sin
            d = h ? -d : d;
            const float t = (k < P.Lp) ? ge[a >> 4][a & 15] * d : 0.f;
            if (c == 0) g0 += t; else if (c == 1) g1 += t; else g2 += t;
        }
        if (h == 0) { g0 += ge[1][14]; g1 += ge[1][15]; } else { g2 += ge[1][14]; }
        g0 += __shfl_xor(g0, 32, 64); g1 += __shfl_xor(g1, 32, 64); g2 += __shfl_xor(g2, 32, 64);
        if (rt.live && h == 0) { P.d_pts[rt.row * 3] = g0; P.d_pts[rt.row * 3 + 1] = g1; P.d_pts[rt.row * 3 + 2] = g2; }
    }
}

// ------------------------------------------------------------------------------------------
// DirectTemporalNeRF training: the deformation net alone, saving its activations (model.py:128-136).
struct DeformDev {
    const float* x; const float* t_emb; int64_t M; int C, Lp, Ct;
    const float* w0; const float* b0; int nbias;
    float* dx; float* act; float* bits;
};

__global__ void __launch_bounds__(256, 1) deform_forward_train_kernel(DeformDev P) {
    extern __shared__ __attribute__((aligned(16))) float lds_bias[];
    RowTile rt;
    if (!row_tile(rt, lds_bias, P.b0, P.nbias, P.M)) return;
    f32x16 emb[2], in[8], out[8];
    float head[3];
    gather_pos(P.x + rt.rr * P.C, rt.h, P.Lp, emb);
    const float ft = P.t_emb[rt.rr * P.Ct];                                // column 0 of gamma(t) is t
    WStream ws;
    ws_start(ws, P.w0 + SW_STEPS_DIR * SW_STEP_FLOATS, lds_bias + SW_DIR_BIAS_TILES * SW_BIAS_TILE_FLOATS, rt.lds_ring, rt.lane);   // (behind the per-ray DIR prefix)
    const TrunkSide side = {P.act + rt.rr * SW_ACT_LD + 4 * rt.h, P.bits + rt.tile * SW_MASK_TILE_FLOATS + rt.lane * 4, true, nullptr, nullptr};
    trunk_pass<true, true>(emb, rt.lds_emb, ft, true, rt.h, in, out, head, ws, side);
    if (rt.live && rt.h == 0) { P.dx[rt.row * 3] = head[0]; P.dx[rt.row * 3 + 1] = head[1]; P.dx[rt.row * 3 + 2] = head[2]; }
}

// dX chain of the deformation net: d h7 = _time_out.weight^T . d dx, then _time.7 .. _time.1 (model.py:128-136 reversed)
struct DeformBwdDev {
    const float* w0; const float* b0;      // SWNERF_BWD_DEFORM stream; its 24 "bias" tiles = _time_out.weight rows
    const float* bits; const float* d_dx;  // [ceil(M/32), SW_MASK_TILE_FLOATS], [M,3]
    int64_t M; float* grad;
};

__global__ void __launch_bounds__(256, 1) deform_backward_dx_kernel(DeformBwdDev P) {
    extern __shared__ __attribute__((aligned(16))) float lds_bias[];
    RowTile rt;
    if (!row_tile(rt, lds_bias, P.b0, SW_DBWD_BIAS_TILES * SW_BIAS_TILE_FLOATS, P.M)) return;
    const int lane = rt.lane, h = rt.h;
    const int64_t rr = rt.rr;
    const float d3[3] = {P.d_dx[rr * 3], P.d_dx[rr * 3 + 1], P.d_dx[rr * 3 + 2]};
    float* grad_row = P.grad + rr * SW_ACT_LD + 4 * h;
    MaskRing mr;
    mask_start(mr, P.bits, rt.tile, rt.lds_emb + 2 * 16 * 64, lane);
    mask_fetch(mr, 7);
    WStream ws;
    ws_start(ws, P.w0, lds_bias, rt.lds_ring, lane);
    f32x16 in[8], out[8];
    wrows_valu<3>(ws.bias, d3, out);                                     // d h7 = _time_out.weight^T . d dx
    dx_trunk<false>(in, out, mr, ws, grad_row, nullptr, lane);
    tiles_store<8>(grad_row, in);                                        // d pre_0 (x and t are data: no further gradient)
}

// ------------------------------------------------------------------------------------------
// Backward of the fused render pass (static net): ONE wavefront owns ONE ray, like the forward.
//   1. compositing backward (autograd of ray.py:155-198) from d rgb_map / d disp_map / d acc_map: forward recompute of
//      T and w from the saved raw and depths, suffix sums of G.w in double, d raw of every sample -> the wave's LDS
//      slice (and, padded to whole tiles, to HBM: the rgb_linear / alpha_linear weight-gradient GEMMs read it);
//   2. per 32-sample tile the dX chain of mlp_backward_dx_kernel, seeded from LDS: d(pre-activation) of every layer
//      -> grad[rows, SW_ACT_LD] as side stores.
// Rows are the forward's padded rows: (ray * ntiles + tile) * 32 + j; samples past S get zero gradients.
struct PassBwdDev {
    const float* w0; const float* b0;                // backward stream; bias tiles: alpha_linear.weight (8) [, _time_out.weight rows (24)]
    const float* bits;                               // [n_rays * ntiles, SW_MASK_TILE_FLOATS]
    const float* raw; const float* z; const float* ray_batch; int cols; const float* noise;
    int64_t n_rays; int S; int white;
    const float* g_rgb; const float* g_disp; const float* g_acc;
    const float* g_raw;                              // upstream gradient of the returned raw [N,S,4] (retraw) or NULL: added to d raw
    float* grad; float* d_raw;                       // [rows, SW_ACT_LD], [rows, 4]
    // D-NeRF: the deformation net's masks, the saved dx = position_delta [N,S,3], its upstream gradient (or NULL),
    // the position-encoding band count, and the outputs grad_d [rows, SW_ACT_LD], g_dx [rows, 4] (= d dx, 4th column 0)
    const float* bits_d; const float* dx; const float* g_pd; int Lp;
    float* grad_d; float* g_dx;
    // net without view directions (MODE 2): channels of output_linear (4 or 5); raw / g_raw are [N,S,out_ch], d_raw is [rows, 8]
    int out_ch;
};

// MODE: 0 static net with view directions | 1 DirectTemporalNeRF | 2 static net WITHOUT view directions (the stream is
// pts_linears.7..1 transposed; output_linear.weight rides as out_ch x 8 bias-style tiles: d h7 = sum_c w_c . d raw_c on the VALU)
template <int MODE>
__global__ void __launch_bounds__(256, 1) render_pass_backward_kernel(PassBwdDev P) {
    constexpr bool DNERF = MODE == 1, NOVIEW = MODE == 2;
    extern __shared__ __attribute__((aligned(16))) float lds_all[];
    constexpr int BIASF = (NOVIEW ? SW_NVBWD_BIAS_TILES : (DNERF ? SW_BWD_BIAS_TILES + SW_DBWD_BIAS_TILES : SW_BWD_BIAS_TILES)) * SW_BIAS_TILE_FLOATS;
    const int oc = NOVIEW ? P.out_ch : 4;
    const int S = P.S;
    BwdRay r;
    bwd_ray_enter(r, lds_all, P.b0, NOVIEW ? oc * 8 * SW_BIAS_TILE_FLOATS : BIASF);
    if (r.ray >= P.n_rays) return;
    bwd_ray_load(r, P.ray_batch, P.cols, P.raw, oc, P.z, S);
    const int lane = r.lane, h = r.h;
    const int64_t ray = r.ray;
    float* lds_ring = lds_all + BIASF + r.wv * SW_LDS_RING_FLOATS;
    float* lds_emb = lds_ring + SW_RING * SW_STEP_FLOATS;
    WStream ws;
    ws_start(ws, P.w0, lds_all, lds_ring, lane);      // the weight ring fills while the compositing backward runs

    // ---- 1. compositing backward (render_pass.h comp_bwd_ray; no d(depth_map) and no d(weights) reach the fused step)
    float* T_ = lds_all + BIASF + 4 * SW_LDS_RING_FLOATS + r.wv * SW_BWD_COMP_FLOATS;
    float* W_ = T_ + SW_BWD_SMAX;
    float* dR = W_ + SW_BWD_SMAX;
    comp_bwd_ray<!NOVIEW>(r.raw, oc, r.zv, P.noise ? P.noise + ray * S : nullptr, S, lane, r.dnorm, P.white, P.g_rgb ? P.g_rgb + ray * 3 : nullptr,
                          P.g_disp ? P.g_disp + ray : nullptr, P.g_acc ? P.g_acc + ray : nullptr, T_, W_, dR);

    // ---- 2. the dX chain(s) of mlp_bwd.h, tile by tile: mlp_backward_dx_kernel<DNERF> [+ deform_backward_dx_kernel]
    const f32x4 nomask = {0.f, 0.f, 0.f, 0.f};
#pragma nounroll
    for (int tile = 0; tile < r.ntiles; ++tile) {
        const BwdTile bt = bwd_tile(r, tile, S, dR, NOVIEW ? nullptr : P.g_raw);
        f32x4 dr = bt.dr;
        float dr5 = 0.f;                                                     // NOVIEW, out_ch 5: the fifth channel gets a gradient from g_raw alone
        if (NOVIEW && P.g_raw && bt.live) {                                  // rows of out_ch floats: no 16-byte loads
            const float* gq = P.g_raw + (ray * S + bt.sc) * oc;
            dr[0] += gq[0]; dr[1] += gq[1]; dr[2] += gq[2]; dr[3] += gq[3];
            if (oc == 5) dr5 = gq[4];
        }
        if (h == 0) {
            if (NOVIEW) {                                                    // [rows, 8]: the A operand of output_linear's weight-gradient GEMM
                const f32x4 hi4 = {dr5, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(P.d_raw + bt.prow * 8) = dr;
                *reinterpret_cast<f32x4*>(P.d_raw + bt.prow * 8 + 4) = hi4;
            } else {
                *reinterpret_cast<f32x4*>(P.d_raw + bt.prow * 4) = dr;
            }
        }
        float* grad_row = P.grad + bt.prow * SW_ACT_LD + 4 * h;
        MaskRing mr;
        mask_start(mr, P.bits, bt.tix, lds_emb + 2 * 16 * 64, lane);
        f32x16 in[8], out[8];
        if constexpr (NOVIEW) {
            mask_fetch(mr, 7);
            // d h7 = output_linear.weight^T . d raw: out_ch weight rows as bias-style tiles (tile n of channel c: [h][r])
            const float* wt = lds_all + h * 16;
            const float d4[4] = {dr[0], dr[1], dr[2], dr[3]}, d5[1] = {dr5};
            wrows_valu<4>(wt, d4, out);
            if (oc == 5) wrows_valu<1, true>(wt + 4 * 8 * SW_BIAS_TILE_FLOATS, d5, out);      // wave-uniform
            ws_wait<0>();            // h7's mask has landed (no segment lies between its fetch and its use here: once per tile, ~1 us)
        } else {
            mask_fetch(mr, 8);
            dx_view_head(dr, h, mr, ws, grad_row, out);
        }
        dx_trunk<DNERF>(in, out, mr, ws, grad_row, lds_emb, lane);           // in = d pre_0 (D-NeRF: the gamma(x+dx) part of the skip input parked)
        if (!DNERF) {
            tiles_store<8>(grad_row, in);
        } else {
            // d gamma(x+dx) -> d(x+dx) through the sin/cos Jacobian (mlp_backward_dx_kernel<true>), + the upstream gradient of
            // position_delta (the TV loss's operand, run_dnerf.py:700-716) = d dx: the seed of the deformation net's chain
            mask_start(mr, P.bits_d, bt.tix, lds_emb + 2 * 16 * 64, lane);
            mask_fetch(mr, 7);                                               // h7 of the deformation net; taken after the next segment
            f32x16 ge[2];
            emb_fetch(lds_emb, lane, ge);
            seg_mfma<2, 8, SEG_ACC, 8>(ge, in, ws, 1.f, SideStore{grad_row, nullptr, nomask});
            const float z = r.zv[bt.sc];
            const float* dxs = P.dx + (ray * S + bt.sc) * 3;
            const float x0 = r.o[0] + r.d[0] * z + dxs[0], x1 = r.o[1] + r.d[1] * z + dxs[1], x2 = r.o[2] + r.d[2] * z + dxs[2];   // x + dx, as the forward formed it
            float g0 = 0.f, g1 = 0.f, g2 = 0.f;                               // the Jacobian of mlp_backward_dx_kernel<true>, in line (see there)
#pragma unroll
            for (int a = 0; a < 30; ++a) {
                const int k = a / 3, c = a % 3;
                const float f = (float)(1 << k);
                const float xc = (c == 0) ? x0 : ((c == 1) ? x1 : x2);
                float d = sw_sin_or_cos(xc * f, 1 - h) * f;                  // d sin = cos, d cos = -sin
                d = h ? -d : d;
                const float t = (k < P.Lp) ? ge[a >> 4][a & 15] * d : 0.f;
                if (c == 0) g0 += t; else if (c == 1) g1 += t; else g2 += t;
            }
            if (h == 0) { g0 += ge[1][14]; g1 += ge[1][15]; } else { g2 += ge[1][14]; }
            g0 += __shfl_xor(g0, 32, 64); g1 += __shfl_xor(g1, 32, 64); g2 += __shfl_xor(g2, 32, 64);
            if (P.g_pd) { const float* gp = P.g_pd + (ray * S + bt.sc) * 3; g0 += gp[0]; g1 += gp[1]; g2 += gp[2]; }
            if (!bt.live) { g0 = 0.f; g1 = 0.f; g2 = 0.f; }
            if (h == 0) { f32x4 g4 = {g0, g1, g2, 0.f}; *reinterpret_cast<f32x4*>(P.g_dx + bt.prow * 4) = g4; }
            // d h7 = _time_out.weight^T . d dx  (24 bias-style tiles right behind alpha_linear's 8), then _time.7 .. _time.1
            float* gd_row = P.grad_d + bt.prow * SW_ACT_LD + 4 * h;
            const float g3[3] = {g0, g1, g2};
            wrows_valu<3>(ws.bias, g3, out);
            dx_trunk<false>(in, out, mr, ws, gd_row, nullptr, lane);
            tiles_store<8>(gd_row, in);                                      // d pre_0 of the deformation net (x, t are data)
        }
        ws_rewind(ws, P.w0, lds_all, lane);
    }
}

extern "C" size_t swnerf_packed_bwd_floats(void) { return (size_t)SW_BWD_FLOATS; }
extern "C" size_t swnerf_act_floats_per_row(void) { return (size_t)SW_ACT_LD; }
extern "C" size_t swnerf_mask_floats(int64_t M) { return M <= 0 ? 0 : (size_t)((M + 31) / 32) * SW_MASK_TILE_FLOATS; }

extern "C" int swnerf_mlp_backward_dx(const float* packed_bwd, const float* bits, const float* d_out, int64_t M,
                                      float* grad, void* stream) {
    if (M == 0 && packed_bwd) return 0;
    if (!packed_bwd || !bits || !d_out || !grad || M < 0) return sw_fail(SWNERF_E_ARG, "mlp_backward_dx: NULL pointer or negative M");
    DxDev P;
    P.w0 = packed_bwd; P.b0 = packed_bwd + SW_BWD_W_FLOATS; P.bits = bits; P.d_out = d_out; P.M = M; P.grad = grad;
    P.pts = nullptr; P.d_pts = nullptr; P.Lp = 0;
    return sw_launch_rows(mlp_backward_dx_kernel<false>, P, M, SW_LDS_FIXED_FLOATS * sizeof(float), stream, "mlp_backward_dx launch");
}

extern "C" int swnerf_mlp_backward_dx_pts(const float* packed_bwd, const float* bits, const float* d_out, const float* pts,
                                          int64_t M, int L_pos, float* grad, float* d_pts, void* stream) {
    if (M == 0 && packed_bwd) return 0;
    if (!packed_bwd || !bits || !d_out || !pts || !grad || !d_pts || M < 0)
        return sw_fail(SWNERF_E_ARG, "mlp_backward_dx_pts: NULL pointer or negative M");
    if (int rc = sw_check_bands("mlp_backward_dx_pts", 1, L_pos)) return rc;
    DxDev P;
    P.w0 = packed_bwd; P.b0 = packed_bwd + SW_BWD_IG_W_FLOATS; P.bits = bits; P.d_out = d_out; P.M = M; P.grad = grad;
    P.pts = pts; P.d_pts = d_pts; P.Lp = L_pos;
    return sw_launch_rows(mlp_backward_dx_kernel<true>, P, M, SW_LDS_FIXED_FLOATS * sizeof(float), stream, "mlp_backward_dx_pts launch");
}

extern "C" int swnerf_deform_backward_dx(const float* packed_bwd, const float* bits_d, const float* d_dx, int64_t M,
                                         float* grad_d, void* stream) {
    if (M == 0 && packed_bwd) return 0;
    if (!packed_bwd || !bits_d || !d_dx || !grad_d || M < 0) return sw_fail(SWNERF_E_ARG, "deform_backward_dx: NULL pointer or negative M");
    DeformBwdDev P;
    P.w0 = packed_bwd; P.b0 = packed_bwd + SW_DBWD_W_FLOATS; P.bits = bits_d; P.d_dx = d_dx; P.M = M; P.grad = grad_d;
    return sw_launch_rows(deform_backward_dx_kernel, P, M, SW_LDS_FIXED_FLOATS * sizeof(float), stream, "deform_backward_dx launch");
}

extern "C" int swnerf_mlp_forward_train(const float* packed, const float* x, int64_t M, int L_pos, int L_dir,
                                        float* out, float* act, float* bits, void* stream) {
    if (M == 0 && packed) return 0;
    if (!packed || !x || !out || !act || !bits || M < 0) return sw_fail(SWNERF_E_ARG, "mlp_forward_train: NULL pointer or negative M");
    if (int rc = sw_check_bands("mlp_forward_train", 2, L_pos, L_dir)) return rc;
    MlpDev P;
    P.x = x; P.M = M; P.Lp = L_pos; P.Ld = L_dir; P.Lt = 0;
    P.Cpos = 3 * (1 + 2 * L_pos); P.C = P.Cpos + 3 * (1 + 2 * L_dir);
    P.t_emb = nullptr; P.Ct = 1; P.out = out; P.dx = nullptr; P.act = act; P.bits = bits;
    int rc = stream_ptrs(SWNERF_NET_CANON, packed, 0, &P.w0, &P.b0, &P.nbias, &P.two_pass);
    if (rc) return rc;
    P.wvl = views_loop_ptr(SWNERF_NET_CANON, packed);
    return sw_launch_rows(mlp_forward_kernel<false, true>, P, M, SW_LDS_FIXED_FLOATS * sizeof(float), stream, "mlp_forward_train launch");
}

extern "C" int swnerf_deform_forward_train(const float* packed, const float* x, const float* t_emb, int64_t M,
                                           int L_pos, int L_dir, int L_time, float* dx, float* act_d, float* bits_d, void* stream) {
    if (M == 0 && packed) return 0;
    if (!packed || !x || !t_emb || !dx || !act_d || !bits_d || M < 0) return sw_fail(SWNERF_E_ARG, "deform_forward_train: NULL pointer or negative M");
    if (int rc = sw_check_bands("deform_forward_train", 3, L_pos, L_dir, L_time)) return rc;
    DeformDev P;
    P.x = x; P.t_emb = t_emb; P.M = M; P.Lp = L_pos; P.C = 3 * (1 + 2 * L_pos) + 3 * (1 + 2 * L_dir); P.Ct = 1 + 2 * L_time;
    P.dx = dx; P.act = act_d; P.bits = bits_d;
    int two = 0;
    int rc = stream_ptrs(SWNERF_NET_DNERF, packed, 1, &P.w0, &P.b0, &P.nbias, &two);
    if (rc) return rc;
    return sw_launch_rows(deform_forward_train_kernel, P, M, SW_LDS_FIXED_FLOATS * sizeof(float), stream, "deform_forward_train launch");
}

// ---- the fused training pass ("backward for the fused path") ---------------------
extern "C" int64_t swnerf_train_rows(int64_t n_rays, int n_samples) { return n_rays * (int64_t)((n_samples + 31) / 32) * 32; }
extern "C" int swnerf_xs_floats_per_row(void) { return SW_XS_LD; }

extern "C" int swnerf_render_pass_train(const swnerf_pass_args* args, float* act, float* bits, float* xs, void* stream) {
    static const PassAccepts accepts = {"render_pass_train", {SW_COLS(11) | SW_COLS(12), 0, SW_COLS(8), 0}, SWNERF_E_UNSUPP,
        "%s: the static net (SWNERF_NET_CANON, 11- or 12-column ray batch) or the one without view directions (SWNERF_NET_NOVIEW, 8 columns)", false, SW_BWD_SMAX};
    if (!args) return sw_fail(SWNERF_E_ARG, "render_pass_train: NULL args");
    const swnerf_pass_args& a = *args;
    if (a.n_rays == 0 && a.packed) return 0;
    if (!act || !bits || !xs) return sw_fail(SWNERF_E_ARG, "render_pass_train: NULL pointer");
    int rc = pass_check(accepts, a);
    if (rc) return rc;
    if (!a.raw || !(a.z_vals || a.z_out)) return sw_fail(SWNERF_E_ARG, "render_pass_train: the backward needs raw and the depths (z_vals given or z_out)");
    if (a.dx) return sw_fail(SWNERF_E_ARG, "render_pass_train: no dx output (static net)");
    const bool noview = a.kind == SWNERF_NET_NOVIEW;
    PassDev P = pass_dev(a);
    rc = noview ? stream_ptrs_noview(a.packed, a.out_ch, &P.w0, &P.b0, &P.nbias, &P.two_pass)
                : stream_ptrs(a.kind, a.packed, 0, &P.w0, &P.b0, &P.nbias, &P.two_pass);
    if (rc) return rc;
    P.act = act; P.bits = bits; P.xs = xs;
    P.dir_steps = noview ? 0 : SW_STEPS_DIR;
    size_t lds = PassLds<false, true>::FIXED * sizeof(float);
    if ((rc = pass_resampling(accepts.name, a, P, lds))) return rc;
    const dim3 grid((unsigned)((a.n_rays + 3) / 4)), block(256);
    pass_startup_args(P, grid.x, noview ? SW_NOVIEW_STEPS : SW_CANON_STEPS);
    if (noview) hipLaunchKernelGGL((render_pass_kernel<false, true, 0, false>), grid, block, lds, (hipStream_t)stream, P);
    else hipLaunchKernelGGL((render_pass_kernel<false, true>), grid, block, lds, (hipStream_t)stream, P);
    return sw_check(hipGetLastError(), "render_pass_train launch");
}

// What the three backward entry points share: the checks (render_pass.h pass_bwd_check), the PassBwdDev they start from
// (w_floats: where the bias tiles follow the stream; D-NeRF members null, out_ch 4) and the launch.
static PassBwdDev pass_bwd_dev(const float* packed_bwd, size_t w_floats, const float* bits, const float* raw, const float* z_vals,
                               const float* ray_batch, int cols, const float* noise, int64_t n_rays, int n_samples, int white_bkgd,
                               const float* g_rgb, const float* g_disp, const float* g_acc, const float* g_raw, float* grad, float* d_raw) {
    PassBwdDev P = {};
    P.w0 = packed_bwd; P.b0 = packed_bwd + w_floats; P.bits = bits; P.raw = raw; P.z = z_vals; P.ray_batch = ray_batch;
    P.cols = cols; P.noise = noise; P.n_rays = n_rays; P.S = n_samples; P.white = white_bkgd;
    P.g_rgb = g_rgb; P.g_disp = g_disp; P.g_acc = g_acc; P.g_raw = g_raw; P.grad = grad; P.d_raw = d_raw;
    P.out_ch = 4;
    return P;
}

template <int MODE>
static int pass_bwd_launch(const char* what, const PassBwdDev& P, int bias_tiles, void* stream) {
    const size_t lds = (bias_tiles * SW_BIAS_TILE_FLOATS + 4 * SW_LDS_RING_FLOATS + 4 * SW_BWD_COMP_FLOATS) * sizeof(float);
    hipLaunchKernelGGL(render_pass_backward_kernel<MODE>, dim3((unsigned)((P.n_rays + 3) / 4)), dim3(256), lds, (hipStream_t)stream, P);
    return sw_check(hipGetLastError(), what);
}

extern "C" int swnerf_render_pass_backward(const float* packed_bwd, const float* bits, const float* raw, const float* z_vals,
                                           const float* ray_batch, int cols, const float* noise, int64_t n_rays, int n_samples,
                                           int white_bkgd, const float* g_rgb, const float* g_disp, const float* g_acc,
                                           const float* g_raw, float* grad, float* d_raw, void* stream) {
    if (n_rays == 0 && packed_bwd) return 0;
    if (int rc = pass_bwd_check("render_pass_backward", packed_bwd && bits && raw && z_vals && ray_batch && grad && d_raw, n_rays, n_samples)) return rc;
    if (cols < 8) return sw_fail(SWNERF_E_ARG, "render_pass_backward: ray_batch needs >= 8 columns");
    const PassBwdDev P = pass_bwd_dev(packed_bwd, SW_BWD_W_FLOATS, bits, raw, z_vals, ray_batch, cols, noise, n_rays, n_samples, white_bkgd,
                                      g_rgb, g_disp, g_acc, g_raw, grad, d_raw);
    return pass_bwd_launch<0>("render_pass_backward launch", P, SW_BWD_BIAS_TILES, stream);
}

// ... and for the net without view directions (SWNERF_NET_NOVIEW): raw / g_raw [N,S,out_ch], d_raw [rows, 8] (columns
// >= out_ch zero: the 16-byte aligned A operand of output_linear's weight-gradient GEMM), packed_bwd = swnerf_pack_net_bwd_noview
extern "C" int swnerf_render_pass_backward_noview(const float* packed_bwd, const float* bits, const float* raw, const float* z_vals,
                                                  const float* ray_batch, int cols, const float* noise, int64_t n_rays, int n_samples,
                                                  int white_bkgd, int out_ch, const float* g_rgb, const float* g_disp, const float* g_acc,
                                                  const float* g_raw, float* grad, float* d_raw8, void* stream) {
    if (n_rays == 0 && packed_bwd) return 0;
    if (int rc = pass_bwd_check("render_pass_backward_noview", packed_bwd && bits && raw && z_vals && ray_batch && grad && d_raw8, n_rays, n_samples)) return rc;
    if (cols < 8 || out_ch < 4 || out_ch > SW_NOVIEW_MAX_OUT) return sw_fail(SWNERF_E_ARG, "render_pass_backward_noview: cols %d / out_ch %d", cols, out_ch);
    PassBwdDev P = pass_bwd_dev(packed_bwd, SW_DBWD_W_FLOATS, bits, raw, z_vals, ray_batch, cols, noise, n_rays, n_samples, white_bkgd,
                                g_rgb, g_disp, g_acc, g_raw, grad, d_raw8);
    P.out_ch = out_ch;
    return pass_bwd_launch<2>("render_pass_backward_noview launch", P, SW_NVBWD_BIAS_TILES, stream);
}

// ---- the same for DirectTemporalNeRF at t != 0 (model.py:128-151; loss of d_nerf/run_dnerf.py:690-725) ----------------
extern "C" int swnerf_render_pass_train_dnerf(const swnerf_pass_args* args, float* act, float* bits, float* xs,
                                              float* act_d, float* bits_d, float* xs_d, void* stream) {
    static const PassAccepts accepts = {"render_pass_train_dnerf", {0, SW_COLS(12), 0, 0}, SWNERF_E_UNSUPP,
        "%s: DirectTemporalNeRF with the deformation pass (t != 0) and a 12-column ray batch", true, SW_BWD_SMAX};
    if (!args) return sw_fail(SWNERF_E_ARG, "render_pass_train_dnerf: NULL args");
    const swnerf_pass_args& a = *args;
    if (a.n_rays == 0 && a.packed) return 0;
    if (!act || !bits || !xs || !act_d || !bits_d || !xs_d) return sw_fail(SWNERF_E_ARG, "render_pass_train_dnerf: NULL pointer");
    int rc = pass_check(accepts, a);
    if (rc) return rc;
    if (!a.run_deform) return sw_fail(accepts.shape_code, accepts.shape_msg, accepts.name);
    if (a.n_importance != 0) return sw_fail(SWNERF_E_UNSUPP, "render_pass_train_dnerf: no resampling in the training pass (give the depths)");
    if (!a.raw || !a.dx || !(a.z_vals || a.z_out)) return sw_fail(SWNERF_E_ARG, "render_pass_train_dnerf: the backward needs raw, dx and the depths (z_vals given or z_out)");
    PassDev P = pass_dev(a);
    if ((rc = stream_ptrs(a.kind, a.packed, 1, &P.w0, &P.b0, &P.nbias, &P.two_pass))) return rc;
    P.act = act; P.bits = bits; P.xs = xs; P.act_d = act_d; P.bits_d = bits_d; P.xs_d = xs_d;
    P.dir_steps = SW_STEPS_DIR;
    P.time_steps = SW_STEPS_TIME;
    P.tb_off = PassLds<true, true>::FIXED;       // the four waves' per-ray TIME tiles, behind everything else
    const size_t lds = (PassLds<true, true>::FIXED + 4 * SW_TB_LDS_FLOATS) * sizeof(float);
    const dim3 grid((unsigned)((a.n_rays + 3) / 4)), block(256);
    pass_startup_args(P, grid.x, SW_DEFORM_STEPS + SW_CANON_STEPS);
    hipLaunchKernelGGL((render_pass_kernel<true, true>), grid, block, lds, (hipStream_t)stream, P);
    return sw_check(hipGetLastError(), "render_pass_train_dnerf launch");
}

extern "C" int swnerf_render_pass_backward_dnerf(const float* packed_bwd_fused, const float* bits, const float* bits_d, const float* raw,
                                                 const float* z_vals, const float* ray_batch, int cols, const float* noise,
                                                 const float* dx, const float* g_position_delta, int64_t n_rays, int n_samples,
                                                 int white_bkgd, int L_pos, const float* g_rgb, const float* g_disp, const float* g_acc,
                                                 const float* g_raw, float* grad, float* grad_d, float* d_raw, float* g_dx, void* stream) {
    if (n_rays == 0 && packed_bwd_fused) return 0;
    if (int rc = pass_bwd_check("render_pass_backward_dnerf", packed_bwd_fused && bits && bits_d && raw && z_vals && ray_batch && dx && grad && grad_d && d_raw && g_dx,
                                n_rays, n_samples)) return rc;
    if (cols < 8 || L_pos < 0 || L_pos > 10) return sw_fail(SWNERF_E_ARG, "render_pass_backward_dnerf: cols %d / L_pos %d", cols, L_pos);
    PassBwdDev P = pass_bwd_dev(packed_bwd_fused, SW_BWD_DN_W_FLOATS, bits, raw, z_vals, ray_batch, cols, noise, n_rays, n_samples, white_bkgd,
                                g_rgb, g_disp, g_acc, g_raw, grad, d_raw);
    P.bits_d = bits_d; P.dx = dx; P.g_pd = g_position_delta; P.Lp = L_pos; P.grad_d = grad_d; P.g_dx = g_dx;
    return pass_bwd_launch<1>("render_pass_backward_dnerf launch", P, SW_BWD_BIAS_TILES + SW_DBWD_BIAS_TILES, stream);
}
