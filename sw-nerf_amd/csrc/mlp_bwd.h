// mlp_bwd.h - what the backward kernels of train_kernels.hip share (mlp_backward_dx_kernel, deform_backward_dx_kernel,
// render_pass_backward_kernel; that unit is the only one to include it): the ReLU-mask ring, the VALU product with a few
// weight rows, and the activation-gradient chain of the 8 x 256 net (the "dX chain"), written once.  Needs mlp_core.h alone.
//
// The dX chain mirrors the forward: one wave per 32 rows, transposed weight streams, the same register-resident
// accumulator->operand hand-over.  The ReLU derivative comes from the forward's bit masks, fetched one layer ahead by LDS-DMA
// into a 1-KiB slot of the wave (nothing the compiler sees is ever pending, like the weight ring); d(pre-activation) of every
// layer goes to grad[M, SW_ACT_LD] (same column map as act) for the weight-gradient GEMMs as side stores of the segment that
// consumes it (mlp_core.h SideStore).   model.py:39-62 reversed.
#pragma once
#include "mlp_core.h"

struct MaskRing {
    const char* base;        // wave-uniform: this tile's SW_MASK_TILE_FLOATS of bit masks
    unsigned voff, lds_addr; // lane * 16; LDS byte address of the slot
    const float* slot;       // the slot + lane * 4 floats
};
__device__ __forceinline__ void mask_start(MaskRing& mr, const float* bits, int64_t tile, float* lds_slot, int lane) {
    mr.base = reinterpret_cast<const char*>(bits + tile * SW_MASK_TILE_FLOATS);
    mr.voff = (unsigned)lane * 16u;
    mr.lds_addr = __builtin_amdgcn_readfirstlane((unsigned)(size_t)lds_slot);
    mr.slot = lds_slot + lane * 4;
}
// fetch layer l's mask; the previous contents must have been read (mask_take ends with lgkmcnt(0))
__device__ __forceinline__ void mask_fetch(const MaskRing& mr, int l) { ws_dma(mr.base + l * 1024, mr.voff, mr.lds_addr); }
// the mask fetched last; legal once a counted wait behind >= SW_RING later DMAs has passed (any full segment)
__device__ __forceinline__ f32x4 mask_take(const MaskRing& mr) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(mr.slot);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    return v;
}

// out = sum_c w_c . d_c (ACC: added to out): NC weight rows of 256 riding as bias-style tiles, tile n of channel c at
// wt + (c * 8 + n) tiles, as [h][r]; wt already points at the lane half's 16 floats.  Summed left to right.
template <int NC, bool ACC = false>
__device__ __forceinline__ void wrows_valu(const float* wt, const float (&d)[NC], f32x16 (&out)[8]) {
#pragma unroll
    for (int n = 0; n < 8; ++n)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 w[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) w[c] = *reinterpret_cast<const f32x4*>(wt + (c * 8 + n) * SW_BIAS_TILE_FLOATS + 4 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float s = ACC ? out[n][4 * g + e] + w[0][e] * d[0] : w[0][e] * d[0];
#pragma unroll
                for (int c = 1; c < NC; ++c) s += w[c][e] * d[c];
                out[n][4 * g + e] = s;
            }
        }
}

// The view head of the static net, backwards: dr = d rgb(3), d sigma of this lane's row; mr holds the fetch of the views-hidden
// mask (layer 8), ws stands at the head of the backward stream.  Leaves d h7 in `out`, h7's mask fetched, d pre_hv stored.
__device__ __forceinline__ void dx_view_head(const f32x4& dr, int h, const MaskRing& mr, WStream& ws, float* grad_row, f32x16 (&out)[8]) {
    const f32x4 nomask = {0.f, 0.f, 0.f, 0.f};
    // d hv = rgb_linear.weight^T . d rgb, masked by hv > 0           (4 tiles <- 1 k-tile holding 3 channels)
    f32x16 k1[1];
#pragma unroll
    for (int r = 0; r < 16; ++r) k1[0][r] = 0.f;
    k1[0][0] = h ? 0.f : dr[0]; k1[0][1] = h ? 0.f : dr[1]; k1[0][2] = h ? 0.f : dr[2];
    f32x16 dhv[4];
    seg_mfma<4, 1, SEG_ZERO>(dhv, k1, ws);
    mask_apply<4>(mask_take(mr), dhv);
    mask_fetch(mr, 7);
    // d h7 = W_vf^T . d pre_hv + alpha_linear.weight * d sigma  (W_vf = views_linears.0.weight[:, :256] . feature_linear.weight:
    // no activation on feature_linear, so the two transposed layers are one, swnerf_common.h SW_BWD_STEPS), masked by h7 > 0 by dx_trunk
    seg_mfma<8, 4, SEG_BIAS_SCALED, 4>(out, dhv, ws, dr[3], SideStore{grad_row + SW_ACT_HV, nullptr, nomask});
}

// The trunk, backwards: on entry out = d h7 and mr holds the fetch of h7's mask; pts_linears.7 .. 1 transposed, d pre_l to
// grad_row + 256 l as side stores; on leaving in = d pre_0 (what follows it - the store, or the embedding segment - is the caller's).
// EMB: at l == 5 also the gamma(x) part of the skip input cat[gamma(x), h4], parked in lds_emb for the caller's SEG_ACC segment.
template <bool EMB>
__device__ __forceinline__ void dx_trunk(f32x16 (&in)[8], f32x16 (&out)[8], const MaskRing& mr, WStream& ws, float* grad_row, float* lds_emb, int lane) {
    const f32x4 nomask = {0.f, 0.f, 0.f, 0.f};
#pragma nounroll
    for (int l = 7; l >= 1; --l) {
        // out = d h_l;  d pre_l = out . [h_l > 0];  d h_{l-1} = W_l[:, -256:]^T . d pre_l
#pragma unroll
        for (int n = 0; n < 8; ++n) in[n] = out[n];
        mask_apply<8>(mask_take(mr), in);
        mask_fetch(mr, l - 1);
        if constexpr (EMB) {
            if (l == 5) {
                f32x16 ge[2];
                seg_mfma<2, 8, SEG_ZERO>(ge, in, ws);
                emb_park(lds_emb, lane, ge);
            }
        }
        seg_mfma<8, 8, SEG_ZERO, 8>(out, in, ws, 1.f, SideStore{grad_row + 256 * l, nullptr, nomask});
    }
#pragma unroll
    for (int n = 0; n < 8; ++n) in[n] = out[n];
    mask_apply<8>(mask_take(mr), in);                                    // d pre_0
}
