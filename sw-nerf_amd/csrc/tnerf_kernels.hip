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
