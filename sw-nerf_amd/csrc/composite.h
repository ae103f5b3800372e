// composite.h - raw2outputs (ray.py:155-198; run_tnerf.py:349-393 is the same code) and its backward: the ONE definition of the
// compositing arithmetic, called by the fused passes (render_pass.h, tnerf_kernels.hip), the standalone op (misc_kernels.hip),
// its backward (backward_kernels.hip) and the fused backward (train_kernels.hip).  A rule - NaN disparity, the 1e10 last interval,
// cumprod precision, white background - changes here and nowhere else (tests/test_host_math.py keeps the literals in this file).
// With c = sigmoid(rgb), e = exp(-relu(sigma)*dist), a = 1-e, p = 1-a+1e-10, T_i = prod_{j<i} p_j, w = a*T:
//   G_i   = dL/dw_i = g_rgb.c_i + gA + gD*z_i (+ g_w_i)
//   dL/da_i = G_i*T_i - (sum_{k>i} G_k*w_k)/p_i ,   da/dsigma = dist*e*[not sigma<=0]
//   dL/drgb_i = w_i * g_rgb * c_i*(1-c_i)
// Pointwise pieces only.  How a kernel loads raw / z / noise is its own business, and so is the cross-lane scan: the three
// forms associate differently (wave_dpp.h), so a caller names the one it uses.
#pragma once
#include "wave_dpp.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// dists (ray.py:170-173): to the next sample's depth `zn`, 1e10 behind the last sample (more = false), times |rays_d|
__device__ __forceinline__ float comp_dist(bool more, float zn, float z, float dnorm) {
    return (more ? (zn - z) : 1e10f) * dnorm;
}

// relu as ATen has it: a NaN density stays NaN (fmaxf is maxNum and would render it as empty space); every other value as fmaxf(x, 0)
__device__ __forceinline__ float comp_relu(float sg) { return (sg < 0.f) ? 0.f : sg; }

// e = exp(-relu(sigma) * dist); alpha = 1 - e (ray.py:157).  `sg` already carries the noise (added after `raw` is stored).
__device__ __forceinline__ float comp_transmit(float sg, float dist) { return expf(-comp_relu(sg) * dist); }

// a lane past the ray's last sample is dead: alpha = 0, so it leaves the product and every sum alone
__device__ __forceinline__ float comp_alpha(float sg, float dist, bool live) {
    return live ? 1.f - comp_transmit(sg, dist) : 0.f;
}

// the factor of the cumprod (ray.py:188): rounded in float like the reference's 1.-alpha+1e-10, then multiplied up in
// double like ATen's CPU cumprod
__device__ __forceinline__ double comp_survival(float alpha) { return (double)(1.f - alpha + 1e-10f); }

// ---- the exclusive cumprod of one sweep of samples: ex = product of the lanes below, total = product of the whole sweep
struct SweepProd { double ex, total; };

// __shfl_up over groups of W lanes (l = lane in its group): 32 = the mirrored halves of the fused passes, 64 = the fused backward
template <int W>
__device__ __forceinline__ SweepProd excl_cumprod_shfl(double ps, int l) {
#pragma unroll
    for (int o = 1; o < W; o <<= 1) { const double up = __shfl_up(ps, o, W); if (l >= o) ps *= up; }
    const double ex = __shfl_up(ps, 1, W);
    return {l == 0 ? 1.0 : ex, __shfl(ps, W - 1, W)};
}

// the DPP scan over the 64 lanes (wave_dpp.h: all lanes active): the standalone op and its backward
__device__ __forceinline__ SweepProd excl_cumprod_dpp64(double ps) {
    ps = wave_incl_prod_f64(ps);
    return {wave_from_below_f64(ps, 1.0), wave_last_f64(ps)};
}

// T = the transmittance in front of this sample (w = alpha * T); Tc = the wave-uniform one in front of the sweep, carried on
__device__ __forceinline__ float comp_transmittance(const SweepProd& sp, double& Tc) {
    const float T = (float)(Tc * sp.ex);                                     // exclusive cumprod (ray.py:188)
    Tc *= sp.total;
    return T;
}

__device__ __forceinline__ float comp_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// ---- forward, per ray: per-lane partial sums of the maps (ray.py:189-193); the caller reduces them over its lanes.  Inputs by
// reference: from by-value copies the compiler packs these multiplies in other pairs than it did for the written-out code.
__device__ __forceinline__ void comp_accumulate(const float& w, const float& c0, const float& c1, const float& c2, const float& z,
                                                float& pr, float& pg, float& pb, float& pd, float& pa) {
    pr += w * comp_sigmoid(c0);
    pg += w * comp_sigmoid(c1);
    pb += w * comp_sigmoid(c2);
    pd += w * z;
    pa += w;
}

// The same sums in two parts, for the pass that knows a tile's colours later than its weights (render_pass.h, the deferred colour
// branch): every sum is its own chain of additions, so the parts give the bits of the whole.
__device__ __forceinline__ void comp_accumulate_density(const float& w, const float& z, float& pd, float& pa) {
    pd += w * z;
    pa += w;
}
__device__ __forceinline__ void comp_accumulate_colour(const float& w, const float& c0, const float& c1, const float& c2,
                                                       float& pr, float& pg, float& pb) {
    pr += w * comp_sigmoid(c0);
    pg += w * comp_sigmoid(c1);
    pb += w * comp_sigmoid(c2);
}

// rgb_map of `ray` from the reduced colour sums and acc (the white background, ray.py:195-196) - on its own for the launch that forms
// the colour sums in a later kernel than the density sums (render_pass.h, the deferred colour branch)
__device__ __forceinline__ void comp_write_rgb(float pr, float pg, float pb, float pa, int white, int64_t ray, float* rgb_map) {
    const float bg = white ? (1.f - pa) : 0.f;
    rgb_map[ray * 3 + 0] = pr + bg;
    rgb_map[ray * 3 + 1] = pg + bg;
    rgb_map[ray * 3 + 2] = pb + bg;
}

// the maps of `ray` from the reduced sums; every pointer may be NULL
__device__ __forceinline__ void comp_write_maps(float pr, float pg, float pb, float pd, float pa, int white, int64_t ray,
                                                float* rgb_map, float* disp_map, float* acc_map, float* depth_map) {
    if (rgb_map) comp_write_rgb(pr, pg, pb, pa, white, ray, rgb_map);
    if (depth_map) depth_map[ray] = pd;
    if (acc_map) acc_map[ray] = pa;
    if (disp_map) {
        const float q = pd / pa;                                             // NaN when acc == 0, kept (ray.py:192)
        disp_map[ray] = 1.f / ((q != q) ? q : fmaxf(1e-10f, q));
    }
}

// ---- backward
// what reaches every sample of a ray alike: d rgb_map, A = dL/d acc, D = dL/d depth.  The caller starts A and D from d(acc_map) and
// d(depth_map), 0 where it has none; the fold adds the white background (rgb_map += 1 - acc) and disp = 1/max(1e-10, depth/acc).
// rgb: d rgb_map is given.  Without it no gradient reaches the colours, whatever they hold: a NaN colour must not enter G as 0 * NaN.
struct CompGrads { float r, g, b, A, D; bool rgb; };

__device__ __forceinline__ void comp_bwd_fold(CompGrads& g, int white, const float* g_disp, float pd, float pa) {
    if (white) g.A -= (g.r + g.g + g.b);
    if (g_disp) {
        const float q = pd / pa;                       // no gradient on the clamped / NaN branch
        if (q > 1e-10f) { const float gq = -*g_disp / (q * q); g.D += gq / pa; g.A -= gq * pd / (pa * pa); }
    }
}

// G = dL/dw of a sample with colours c = sigmoid(rgb), without a d(weights) term (the caller adds its own)
__device__ __forceinline__ float comp_bwd_G(const CompGrads& g, float c0, float c1, float c2, float z) {
    return (g.rgb ? g.r * c0 + g.g * c1 + g.b * c2 : 0.f) + g.A + g.D * z;
}

// d raw of a sample: R = sum_{k>i} G_k*w_k in double (the caller's suffix scan), T and w as the forward stored them.
// p is rebuilt as 1 - (1 - e) + 1e-10 so that it rounds like the forward's 1 - alpha + 1e-10.
__device__ __forceinline__ f32x4 comp_bwd_sample(const CompGrads& g, float G, float T, float w, double R, float sg, float dist,
                                                 float c0, float c1, float c2) {
    const float e = comp_transmit(sg, dist);
    const float p = 1.f - (1.f - e) + 1e-10f;
    const float dLda = G * T - (float)(R / (double)p);
    const float dsig = (sg <= 0.f) ? 0.f : dLda * dist * e;                  // ATen's threshold backward: a NaN sigma passes the gradient
    if (!g.rgb) return {0.f, 0.f, 0.f, dsig};
    return {w * g.r * c0 * (1.f - c0), w * g.g * c1 * (1.f - c1), w * g.b * c2 * (1.f - c2), dsig};
}
