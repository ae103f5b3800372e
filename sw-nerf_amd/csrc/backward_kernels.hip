// backward_kernels.hip - the standalone compositing backward:
//   raw2outputs backward: d(raw) from d(rgb_map, disp_map, acc_map, depth_map, weights)   (ray.py:155-198)
// The dX chain is written once in mlp_bwd.h; the kernels that run it - per row and fused - live in train_kernels.hip next to
// the forward they mirror, the per-ray and per-tile set-up of the fused backwards in render_pass.h; the weight-gradient GEMMs and
// everything else swnerf/wgrad.py drives live in wgrad_kernels.hip.
#include <hip/hip_runtime.h>
#include "../../include/swnerf.h"
#include "swnerf_common.h"
#include "wave_dpp.h"
#include "composite.h"
#include "host_util.h"

// ---------------------------------------------------------------------------------------------
// raw2outputs backward, one wave per ray: the arithmetic and its derivation are composite.h's.  Prefix products and suffix
// sums run in double like the forward.
// Both scans run on the DPP path (wave_dpp.h; the kernel is VALU-issue bound).  The suffix sums of pass 2 become PREFIX sums
// over lanes by handing the samples of a 64-sample chunk to the lanes in REVERSE order (lane L owns sample 64 ch + 63 - L): the
// loads stay one contiguous 1 KiB / 256 B block per wave instruction.  T and w of pass 1 wait in the wave's 2 x S floats of LDS.
#define R2B_SMAX 1024
__global__ void __launch_bounds__(256) raw2outputs_bwd_kernel(const float* raw, const float* zv, const float* rd, const float* noise,
                                                              int64_t N, int S, int white, const float* g_rgb, const float* g_disp,
                                                              const float* g_acc, const float* g_depth, const float* g_w, float* d_raw, int Sp) {
    extern __shared__ __attribute__((aligned(16))) float r2b_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t ray = (int64_t)blockIdx.x * 4 + wv;
    if (ray >= N) return;
    float* T_ = r2b_lds + wv * 2 * Sp; float* W_ = T_ + Sp;
    const float dx = rd[ray * 3], dy = rd[ray * 3 + 1], dz = rd[ray * 3 + 2];
    const float dnorm = sqrtf(dx * dx + dy * dy + dz * dz);
    CompGrads g = {g_rgb ? g_rgb[ray * 3] : 0.f, g_rgb ? g_rgb[ray * 3 + 1] : 0.f, g_rgb ? g_rgb[ray * 3 + 2] : 0.f,
                   g_acc ? g_acc[ray] : 0.f, g_depth ? g_depth[ray] : 0.f, g_rgb != nullptr};
    const float* zr = zv + ray * S;
    const float4* rr = reinterpret_cast<const float4*>(raw) + ray * S;
    const float* nr = noise ? noise + ray * S : nullptr;
    // pass 1: forward recompute of T, w; accumulate acc and depth for the disparity term
    double Tc = 1.0;
    float pa = 0.f, pd = 0.f;
    for (int base = 0; base < S; base += 64) {
        const int s = base + lane;
        const bool live = s < S;
        const int sc = live ? s : S - 1;
        const float z = zr[sc];
        const float z_edge = (lane == 63 && s + 1 < S) ? zr[s + 1] : 0.f;
        const float zn = wave_from_above_f32(z, z_edge);          // a cross-lane read: never under a lane-dependent branch
        const float dist = comp_dist(s + 1 < S, zn, z, dnorm);
        float sg = rr[sc].w;
        if (nr) sg += nr[sc];
        const float alpha = comp_alpha(sg, dist, live);
        const float T = comp_transmittance(excl_cumprod_dpp64(comp_survival(alpha)), Tc);
        const float w = alpha * T;
        if (live) { T_[s] = T; W_[s] = w; }
        pa += w; pd += w * z;
    }
    pa = __shfl(wave_sum_to_last_f32(pa), 63, 64); pd = __shfl(wave_sum_to_last_f32(pd), 63, 64);
    comp_bwd_fold(g, white, g_disp ? g_disp + ray : nullptr, pd, pa);
    // pass 2: G_i, then the suffix sums of G*w from the last chunk to the first
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    double carry = 0.0;
    const int nch = (S + 63) / 64;
    for (int ch = nch - 1; ch >= 0; --ch) {
        const int s = ch * 64 + 63 - lane;               // reversed: lane 0 owns the chunk's last sample
        const bool live = s < S;
        const int sc = live ? s : S - 1;
        const float4 r4 = rr[sc];
        const float z = zr[sc];
        const float c0 = comp_sigmoid(r4.x), c1 = comp_sigmoid(r4.y), c2 = comp_sigmoid(r4.z);
        const float w = live ? W_[sc] : 0.f, T = live ? T_[sc] : 0.f;
        float G = comp_bwd_G(g, c0, c1, c2, z);
        if (g_w) G += g_w[ray * S + sc];
        // inclusive sum of G*w over the lanes <= this one = the samples >= s of the chunk, in double
        const double v = live ? (double)G * (double)w : 0.0;
        const double incl = wave_incl_sum_f64(v);
        const double R = carry + wave_from_below_f64(incl, 0.0);     // everything strictly behind sample s
        carry += wave_last_f64(incl);
        const float z_edge = (lane == 0 && s + 1 < S) ? zr[s + 1] : 0.f;      // sample s+1 sits one lane BELOW
        const float zn = dpp_f32<SW_DPP_WAVE_SHR1>(z_edge, z);    // (cross-lane: outside the lane-dependent select)
        const float dist = comp_dist(s + 1 < S, zn, z, dnorm);
        float sg = r4.w;
        if (nr) sg += nr[sc];
        const f32x4 o4 = comp_bwd_sample(g, G, T, w, R, sg, dist, c0, c1, c2);
        if (live) *reinterpret_cast<f32x4*>(d_raw + (ray * S + s) * 4) = o4;
    }
}

extern "C" int swnerf_raw2outputs_backward(const float* raw, const float* z_vals, const float* rays_d, const float* noise,
                                           int64_t N, int S, int white_bkgd, const float* g_rgb, const float* g_disp,
                                           const float* g_acc, const float* g_depth, const float* g_weights, float* d_raw,
                                           void* stream) {
    if (S < 2 || S > R2B_SMAX) return sw_fail(SWNERF_E_UNSUPP, "raw2outputs_backward: 2 <= S <= %d (got %d)", R2B_SMAX, S);
    if (N == 0) return 0;
    if (!raw || !z_vals || !rays_d || !d_raw || N < 0) return sw_fail(SWNERF_E_ARG, "raw2outputs_backward: NULL pointer / negative N");
    const int Sp = (S + 63) & ~63;
    hipLaunchKernelGGL(raw2outputs_bwd_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), (size_t)4 * 2 * Sp * sizeof(float), (hipStream_t)stream,
                       raw, z_vals, rays_d, noise, N, S, white_bkgd, g_rgb, g_disp, g_acc, g_depth, g_weights, d_raw, Sp);
    return sw_check(hipGetLastError(), "raw2outputs_backward launch");
}
