// colour_kernels.hip - phases B and C of the deferred colour branch of the static fp32 inference pass (view_ws.h):
// the view layer and the rgb head on the rows that phase A (render_pass_kernel<false>) stashed in the workspace, packed 32 to
// a view segment across rays, then the colour sums and rgb_map per ray.  Three kernels behind phase A on its stream:
//   colour_scan_kernel   exclusive prefix of the rays' stashed-row counts, and for every segment the ray that holds its first row
//   colour_rows_kernel   persistent waves, one view segment per turn: raw colours -> c[3][S] of each row's ray
//   colour_maps_kernel   one wave per ray: the colour sums in the in-line pass's order, rgb_map
// A unit of its own: render_kernels.hip's kernel set and static instruction counts are pinned by tests/test_isa_audit.py.
#include <hip/hip_runtime.h>
#include "../../include/swnerf.h"
#include "swnerf_common.h"
#include "mlp_core.h"
#include "host_util.h"
#include "composite.h"
#include "view_ws.h"

// ---- phase A left every ray's stashed-row count in off[ray]; in place: off[r] = stashed rows of the rays below r, off[n_rays] =
// their total; segray[g] = the ray that holds row 32 g.  One workgroup: thread t takes the rays [t K, (t + 1) K) - its own
// entries of off[] alone, read before they are written - sums their counts, and the workgroup scans the 1024 sums.
__global__ void __launch_bounds__(1024) colour_scan_kernel(ViewWs vw, int64_t n_rays) {
    __shared__ int part[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t K = (n_rays + 1023) / 1024;
    const int64_t r0 = tid * K, r1 = r0 + K < n_rays ? r0 + K : n_rays;
    int* off = vw_off(vw);
    int* segray = vw_segray(vw, n_rays);
    int sum = 0;
    for (int64_t r = r0; r < r1; ++r) sum += off[r];
    int v = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(v, o, 64); if (lane >= o) v += up; }
    if (lane == 63) part[wv] = v;
    __syncthreads();
    int below = v - sum, total = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) { if (k < wv) below += part[k]; total += part[k]; }
    for (int64_t r = r0; r < r1; ++r) {
        const int cnt = off[r];
        off[r] = below;
        for (int g = (below + 31) >> 5; 32 * g < below + cnt; ++g) segray[g] = (int)r;
        below += cnt;
    }
    if (tid == 0) off[n_rays] = total;
}

struct ColourDev {
    ViewWs vw;
    const float* ray_batch; int cols; int64_t n_rays;
    const float* b0; int nbias;         // the canonical net's bias tiles
    const float* wvl;                   // the blob's views-loop stream: the 4 x 9 view layer on [gamma(d) | h7], its tail is its own head
};

// ---- one view segment per turn of a wave: segment g = stashed rows 32 g .. 32 g + 31 of the launch, in ray order.
// mlp_kernels.h views_mean with the rows read instead of computed, each with the direction of its own ray; the ring is primed
// once per wave and follows the views-loop stream round and round.  A lane past the last row computes on a copy of it and
// stores nothing.
__global__ void __launch_bounds__(256, 2) colour_rows_kernel(ColourDev P) {
    extern __shared__ __attribute__((aligned(16))) float lds_bias[];
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    bias_to_lds(lds_bias, P.b0, P.nbias);         // the only block barrier: in front of the early exit
    const int* off = vw_off(P.vw);
    const int* segray = vw_segray(P.vw, P.n_rays);
    const int total = __builtin_amdgcn_readfirstlane(off[P.n_rays]);
    const int nseg = (total + 31) >> 5, nwaves = (int)gridDim.x * 4;
    int g = (int)blockIdx.x * 4 + wv;
    if (g >= nseg) return;                        // wave-uniform
    WStream ws;
    ws_start(ws, P.wvl, lds_bias, lds_bias + P.nbias + wv * SW_RING * SW_STEP_FLOATS, lane);
    const float* rgb_tiles = ws.bias + (SW_DIR_BIAS_TILES + 64 + 8 + 1) * SW_BIAS_TILE_FLOATS;   // rgb_linear.weight as bias-style tiles
    const float* hb_rgb = rgb_tiles - SW_BIAS_TILE_FLOATS;                                      // [b_alpha, b_r, b_g, b_b]
    const int gs = vw_group_stride(P.vw);
#pragma nounroll
    for (; g < nseg; g += nwaves) {
        const int row = 32 * g + j;
        const bool valid = row < total;
        const int i = valid ? row : total - 1;
        // the row's ray: every ray holds at least its sample 0, so a segment spans at most 32 rays from the one of its first row
        const int rg = __builtin_amdgcn_readfirstlane(segray[g]);
        const int64_t rk = (int64_t)rg + j + 1;
        const int nxt = off[rk < P.n_rays ? rk : P.n_rays];
        int dr = 0;
#pragma unroll
        for (int k = 0; k < 32; ++k) dr += (__shfl(nxt, k, 32) <= i) ? 1 : 0;
        const int64_t ray = (int64_t)rg + dr;
        const int slot = i - off[ray];
        float* reg = vw_ray(P.vw, ray);
        const int s = vw_sample(P.vw, reg)[slot];
        const float* q = vw_row(P.vw, reg, slot, h);
        f32x16 in[8], demb, hv[4];
#pragma unroll
        for (int c = 0; c < 32; ++c) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(q + (size_t)c * gs);
            in[c >> 2][4 * (c & 3) + 0] = v[0]; in[c >> 2][4 * (c & 3) + 1] = v[1];
            in[c >> 2][4 * (c & 3) + 2] = v[2]; in[c >> 2][4 * (c & 3) + 3] = v[3];
        }
        const float* dp = P.ray_batch + ray * P.cols + (P.cols - 3);
        pe_dir(dp[0], dp[1], dp[2], h, demb);
        ws.bias = rgb_tiles;
        ws.base = reinterpret_cast<const char*>(P.wvl);
        canon_tail_rows(in, demb, hv, lds_bias + h * 16, ws);
        float c3[3];
        head_valu<3, 4>(hv, ws, c3);
        if (valid && h == 0) {
            float* c = vw_c(P.vw, reg);
            c[s] = c3[0] + hb_rgb[1]; c[P.vw.sp + s] = c3[1] + hb_rgb[2]; c[2 * P.vw.sp + s] = c3[2] + hb_rgb[3];
        }
    }
}

// ---- the colour sums of a ray, as the tile loop of the pass forms them in line: lane j takes sample 32 t + j, tiles ascending
// (both lane halves mirror each other), then the sum over the 32 lanes; rgb_map with the white background from the stored acc.
__global__ void __launch_bounds__(256) colour_maps_kernel(ViewWs vw, int64_t n_rays, int S, int white, float* rgb_map) {
    const int lane = threadIdx.x & 63, j = lane & 31;
    const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    float* reg = vw_ray(vw, ray);
    const float* wq = vw_w(reg);
    const float* cq = vw_c(vw, reg);
    float pr = 0.f, pg = 0.f, pb = 0.f;
    const int ntiles = (S + 31) >> 5;
#pragma nounroll
    for (int t = 0; t < ntiles; ++t) {
        const int s = t * 32 + j;
        const int sc = s < S ? s : S - 1;
        const float w = s < S ? wq[sc] : 0.f;
        const float c0 = cq[sc], c1 = cq[vw.sp + sc], c2 = cq[2 * vw.sp + sc];
        comp_accumulate_colour(w, c0, c1, c2, pr, pg, pb);
    }
    pr = wave32_sum(pr); pg = wave32_sum(pg); pb = wave32_sum(pb);
    if (lane == 0) comp_write_rgb(pr, pg, pb, reg[0], white, ray, rgb_map);
}

// behind phase A on `st`; a.rgb_map != NULL
int sw_colour_split_launch(const swnerf_pass_args& a, const ViewWs& vw, const float* b0, int nbias, const float* wvl, hipStream_t st) {
    hipLaunchKernelGGL(colour_scan_kernel, dim3(1), dim3(1024), 0, st, vw, a.n_rays);
    // persistent: at most two workgroups per CU (256 registers: while one wave of a SIMD waits for its rows the other one has
    // the matrix pipe), and no more than the launch can have segments
    const int64_t rows_max = a.n_rays * (int64_t)(vw.rows < a.n_samples ? vw.rows : a.n_samples);
    const int64_t wgs = (rows_max + 127) / 128;
    if (wgs > 0) {
        ColourDev P;
        P.vw = vw; P.ray_batch = a.ray_batch; P.cols = a.cols; P.n_rays = a.n_rays; P.b0 = b0; P.nbias = nbias; P.wvl = wvl;
        const size_t lds = ((size_t)nbias + 4 * SW_RING * SW_STEP_FLOATS) * sizeof(float);
        hipLaunchKernelGGL(colour_rows_kernel, dim3((unsigned)(wgs < 512 ? wgs : 512)), dim3(256), lds, st, P);
    }
    hipLaunchKernelGGL(colour_maps_kernel, dim3((unsigned)((a.n_rays + 3) / 4)), dim3(256), 0, st, vw, a.n_rays, a.n_samples, a.white_bkgd, a.rgb_map);
    return sw_check(hipGetLastError(), "render_pass colour launch");
}
