// render_pass.h - the fused NeRF render pass for gfx950 (MI355X): ONE wavefront owns ONE ray.
//
// For each 32-sample tile of its ray the wave computes depths -> points -> positional encoding (VALU) ->
// [deformation MLP ->] canonical MLP (MFMA, registers: mlp_core.h) -> alpha compositing (wave scan), and after the
// last tile optionally the hierarchical resampling (inverse-CDF + rank merge in the wave's LDS slice).  Nothing
// per-sample touches HBM unless the caller asks for it (raw / weights / dx / z_out).
// Shared by the inference translation unit (render_kernels.hip, ring depth 8) and the training one
// (train_kernels.hip, ring depth 16, TRAIN = true: the same pass that also saves what the backward needs).
//
// Reference: render_rays nerf/run.py:316-422, d_nerf/run_dnerf.py:354-480; raw2outputs ray.py:155-198;
// sample_pdf ray.py:96-153; run_network nerf/run.py:73-87.
#pragma once
#include <cstdlib>
#include "mlp_kernels.h"
#include "mlp_core_x3.h"
#include "resample.h"
#include "composite.h"
#include "ray_rows.h"
#include "view_ws.h"

#define SW_LDS_SC 256                    // max coarse samples when resampling
#define SW_LDS_SORT 1024                 // max S + n_importance (padded to a power of two)
#define SW_LDS_WAVE_FLOATS (3 * SW_LDS_SC + SW_LDS_SORT)

struct PassDev {
    swnerf_pass_args a;
    const float* w0;        // weight stream this pass runs per tile
    const float* b0;        // its bias stream
    int nbias;              // floats in the bias stream (multiple of 32)
    int two_pass;           // 1: deformation net then canonical net
    int sort_n, sort_s;     // powers of two >= n_importance / >= n_samples (fallback sort of an unsorted list)
    // TRAIN only (swnerf_render_pass_train): what the backward needs.  Rows are PADDED to whole 32-sample tiles per ray:
    // row = (ray * ceil(S/32) + tile) * 32 + j; rows past S carry copies of the last sample and get zero gradients.
    float* act;             // [rows, SW_ACT_LD]   post-ReLU activations (column map: swnerf_common.h)
    float* bits;            // [rows/32, SW_MASK_TILE_FLOATS]   ReLU bit masks
    float* xs;              // [rows, SW_XS_LD]    the encodings gamma(x), gamma(d) in B-operand SLOT order (sw_xs_col)
    // TRAIN + DNERF: the same three for the deformation net (act_d uses the first 2048 columns; xs_d = gamma(x), gamma(t))
    float* act_d; float* bits_d; float* xs_d;
    // start-up shaping of a launch (fp32 inference pass; pass_startup() below): L2 warm-up of the weight stream and a skew
    // of the waves' start.  warm_steps = 0 / skew_mode = 0 switch them off.
    int dir_steps;          // SW_STEPS_DIR when the stream starts with the per-ray DIR prefix (nets with view directions, fp32), else 0
    int time_steps;         // SW_STEPS_TIME when the deformation net's TIME segment follows it (D-NeRF with the deformation pass), else 0
    int tb_off;             // floats: where the four waves' per-ray TIME tiles sit in the dynamic LDS (behind everything else)
    int warm_steps;         // 1-KiB steps of the weight stream to pull into the XCD's L2 at kernel start
    int warm_blocks;        // workgroups per XCD that share the warm-up (blocks b with b < 8 * warm_blocks take part)
    int skew_mode;          // 0 none | 1 per workgroup | 2 per wave
    ViewWs vw;              // swnerf_render_pass_ws: the deferred colour branch's workspace (vw.base NULL = in line)
};

__device__ __forceinline__ float z_linear(const swnerf_pass_args& a, float near, float far, int s) {
    const float t = sw_linspace(0.f, 1.f, a.n_samples, s);
    if (!a.lindisp) return near * (1.f - t) + far * t;                       // nerf/run.py:363
    return 1.f / (1.f / near * (1.f - t) + 1.f / far * t);                   // nerf/run.py:365
}

// depth of sample s (0 <= s < S) of this ray
__device__ __forceinline__ float z_sample(const swnerf_pass_args& a, int64_t ray, float near, float far, int s) {
    const int S = a.n_samples;
    if (a.z_vals) return a.z_vals[ray * S + s];
    const float zs = z_linear(a, near, far, s);
    if (!a.t_rand) return zs;
    // stratified jitter, nerf/run.py:369-383
    const float upper = (s < S - 1) ? .5f * (z_linear(a, near, far, s + 1) + zs) : zs;
    const float lower = (s > 0) ? .5f * (zs + z_linear(a, near, far, s - 1)) : zs;
    return lower + (upper - lower) * a.t_rand[ray * S + s];
}

// ---- start-up shaping ----------------------------------------------------------------------------------------
// Every launch starts with the weight stream cold in the 8 XCD L2s (they are written back / invalidated at kernel
// boundaries) and with all resident waves at stream position 0.  The wave that leads takes every L2 miss, the others
// catch up behind it, and from then on all 128 waves of an XCD ask for the SAME 1-KiB step at the same moment: half of
// the L2 channels serve all of them while the other half idle.  A launch of many rounds pays that once (about 24 us at
// 4096 rays), a single-round launch (1024 rays = one wave per SIMD) for its whole duration.  So, before anything else:
//   warm-up: the first-round waves of an XCD split the stream between them and pull it into L2 with LDS-DMA into a junk
//            slot (no registers, nothing to wait for except the in-order vmcnt of the ring prime that follows);
//   skew:    waves (or workgroups) start 0..15 ring steps apart, so that concurrent requests spread over the channels.
#define SW_WARM_MAX_PER_WAVE 48
__device__ __forceinline__ void pass_startup(const PassDev& P, const float* w0, float* junk, int lane, int wv) {
    const unsigned b = blockIdx.x;
    if (P.warm_steps > 0 && (int)(b >> 3) < P.warm_blocks) {
        const unsigned junk_addr = __builtin_amdgcn_readfirstlane((unsigned)(size_t)junk);
        const int stride = P.warm_blocks * 4;
        int s = (int)(b >> 3) * 4 + wv;
#pragma nounroll
        for (int i = 0; i < SW_WARM_MAX_PER_WAVE && s < P.warm_steps; ++i, s += stride)
            ws_dma(reinterpret_cast<const char*>(w0) + (size_t)s * 1024, (unsigned)lane * 16u, junk_addr);
    }
    if (P.skew_mode) {
        const int k = (P.skew_mode == 1 ? (int)(b >> 3) : (int)(b >> 3) * 4 + wv) & 15;
#pragma nounroll
        for (int i = 0; i < k; ++i) __builtin_amdgcn_s_sleep(4);
    }
}

// host side: fill the start-up fields for a launch of `grid_x` workgroups whose pass streams `steps` weight steps per tile.
// SWNERF_WARM / SWNERF_SKEW (experiments: tools/probe_small_batch.py) override the defaults.
static inline void pass_startup_args(PassDev& P, unsigned grid_x, int steps) {
    // read per launch (two getenv calls, ~100 ns): tests flip them between launches to show that the shaping changes no bit
    const char* ew = getenv("SWNERF_WARM");
    const char* es = getenv("SWNERF_SKEW");
    const int env_warm = ew ? atoi(ew) : 1, env_skew = es ? atoi(es) : 2;
    const unsigned first_round = grid_x < 256u ? grid_x : 256u;      // one workgroup per CU is resident
    P.warm_blocks = (int)(first_round / 8u);
    P.warm_steps = (env_warm && P.warm_blocks > 0) ? steps + SW_TAIL : 0;
    P.skew_mode = env_skew;
}

// ---- host side: what every entry point of the pass checks and sets up (the per-variant checks stay with the entry point) ----
// What one entry point accepts.
struct PassAccepts {
    const char* name;           // prefix of every message
    unsigned cols[4];           // per net kind (SWNERF_NET_*): bit c set = a ray batch of c columns is accepted; 0 = kind refused
    int shape_code;             // a kind / column count outside `cols` is refused with this code ...
    const char* shape_msg;      // ... and this message (printf arguments: name, cols, kind)
    bool time_band;             // L_time is checked (and named) with L_pos / L_dir
    int smax;                   // training passes: n_samples <= smax; 0 = inference, no cap
};
#define SW_COLS(c) (1u << (c))

static inline int pass_check(const PassAccepts& e, const swnerf_pass_args& a) {
    if (!a.packed || (!a.ray_batch && a.n_rays != 0)) return sw_fail(SWNERF_E_ARG, e.smax ? "%s: NULL pointer" : "%s: NULL ray_batch/packed", e.name);
    if (a.kind < 0 || a.kind > 3 || a.cols < 0 || a.cols > 31 || !(e.cols[a.kind] >> a.cols & 1u)) return sw_fail(e.shape_code, e.shape_msg, e.name, a.cols, a.kind);
    if (e.smax && (a.n_rays < 0 || a.n_samples < 2 || a.n_samples > e.smax))
        return sw_fail(SWNERF_E_UNSUPP, "%s: 2 <= n_samples <= %d (got %d)", e.name, e.smax, a.n_samples);
    if (a.n_rays < 0 || a.n_samples < 2) return sw_fail(SWNERF_E_ARG, "%s: n_rays %lld, n_samples %d", e.name, (long long)a.n_rays, a.n_samples);
    if (a.L_pos < 0 || a.L_pos > 10 || a.L_dir < 0 || a.L_dir > 4 || (e.time_band && (a.L_time < 0 || a.L_time > 10)))
        return e.time_band ? sw_fail(SWNERF_E_UNSUPP, "%s: embedder bands (%d,%d,%d) exceed (10,4,10)", e.name, a.L_pos, a.L_dir, a.L_time)
                           : sw_fail(SWNERF_E_UNSUPP, "%s: embedder bands (%d,%d) exceed (10,4)", e.name, a.L_pos, a.L_dir);
    if (a.z_vals && a.t_rand) return sw_fail(SWNERF_E_ARG, "%s: t_rand only applies to coarse sampling", e.name);
    return 0;
}

// every launch starts from this: no member is left indeterminate
static inline PassDev pass_dev(const swnerf_pass_args& a) {
    PassDev P = {};
    P.a = a;
    return P;
}

// n_importance > 0: the limits of the in-LDS resampling, the two sort sizes, and its scratch behind the `lds` bytes so far
static inline int pass_resampling(const char* name, const swnerf_pass_args& a, PassDev& P, size_t& lds) {
    if (a.n_importance <= 0) return 0;
    if (!a.z_fine && a.n_rays != 0) return sw_fail(SWNERF_E_ARG, "%s: n_importance>0 needs z_fine", name);
    if (a.n_samples < 3 || a.n_samples > SW_LDS_SC || a.n_samples + a.n_importance > SW_LDS_SORT)
        return sw_fail(SWNERF_E_UNSUPP, "%s: resampling supports 3<=N_samples<=%d and N_samples+N_importance<=%d", name, SW_LDS_SC, SW_LDS_SORT);
    P.sort_n = P.sort_s = 2;                     // fallback sort of an unsorted sample list: powers of two >= n_importance / n_samples
    while (P.sort_n < a.n_importance) P.sort_n <<= 1;
    while (P.sort_s < a.n_samples) P.sort_s <<= 1;
    lds += 4 * SW_LDS_WAVE_FLOATS * sizeof(float);
    return 0;
}

// ---- what the fused backward kernels share (train_kernels.hip render_pass_backward_kernel, tnerf_train_kernels.hip
// tnerf_backward_kernel): ONE wavefront owns ONE ray, like the forward; rows are the forward's padded rows (TrainRows).
#define SW_BWD_SMAX 256                          // samples per ray: each wave keeps T[S], w[S], d_raw[S][4] in LDS
#define SW_BWD_COMP_FLOATS (6 * SW_BWD_SMAX)

// host side: what every entry point of a fused backward checks first (`ptrs`: every pointer this variant requires is there)
static inline int pass_bwd_check(const char* name, bool ptrs, int64_t n_rays, int n_samples) {
    if (!ptrs || n_rays < 0) return sw_fail(SWNERF_E_ARG, "%s: NULL pointer or negative n_rays", name);
    if (n_samples < 2 || n_samples > SW_BWD_SMAX) return sw_fail(SWNERF_E_UNSUPP, "%s: 2 <= n_samples <= %d (got %d)", name, SW_BWD_SMAX, n_samples);
    return 0;
}

// A wave's ray as the backward reads it (the forward's RayRow is the model): indices, this ray's saved raw [S, oc] and depths
// [S], origin and direction.  dnorm is sqrtf(d.d) WITHOUT row_dnorm's finiteness test: the backward never had it.
struct BwdRay {
    int lane, j, h, wv;                 // lane of the wave, its row of a tile, its lane half; wave of the workgroup (scalar)
    int64_t ray; int ntiles;
    const float* raw; const float* zv;
    float o[3], d[3], dnorm;
};
// The indices, and the bias tiles to LDS: bias_to_lds() holds the workgroup's only barrier, so it stands in front of the early
// exit of a wave without a ray (r.ray >= n_rays, wave-uniform), which the kernel takes right behind this ...
__device__ __forceinline__ void bwd_ray_enter(BwdRay& r, float* lds, const float* b0, int nbias) {
    r.lane = threadIdx.x & 63; r.j = r.lane & 31; r.h = r.lane >> 5;
    r.wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    r.ray = (int64_t)blockIdx.x * 4 + r.wv;
    bias_to_lds(lds, b0, nbias);
}
// ... and the row of a ray that exists
__device__ __forceinline__ void bwd_ray_load(BwdRay& r, const float* ray_batch, int cols, const float* raw, int oc, const float* z, int S) {
    r.ntiles = (S + 31) >> 5;
    const float* rb = ray_batch + r.ray * cols;
    r.o[0] = rb[0]; r.o[1] = rb[1]; r.o[2] = rb[2]; r.d[0] = rb[3]; r.d[1] = rb[4]; r.d[2] = rb[5];
    r.dnorm = sqrtf(r.d[0] * r.d[0] + r.d[1] * r.d[1] + r.d[2] * r.d[2]);
    r.zv = z + r.ray * S;
    r.raw = raw + r.ray * S * oc;
}

// The head of a tile: this lane's sample (sc: the last one for lanes past S), its tile and padded row, and d raw of the sample
// = what comp_bwd_ray left in LDS + the upstream gradient of the returned raw (g_raw4 [N,S,4] or NULL), zero past S.
struct BwdTile { int s, sc; bool live; int64_t tix, prow; f32x4 dr; };
__device__ __forceinline__ BwdTile bwd_tile(const BwdRay& r, int tile, int S, const float* dR, const float* g_raw4) {
    BwdTile t;
    t.s = tile * 32 + r.j;
    t.live = t.s < S;
    t.sc = t.live ? t.s : S - 1;
    t.tix = r.ray * r.ntiles + tile;
    t.prow = t.tix * 32 + r.j;
    t.dr = *reinterpret_cast<const f32x4*>(dR + 4 * t.sc);
    if (g_raw4) t.dr += *reinterpret_cast<const f32x4*>(g_raw4 + (r.ray * S + t.sc) * 4);
    if (!t.live) t.dr = f32x4{0.f, 0.f, 0.f, 0.f};
    return t;
}

// ---- the compositing backward of ONE ray by its wave (autograd of ray.py:155-198; composite.h): forward recompute of T and
// w from the saved raw [S, oc] and depths zv [S] (-> T_[S], W_[S] in the wave's LDS slice), suffix sums of G.w in double, d raw of
// every sample -> dR[S][4] in LDS.  noise: this ray's [S] or NULL; g_rgb [3] / g_disp [1] / g_acc [1]: this ray's upstream
// gradients, each may be NULL.  VEC4: raw rows are 16-byte aligned (oc == 4).  Ends with the LDS visible to the whole wave.
template <bool VEC4>
__device__ __forceinline__ void comp_bwd_ray(const float* raw, int oc, const float* zv, const float* noise, int S, int lane, float dnorm,
                                             int white, const float* g_rgb, const float* g_disp, const float* g_acc,
                                             float* T_, float* W_, float* dR) {
    CompGrads g = {g_rgb ? g_rgb[0] : 0.f, g_rgb ? g_rgb[1] : 0.f, g_rgb ? g_rgb[2] : 0.f, g_acc ? g_acc[0] : 0.f, 0.f, g_rgb != nullptr};
    double Tc = 1.0;
    float pa = 0.f, pd = 0.f;
    for (int base = 0; base < S; base += 64) {
        const int s = base + lane;
        const bool live = s < S;
        const int sc = live ? s : S - 1;
        const float z = zv[sc];
        const float zn = (s + 1 < S) ? zv[s + 1] : z;
        const float dist = comp_dist(s + 1 < S, zn, z, dnorm);
        float sg = raw[sc * oc + 3];
        if (noise) sg += noise[sc];
        const float alpha = comp_alpha(sg, dist, live);
        const float T = comp_transmittance(excl_cumprod_shfl<64>(comp_survival(alpha), lane), Tc);
        const float w = alpha * T;
        if (live) { T_[s] = T; W_[s] = w; }
        pa += w; pd += w * z;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { pa += __shfl_xor(pa, o, 64); pd += __shfl_xor(pd, o, 64); }
    comp_bwd_fold(g, white, g_disp, pd, pa);
    wave_lds_sync();
    double carry = 0.0;
    const int nch = (S + 63) / 64;
    for (int ch = nch - 1; ch >= 0; --ch) {
        const int s = ch * 64 + lane;
        const bool live = s < S;
        const int sc = live ? s : S - 1;
        f32x4 r4;
        if (!VEC4) { r4[0] = raw[sc * oc]; r4[1] = raw[sc * oc + 1]; r4[2] = raw[sc * oc + 2]; r4[3] = raw[sc * oc + 3]; }   // rows of 5 floats are not 16-byte aligned
        else r4 = *reinterpret_cast<const f32x4*>(raw + sc * 4);
        const float z = zv[sc];
        const float c0 = comp_sigmoid(r4[0]), c1 = comp_sigmoid(r4[1]), c2 = comp_sigmoid(r4[2]);
        const float w = live ? W_[sc] : 0.f, T = live ? T_[sc] : 0.f;
        const float G = comp_bwd_G(g, c0, c1, c2, z);
        double v = live ? (double)G * (double)w : 0.0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const double dn = __shfl_down(v, o, 64); if (lane + o < 64) v += dn; }
        double after = __shfl_down(v, 1, 64);
        if (lane == 63) after = 0.0;
        const double R = carry + after;
        carry += __shfl(v, 0, 64);
        const float zn = (s + 1 < S) ? zv[s + 1] : z;
        const float dist = comp_dist(s + 1 < S, zn, z, dnorm);
        float sg = r4[3];
        if (noise) sg += noise[sc];
        const f32x4 o4 = comp_bwd_sample(g, G, T, w, R, sg, dist, c0, c1, c2);
        if (live) *reinterpret_cast<f32x4*>(dR + 4 * s) = o4;
    }
    wave_lds_sync();
}

// ------------------------------------------------------------------------------------------
// TRAIN, static net: the LDS bias region holds the canonical tiles alone (the deformation tiles' 11 KB are what lets the
// 16-deep ring of the training translation unit AND the resampling scratch fit into 160 KB).  TRAIN + DNERF keeps both
// tile sets and has no resampling scratch (the D-NeRF training pass runs on given depths: the coarse pass of the
// one-model configuration is a no_grad inference pass, d_nerf/run_dnerf.py:417-421).
template <bool DNERF, bool TRAIN> struct PassLds {
    // (TRAIN static: room for the larger of the canonical tile set, 97, and the no-view-direction set, 64 + 8 x 5 + 1 = 105)
    static constexpr int TRAIN_TILES = SW_NOVIEW_BIAS_TILES(SW_NOVIEW_MAX_OUT) > SW_CANON_BIAS_TILES ? SW_NOVIEW_BIAS_TILES(SW_NOVIEW_MAX_OUT) : SW_CANON_BIAS_TILES;
    static constexpr int BIAS = (TRAIN && !DNERF) ? TRAIN_TILES * SW_BIAS_TILE_FLOATS : SW_LDS_BIAS_FLOATS;
    static constexpr int FIXED = BIAS + 4 * SW_LDS_RING_FLOATS;
};
// PREC != 0 (bf16x3 / bf16 pass, mlp_core_x3.h): bias tiles | the workgroup's shared weight ring | per wave: gamma(d)
// tile + depth slots | per wave: resampling scratch
// (D-NeRF: both bias-tile sets, and no gamma(d) tile - x3_net_dn_pipe evaluates it - so that the resampling scratch still fits)
template <bool DNERF> struct X3Lds {
    static constexpr int BIAS = (DNERF ? SW_DEFORM_BIAS_TILES + SW_X3_CANON_BIAS_TILES : SW_X3_CANON_BIAS_TILES) * SW_BIAS_TILE_FLOATS;
    static constexpr int DIR = DNERF ? 0 : 16 * 64;
    static constexpr int WAVE = DIR + SW_ZSLOT_FLOATS;
    static constexpr int FIXED = BIAS + X3_RING_FLOATS + 4 * WAVE;
};

// ---- the steps of the tile loop, each written once (tnerf_pass.h runs the per-ray and compositing ones too) -----------------
// this lane's row of a tile: its sample, its lane of the half, the half, and whether the sample exists
struct TileRow { int s, j, h; bool live; };

// position_delta of sample s, by the lower lane half of a live row
__device__ __forceinline__ void pass_store_dx(const swnerf_pass_args& a, int64_t ray, int s, bool live, int h, float ex, float ey, float ez) {
    if (live && h == 0) {
        float* o = a.dx + (ray * a.n_samples + s) * 3;
        o[0] = ex; o[1] = ey; o[2] = ez;
    }
}

// TRAIN: this lane's padded row of the side buffers of one net (PassDev act / bits / xs); tix = ray * ntiles + tile
struct TrainRows { float* act_row; float* mask_tile; float* xs_row; };
__device__ __forceinline__ TrainRows train_rows(float* act, float* bits, float* xs, int64_t tix, int j, int h, int lane) {
    const int64_t prow = tix * 32 + j;
    return {act + prow * SW_ACT_LD + 4 * h, bits + tix * SW_MASK_TILE_FLOATS + lane * 4, xs + prow * SW_XS_LD + 4 * h};
}

// outputs = output_linear(h) (model.py:59-60) as VALU heads behind a NOHEAD trunk: [rgb(3), sigma, (5th, shown by `raw` alone)].
// nout <= out_ch channels are evaluated; the weight tiles of the others are skipped, so ws.bias ends at the head-bias tile.
__device__ __forceinline__ void noview_heads(const f32x16 (&in)[8], WStream& ws, int nout, int out_ch, float (&rgb)[3], float (&head)[3], float& extra) {
    float o5[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    head_valu_rt<8>(in, ws, nout, o5);
    ws.bias += (out_ch - nout) * 8 * SW_BIAS_TILE_FLOATS;
    rgb[0] = o5[0] + ws.bias[0]; rgb[1] = o5[1] + ws.bias[1]; rgb[2] = o5[2] + ws.bias[2];
    head[0] = o5[3] + ws.bias[3]; head[1] = 0.f; head[2] = 0.f;
    extra = o5[4] + ws.bias[4];
}

// raw2outputs on one tile, the density side (composite.h; both lane halves mirror each other): noise, alpha, the weight from the
// exclusive cumprod over the 32 lanes and the transmittance Tc carried across tiles ...
__device__ __forceinline__ float pass_weight(const swnerf_pass_args& a, int64_t ray, int s, int sc, bool live, int j, float sg, float z, float zn,
                                             float dnorm, double& Tc, float& alpha) {
    const int S = a.n_samples;
    if (a.noise) sg += a.noise[ray * S + sc];
    alpha = comp_alpha(sg, comp_dist(s + 1 < S, zn, z, dnorm), live);
    return alpha * comp_transmittance(excl_cumprod_shfl<32>(comp_survival(alpha), j), Tc);
}
// ... and the per-sample outputs of a live row, by its lower lane half
__device__ __forceinline__ void pass_store_wz(const swnerf_pass_args& a, int64_t ray, int s, int h, float w, float z) {
    if (a.weights && h == 0) a.weights[ray * a.n_samples + s] = w;
    if (a.z_out && h == 0) a.z_out[ray * a.n_samples + s] = z;
}

// after the last tile: the five sums over the 32 lanes (left in place: pa is acc); lane 0 of a wave that is no ghost writes the maps.
// (lane and ghost apart: the condition formed by the caller and handed in as one bool moved the s_waitcnt count of three kernels.)
__device__ __forceinline__ void pass_write_maps(float& pr, float& pg, float& pb, float& pd, float& pa, int lane, bool ghost,
                                                const swnerf_pass_args& a, int64_t ray, float* rgb_map) {
    pr = wave32_sum(pr); pg = wave32_sum(pg); pb = wave32_sum(pb);
    pd = wave32_sum(pd); pa = wave32_sum(pa);
    if (lane == 0 && !ghost) comp_write_maps(pr, pg, pb, pd, pa, a.white_bkgd, ray, rgb_map, a.disp_map, a.acc_map, a.depth_map);
}

// ---- the deferred colour branch, phase A (view_ws.h): a tile that stashes packs its lit rows' h7 (`in`) into the ray's region
// `vreg` behind the `wr` rows already there, in sample order, with each row's sample index; returns how many it added (wave-uniform)
__device__ __forceinline__ int defer_stash(const ViewWs& vw, float* vreg, const f32x16 (&in)[8], bool lit, int wr, const TileRow& t) {
    const unsigned m = (unsigned)__ballot(lit);          // lanes 0..31: one bit per row
    const int slot = wr + __popc(m & ((1u << t.j) - 1u));
    if (lit) {
        if (t.h == 0) vw_sample(vw, vreg)[slot] = t.s;
        float* q = vw_row(vw, vreg, slot, t.h);
        const int gs = vw_group_stride(vw);
#pragma unroll
        for (int c = 0; c < 32; ++c) {
            const f32x4 v = {in[c >> 2][4 * (c & 3)], in[c >> 2][4 * (c & 3) + 1], in[c >> 2][4 * (c & 3) + 2], in[c >> 2][4 * (c & 3) + 3]};
            *reinterpret_cast<f32x4*>(q + (size_t)c * gs) = v;
        }
    }
    return __builtin_amdgcn_readfirstlane(__popc(m));
}
// the region's raw colours of sample s: what the tile evaluated in line (`here`), 0 for a dead row and for a stashed one (phase B's)
__device__ __forceinline__ void defer_colours(const ViewWs& vw, float* vreg, const TileRow& t, bool here, float c0, float c1, float c2) {
    if (t.live && t.h == 0) {
        float* c = vw_c(vw, vreg);
        c[t.s] = here ? c0 : 0.f; c[vw.sp + t.s] = here ? c1 : 0.f; c[2 * vw.sp + t.s] = here ? c2 : 0.f;
    }
}

// PREC: 0 = fp32 MFMA (mlp_core.h, the parity path); 3 = bf16x3, 1 = plain bf16 (mlp_core_x3.h; static net, inference)
// VIEWS = false: the net without view directions (SWNERF_NET_NOVIEW; model.py:59-60, 8-column ray batch nerf/run.py:152-157):
// the trunk, then output_linear as VALU heads - no feature / view branch, no gamma(d).  Static net, fp32, inference or TRAIN.
template <bool DNERF, bool TRAIN = false, int PREC = 0, bool VIEWS = true>
__global__ void __launch_bounds__(256, 1) render_pass_kernel(PassDev P) {
    static_assert(PREC == 0 || !TRAIN, "the bf16 paths cover the inference passes");
    static_assert(VIEWS || (!DNERF && PREC == 0), "the no-view-direction variant is a static fp32 pass (inference or TRAIN)");
    extern __shared__ __attribute__((aligned(16))) float lds_all[];
    const swnerf_pass_args& a = P.a;
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t ray_id = (int64_t)blockIdx.x * 4 + wv;
    if constexpr (PREC == 0)                     // junk slot = this wave's parked-encoding region: nothing is parked before ws_start's wait
        pass_startup(P, P.w0, lds_all + PassLds<DNERF, TRAIN>::BIAS + wv * SW_LDS_RING_FLOATS + SW_RING * SW_STEP_FLOATS, lane, wv);
    bias_to_lds(lds_all, P.b0, P.nbias);         // fp32 path: the only block barrier; waves are independent after it
    // PREC: the four waves share the weight ring and run in step, so a wave past the last ray follows along on the
    // last ray and stores nothing
    const bool ghost = PREC != 0 && ray_id >= a.n_rays;
    if (PREC == 0 && ray_id >= a.n_rays) return; // wave-uniform
    const int64_t ray = ghost ? a.n_rays - 1 : ray_id;
    const float* lds_bias = lds_all;
    float* lds_ring = PREC ? lds_all + X3Lds<DNERF>::BIAS
                           : lds_all + PassLds<DNERF, TRAIN>::BIAS + wv * SW_LDS_RING_FLOATS;
    float* lds_emb = lds_ring + SW_RING * SW_STEP_FLOATS;
    float* lds_x3w = lds_ring + X3_RING_FLOATS + wv * X3Lds<DNERF>::WAVE;
    float* lds_dir = PREC ? lds_x3w : lds_emb + 2 * 16 * 64;
    float* lds_vb = lds_emb + SW_EMB_LDS_FLOATS + SW_ZSLOT_FLOATS;          // fp32, VIEWS: the per-ray init tiles of the view layer
    const float* lds_tb = (DNERF && PREC == 0 && P.time_steps) ? lds_all + P.tb_off + wv * SW_TB_LDS_FLOATS : nullptr;   // ... of _time.0
    float* lds = PREC ? lds_all + X3Lds<DNERF>::FIXED + wv * SW_LDS_WAVE_FLOATS
                      : lds_all + PassLds<DNERF, TRAIN>::FIXED + wv * SW_LDS_WAVE_FLOATS;
    float* zc = lds;                             // [S]   depths of this pass
    float* wc = lds + SW_LDS_SC;                 // [S]   compositing weights
    float* cdf = lds + 2 * SW_LDS_SC;            // [S-1]
    float* srt = lds + 3 * SW_LDS_SC;            // [sort_n]

    const int S = a.n_samples;
    const bool resample = a.n_importance > 0;
    const RayRow r = ray_row_load<VIEWS>(a.ray_batch + ray * a.cols, a.cols);

    WStream ws;
    XStream xs;
    if constexpr (PREC != 0) {
        if (!DNERF) {         // once per ray: the view-direction encoding, parked in LDS (see tile_park)
            f32x16 demb;
            pe_dir(r.v[0], r.v[1], r.v[2], h, demb);
            tile_park(lds_dir, lane, demb);
        }
        x3_start(xs, reinterpret_cast<const char*>(P.w0), lds_bias, lds_ring, lane, wv);
    } else {
        // ring prime first (its wait also retires the warm-up DMAs into the junk slot, vmcnt being in order), THEN the
        // view-direction encoding is parked where the junk went; its ~300 VALU cycles run while steps 1..7 are in flight
        ws_start(ws, P.w0, lds_bias, lds_ring, lane);
        if constexpr (VIEWS) {
            // the stream's DIR prefix, once per ray: c = Wv[:, 256:] gamma(d) + b_vf -> the view layer's init tiles (mlp_core.h)
            f32x16 demb;
            pe_dir(r.v[0], r.v[1], r.v[2], h, demb);
            if constexpr (TRAIN) tile_park(lds_dir, lane, demb);               // the training passes also store gamma(d) per row (xs)
            ray_init_tile<4>(demb, lds_vb, lane, ws);
        }
        // D-NeRF with the deformation pass: the stream's TIME segment, once per ray: _time.0.bias + its gamma(t) columns (mlp_core.h)
        if constexpr (DNERF) {
            if (P.time_steps) {
                f32x16 temb;
                pe_time(r.ft, h, temb);
                ray_init_tile<8>(temb, lds_all + P.tb_off + wv * SW_TB_LDS_FLOATS, lane, ws);
            }
        }
    }

    const float* zrow = a.z_vals ? a.z_vals + ray * S : nullptr;
    const float* zslot = PREC ? lds_x3w + X3Lds<DNERF>::DIR : lds_emb + SW_EMB_LDS_FLOATS;
    const unsigned zslot_addr = __builtin_amdgcn_readfirstlane((unsigned)(size_t)zslot);
    float pr = 0.f, pg = 0.f, pb = 0.f, pd = 0.f, pa = 0.f;
    double Tc = 1.0;                              // transmittance carried across tiles
    const int ntiles = (S + 31) >> 5;
    // the deferred colour branch (view_ws.h); DEFER_OK = false compiles every line of it away
    constexpr bool DEFER_OK = !DNERF && !TRAIN && PREC == 0 && VIEWS;
    const bool defer = DEFER_OK && P.vw.base != nullptr;
    float* vreg = defer ? vw_ray(P.vw, ray) : nullptr;                     // this ray's region of the workspace
    const char* main_head = reinterpret_cast<const char*>(P.w0 + (P.dir_steps + P.time_steps) * SW_STEP_FLOATS);
    int wr = 0;                                   // wave-uniform: rows stashed so far
#pragma nounroll
    for (int tile = 0; tile < ntiles; ++tile) {
        // this tile stashes its live rows and leaves the view segment out: all the rows it may hold are certain to fit
        const bool stash = defer && wr + min(32, S - tile * 32) <= P.vw.rows;
        const int s = tile * 32 + j;
        const bool live = s < S && !ghost;
        const int sc = live ? s : S - 1;
        const TileRow t = {s, j, h, live};

        // ---- depths
        float z, zn;
        if (zrow && tile > 0) {
            // depths given (fine pass): fetched by LDS-DMA while the previous tile's MLP ran - issued before that
            // tile's weight stream, so long landed - instead of a global load whose latency every tile would expose
            const float* zs = zslot + (tile & 1) * 64;
            z = zs[j];
            const float z1 = zs[j + 1];
            zn = (s + 1 < S) ? z1 : z;
        } else {
            z = z_sample(a, ray, r.near, r.far, sc);
            zn = (s + 1 < S) ? z_sample(a, ray, r.near, r.far, s + 1) : z;
        }
        if (zrow && tile + 1 < ntiles)
            lds_dma_dword(reinterpret_cast<const char*>(zrow), (unsigned)min(32 * (tile + 1) + lane, S - 1) * 4u,
                          zslot_addr + (unsigned)((tile + 1) & 1) * 256u);

        // ---- the net on pts = rays_o + rays_d * z  (two roundings, nerf/run.py:385): one branch per instantiation.  On leaving it
        // head[0] = sigma; rgb = the raw colours, except in the fp32 inference passes with view directions, which leave `in` =
        // relu(h7) to the colour stage below.  (In line ON PURPOSE: as one __forceinline__ function this stage moves the registers of five
        // kernels, <true, true> 508 -> 504, <false, true> 420 -> 419, <true> 394 -> 392, the bf16 <true> pair +4 / +2 - profiles/pass_stages.md.)
        f32x16 in[8];
        float head[3], rgb[3];
        float extra = 0.f;                          // VIEWS = false, out_ch == 5: the fifth channel of output_linear (only `raw` shows it)
        float px = r.o[0] + r.d[0] * z, py = r.o[1] + r.d[1] * z, pz = r.o[2] + r.d[2] * z;
        f32x16 emb[2], out[8];
        pe_pos(px, py, pz, h, emb);
        if constexpr (DNERF && PREC != 0) {
            // (the dx stores stay in line here: with pass_store_dx the two bf16 D-NeRF kernels went from 425 / 449 to 420 / 443 registers)
#pragma nounroll
            for (int pass = P.two_pass ? 0 : 1; pass < 2; ++pass) {
                x3_net_dn_pipe<PREC>(px, py, pz, r.ft, pass == 0, h, r.v[0], r.v[1], r.v[2], head, rgb, xs);
                if (pass == 0) {
                    const float ex = head[0], ey = head[1], ez = head[2];
                    if (a.dx && live && h == 0) {
                        float* o = a.dx + (ray * S + s) * 3;
                        o[0] = ex; o[1] = ey; o[2] = ez;
                    }
                    px = px + ex; py = py + ey; pz = pz + ez;            // re-embedded inside the canonical pass
                }
            }
            if (!P.two_pass && a.dx && live && h == 0) {
                float* o = a.dx + (ray * S + s) * 3;
                o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
            }
            x3_rewind(xs, P.two_pass ? SW_X3_DEFORM_CHUNKS + SW_X3_CANON_CHUNKS : SW_X3_CANON_CHUNKS, lds_bias, lane);
        } else if constexpr (DNERF) {
            // deformation net, then the canonical net on gamma(x + dx) (model.py:128-151).  TRAIN: always both passes (the t == 0 /
            // zero_canonical case trains the canonical net alone through the static kernel), and both nets save what their dX
            // chains and weight-gradient GEMMs need, as side stores (see the static branch below).
            TrainRows rc = {}, rd = {};             // the canonical net's rows, the deformation net's
            if constexpr (TRAIN) {
                rc = train_rows(P.act, P.bits, P.xs, ray * ntiles + tile, j, h, lane);
                rd = train_rows(P.act_d, P.bits_d, P.xs_d, ray * ntiles + tile, j, h, lane);
            }
            f32x4 mb = {0.f, 0.f, 0.f, 0.f};
            // ONE call site for both nets (a runtime loop): two would unroll the 8-layer body twice - 4800 static MFMAs, beyond
            // what the instruction cache holds comfortably
#pragma nounroll
            for (int pass = (TRAIN || P.two_pass) ? 0 : 1; pass < 2; ++pass) {
                const bool dp = pass == 0;
                trunk_pass_flat<true, TRAIN, TRAIN, false, true, false>(emb, lds_emb, r.ft, dp, h, in, out, head, ws,      // flat: see mlp_core.h
                                             dp ? rd.act_row : rc.act_row, dp ? rd.mask_tile : rc.mask_tile, dp, &mb,
                                             dp ? rd.xs_row : rc.xs_row, lds_tb, nullptr);
                if (dp) {
                    // dx = _time_out(h) (model.py:136,146-149)
                    const float ex = head[0], ey = head[1], ez = head[2];
                    if (TRAIN || a.dx) pass_store_dx(a, ray, s, live, h, ex, ey, ez);
                    px = px + ex; py = py + ey; pz = pz + ez;
                    pe_pos(px, py, pz, h, emb);                              // re-embed (model.py:148-149)
                    if constexpr (TRAIN) {
                        f32x16 demb;
                        tile_fetch(lds_dir, lane, demb);
                        xs_store_tile(rc.xs_row + 64, demb);
                    }
                }
            }
            if constexpr (TRAIN) canon_tail<true>(in, lds_vb, rgb, ws.bias - SW_BIAS_TILE_FLOATS, ws, TrunkSide{rc.act_row, rc.mask_tile, false, &mb, rc.xs_row});
            else if (!P.two_pass && a.dx) pass_store_dx(a, ray, s, live, h, 0.f, 0.f, 0.f);       // model.py:144-145
        } else if constexpr (PREC != 0) {
            head[1] = 0.f; head[2] = 0.f;
            x3_canon_pipe<PREC>(px, py, pz, h, lds_dir, lane, head[0], rgb, xs);
            x3_rewind(xs, SW_X3_CANON_CHUNKS, lds_bias, lane);
        } else {
            // the static fp32 net.  TRAIN: everything the backward needs goes out as side stores of the segments (mlp_core.h
            // SideStore): gamma(x) with layer 0, h_l and its ReLU mask with layer l+1, h7 with the view layer (VIEWS = false: on the
            // spot, no segment follows it), gamma(d) here.  Inference with view directions: a tile that leaves the view segment out
            // continues at the head of MAIN behind layer 7.
            f32x4 mb = {0.f, 0.f, 0.f, 0.f};
            TrunkSide side = {};
            if constexpr (TRAIN) {
                const TrainRows rc = train_rows(P.act, P.bits, P.xs, ray * ntiles + tile, j, h, lane);
                side = TrunkSide{rc.act_row, rc.mask_tile, !VIEWS, &mb, rc.xs_row};
                if constexpr (VIEWS) {
                    f32x16 demb;
                    tile_fetch(lds_dir, lane, demb);
                    xs_store_tile(side.xs_row + 64, demb);                   // gamma(d): k-tile 2 of the slot-ordered row
                }
            }
            trunk_pass<false, TRAIN, TRAIN, !VIEWS, false, !TRAIN && VIEWS>(emb, lds_emb, 0.f, false, h, in, out, head, ws, side, nullptr,
                                                                            stash ? main_head : nullptr);
            // outputs = output_linear(h) (model.py:59-60): [rgb(3), sigma, (5th: only `raw` of an inference launch shows it)]
            if constexpr (!VIEWS) noview_heads(in, ws, (!TRAIN && a.out_ch == 5 && !a.raw) ? 4 : a.out_ch, a.out_ch, rgb, head, extra);
            else if constexpr (TRAIN) canon_tail<true>(in, lds_vb, rgb, ws.bias - SW_BIAS_TILE_FLOATS, ws, side);
        }

        // ---- raw2outputs on this tile, the density side
        const float sg_raw = head[0];
        float alpha;
        const float w = pass_weight(a, ray, s, sc, live, j, sg_raw, z, zn, r.dnorm, Tc, alpha);
        if (live) {
            pass_store_wz(a, ray, s, h, w, z);
            if (resample && h == 0) { zc[s] = z; wc[s] = w; }
        }
        comp_accumulate_density(w, z, pd, pa);

        // ---- the colour branch of the fp32 inference passes with view directions: stashed for phase B, or in line
        bool lit = live;                             // this row's colour enters the outputs
        if constexpr (DEFER_OK) {
            if (defer) {
                lit = live && (!(alpha == 0.f) || s == 0);
                if (live && h == 0) vw_w(vreg)[s] = w;
                if (stash) wr += defer_stash(P.vw, vreg, in, lit, wr, t);
            }
        }
        if constexpr (!TRAIN && PREC == 0 && VIEWS) {
            if (!stash) {
                if constexpr (DEFER_OK) ws.cont = ws.base + SW_STEPS_VIEWSH * 1024;
                canon_tail<false, DEFER_OK>(in, lds_vb, rgb, ws.bias - SW_BIAS_TILE_FLOATS, ws);
            } else {
                rgb[0] = 0.f; rgb[1] = 0.f; rgb[2] = 0.f;
            }
        }
        if constexpr (PREC == 0) {               // back to the head of MAIN: behind the per-ray prefixes (DIR with its b_vf tiles, TIME with its 8 bias tiles)
            ws_rewind(ws, P.w0 + (P.dir_steps + P.time_steps) * SW_STEP_FLOATS,
                      lds_bias + ((P.dir_steps ? SW_DIR_BIAS_TILES : 0) + (P.time_steps ? 8 : 0)) * SW_BIAS_TILE_FLOATS, lane);
        }

        // ---- outputs: the colours to the ray's region (phase B adds the stashed rows', phase C forms the sums), or raw and the colour sums
        const float c0 = rgb[0], c1 = rgb[1], c2 = rgb[2];
        if (DEFER_OK && defer) {
            defer_colours(P.vw, vreg, t, lit && !stash, c0, c1, c2);
        } else {
            if (a.raw && live && h == 0) {
                if (!VIEWS && a.out_ch == 5) {
                    float* o = a.raw + (ray * S + s) * 5;
                    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = sg_raw; o[4] = extra;
                } else {
                    f32x4 r4 = {c0, c1, c2, sg_raw};
                    *reinterpret_cast<f32x4*>(a.raw + (ray * S + s) * 4) = r4;
                }
            }
            comp_accumulate_colour(w, c0, c1, c2, pr, pg, pb);
        }
    }

    pass_write_maps(pr, pg, pb, pd, pa, lane, ghost, a, ray, defer ? nullptr : a.rgb_map);
    if constexpr (DEFER_OK) {
        if (defer && lane == 0) { vw_off(P.vw)[ray] = wr; vreg[0] = pa; }
    }
    if (!resample || ghost) return;

    // ---- sample_pdf (ray.py:96-153) on bins = mid-points, weights[1:-1]; z_std; then sort (nerf/run.py:396-400, 416) as a rank
    // merge - the wave-level routines of resample.h, shared with the standalone op
    wave_lds_sync();
    const int Ni = a.n_importance;
    const double sm = wave_sample_pdf(wc + 1, S - 1, MidBins{zc}, a.u ? a.u + ray * Ni : nullptr, Ni, cdf, srt, lane);
    if (a.z_std) {
        const float sd = wave_zstd(sm, srt, Ni, lane);
        if (lane == 0) a.z_std[ray] = sd;
    }
    wave_rank_merge(zc, S, P.sort_s, srt, Ni, P.sort_n, a.z_fine + ray * (S + Ni), lane);
}
