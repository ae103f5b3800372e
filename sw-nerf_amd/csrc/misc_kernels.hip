// misc_kernels.hip - the HBM-bound satellites of the render path as standalone gfx950
// kernels (API parity with ray.py / embedder.py; the fused pass in render_kernels.hip does
// the same arithmetic in registers).  All are elementwise or one-wave-per-ray, coalesced.
#include <hip/hip_runtime.h>
#include "../../include/swnerf.h"
#include "swnerf_common.h"
#include "host_util.h"
#include "ray_rows.h"
#include "resample.h"
#include "composite.h"

static thread_local char g_err[SW_ERRBUF_LEN] = "";
char* sw_errbuf() { return g_err; }
extern "C" const char* swnerf_last_error(void) { return g_err; }
extern "C" int swnerf_version(void) { return SWNERF_VERSION; }
extern "C" size_t swnerf_packed_floats(int kind) {
    return kind == SWNERF_NET_CANON ? (size_t)SW_CANON_FLOATS
         : (kind == SWNERF_NET_DNERF ? (size_t)SW_DNERF_FLOATS : (kind == SWNERF_NET_NOVIEW ? (size_t)SW_NOVIEW_FLOATS
         : (kind == SWNERF_NET_TNERF ? (size_t)SW_TN_FLOATS : 0)));
}

static inline unsigned nblocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// ---- get_rays (ray.py:10-38) ---------------------------------------------------------------
// the arithmetic of a ray, of the NDC warp and of a batch row: ray_rows.h (shared with batch_kernels.hip)
__global__ void __launch_bounds__(256) get_rays_kernel(Cam c, int W, int64_t ray0, int64_t n, float* ro, float* rd) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t p = ray0 + i;
    ray_dir(c, (float)(p % W), (float)(p / W), rd[i * 3 + 0], rd[i * 3 + 1], rd[i * 3 + 2]);
    if (ro) { ro[i * 3 + 0] = c.t[0]; ro[i * 3 + 1] = c.t[1]; ro[i * 3 + 2] = c.t[2]; }
}

extern "C" int swnerf_get_rays(int H, int W, double fx, double fy, double cx, double cy, int focal_branch,
                               const float* c2w, int64_t ray0, int64_t n, float* rays_o, float* rays_d, void* stream) {
    if (n == 0 && H > 0 && W > 0) return 0;
    if (!c2w || !rays_d || H <= 0 || W <= 0 || n < 0 || ray0 < 0 || ray0 + n > (int64_t)H * W)
        return sw_fail(SWNERF_E_ARG, "get_rays: bad arguments (H=%d W=%d ray0=%lld n=%lld)", H, W, (long long)ray0, (long long)n);
    Cam c;
    cam_intrinsics(c, H, W, fx, fy, cx, cy, focal_branch);
    cam_pose(c, c2w);
    if (n == 0) return 0;
    hipLaunchKernelGGL(get_rays_kernel, dim3(nblocks(n, 256)), dim3(256), 0, (hipStream_t)stream, c, W, ray0, n, rays_o, rays_d);
    return sw_check(hipGetLastError(), "get_rays launch");
}

// ---- ndc_rays (ray.py:75-92) -----------------------------------------------------------------
__global__ void __launch_bounds__(256) ndc_kernel(float sx, float sy, float near, const float* ro, const float* rd,
                                                  int64_t n, float* oo, float* od) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float ox = ro[i * 3], oy = ro[i * 3 + 1], oz = ro[i * 3 + 2], dx = rd[i * 3], dy = rd[i * 3 + 1], dz = rd[i * 3 + 2];
    ndc_one(sx, sy, near, ox, oy, oz, dx, dy, dz);
    oo[i * 3] = ox; oo[i * 3 + 1] = oy; oo[i * 3 + 2] = oz;
    od[i * 3] = dx; od[i * 3 + 1] = dy; od[i * 3 + 2] = dz;
}

extern "C" int swnerf_ndc_rays(int H, int W, double focal, double near, const float* rays_o, const float* rays_d,
                               int64_t n, float* o_out, float* d_out, void* stream) {
    if (n == 0) return 0;
    if (!rays_o || !rays_d || !o_out || !d_out || n < 0) return sw_fail(SWNERF_E_ARG, "ndc_rays: NULL pointer / negative n");
    hipLaunchKernelGGL(ndc_kernel, dim3(nblocks(n, 256)), dim3(256), 0, (hipStream_t)stream,
                       ndc_scale(W, focal), ndc_scale(H, focal), (float)near, rays_o, rays_d, n, o_out, d_out);
    return sw_check(hipGetLastError(), "ndc_rays launch");
}

// ---- ray batch packing (nerf/run.py:137-158, d_nerf/run_dnerf.py:137-160) ----------------------
// A block packs 256 rays: the 11- / 12-float rows are assembled in LDS (pack_row) and leave as 16-byte stores
// (rows_to_global, ray_rows.h).
__global__ void __launch_bounds__(256) pack_rays_kernel(const float* ro, const float* rd, int64_t n, float near, float far,
                                                        int has_time, float ft, int ndc, float sx, float sy, float* out) {
    __shared__ __attribute__((aligned(16))) float rows[256 * 12];
    const int t = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * 256, i = i0 + t;
    const int cols = has_time ? 12 : 11;
    if (i < n)
        pack_row(rows + t * cols, cols, ro[i * 3], ro[i * 3 + 1], ro[i * 3 + 2], rd[i * 3], rd[i * 3 + 1], rd[i * 3 + 2],
                 near, far, ft, ndc, sx, sy);
    __syncthreads();
    rows_to_global(rows, out, i0, n, cols, t);
}

extern "C" int swnerf_pack_ray_batch(const float* rays_o, const float* rays_d, int64_t n, double near, double far,
                                     int has_time, double frame_time, int ndc, int H, int W, double ndc_focal,
                                     float* ray_batch, void* stream) {
    if (n == 0) return 0;
    if (!rays_o || !rays_d || !ray_batch || n < 0) return sw_fail(SWNERF_E_ARG, "pack_ray_batch: NULL pointer / negative n");
    const float sx = ndc ? ndc_scale(W, ndc_focal) : 0.f, sy = ndc ? ndc_scale(H, ndc_focal) : 0.f;
    hipLaunchKernelGGL(pack_rays_kernel, dim3(nblocks(n, 256)), dim3(256), 0, (hipStream_t)stream, rays_o, rays_d, n,
                       (float)near, (float)far, has_time, (float)frame_time, ndc, sx, sy, ray_batch);
    return sw_check(hipGetLastError(), "pack_ray_batch launch");
}

// ---- Embedder.embed (embedder.py:33-42) --------------------------------------------------------
// out[row] = [x, sin(2^0 x), cos(2^0 x), ..., sin(2^(L-1) x), cos(2^(L-1) x)], blocks d wide.  VALU-issue bound, not HBM
// bound, once the stores are coalesced: what counts is instructions per output float.  A workgroup builds the image of
// EMB_ROWS output rows in LDS - one job per (row, band, component) evaluates the sine AND the cosine of its argument with one
// reduction (sw_embed_sincos: the bits of sw_sin_or_cos for the bands k < 10 the fused kernels have, the reduction in double for
// the bands above, where the float one fails - all 24 accepted bands within 1.2e-7 of libm at |x| <= 6, tests/test_host_math.py
// and tests/test_gpu_op_domain.py), one job per (row, component) copies x - and the image, contiguous in
// the output and 16-byte aligned, leaves as float4 stores.  Job -> (row, slot) by a multiply-shift (q_magic = ceil(2^24 / Q),
// exact for the jobs of a block - checked on the host for every accepted (d, L); the 64-bit division per element of the round 1-3 kernel cost more than the sin/cos).
// WIDE = some band k >= SW_SINCOS_F32_BANDS (L > 10): only that instantiation carries the double reduction; L <= 10 - every
// embedder the reference builds - runs the float-only kernel, instruction for instruction what it was before the bands above 10 were fixed.
#define EMB_ROWS 64
template <bool WIDE>
__global__ void __launch_bounds__(256) embed_kernel(const float* x, int64_t M, int d, int L, int R, unsigned q_magic, unsigned d_magic, float* out) {
    extern __shared__ __attribute__((aligned(16))) float emb_img[];           // [rows][C]
    const int C = d * (1 + 2 * L), Q = d * (1 + L);                             // jobs per row: d copies + d * L (sin, cos) pairs
    const int64_t row0 = (int64_t)blockIdx.x * R;                             // R <= EMB_ROWS rows per workgroup (fewer for very wide rows: LDS)
    const int rows = (int)min((int64_t)R, M - row0);
    const float* xb = x + row0 * d;
    for (unsigned j = threadIdx.x; j < (unsigned)(rows * Q); j += 256) {
        const unsigned row = (j * q_magic) >> 24, q = j - row * (unsigned)Q;
        float* o = emb_img + row * C;
        if (q < (unsigned)d) {
            o[q] = xb[row * d + q];
        } else {
            const unsigned p = q - d, k = (p * d_magic) >> 24, c = p - k * (unsigned)d;
            float sv, cv;
            if (WIDE) sw_embed_sincos(xb[row * d + c], (int)k, &sv, &cv);   // bands >= 10 reduce in double (swnerf_common.h)
            else sw_sincos_pair(xb[row * d + c] * (float)(1 << k), &sv, &cv);   // = sw_embed_sincos for k < 10; x * 2^k is exact (embedder.py:29,36)
            o[d + 2 * k * d + c] = sv;
            o[d + 2 * k * d + d + c] = cv;
        }
    }
    __syncthreads();
    float* dst = out + row0 * C;
    const int total = rows * C;
    if ((total & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        for (int i = threadIdx.x; i < total / 4; i += 256) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(emb_img)[i];
    } else {
        for (int i = threadIdx.x; i < total; i += 256) dst[i] = emb_img[i];
    }
}

extern "C" int swnerf_embed(const float* x, int64_t M, int d, int L, float* out, void* stream) {
    if (M == 0 && d > 0 && L >= 0) return 0;
    if (!x || !out || M < 0 || d <= 0 || d > 16 || L < 0 || L > 24) return sw_fail(SWNERF_E_ARG, "embed: bad arguments (M=%lld d=%d L=%d; d <= 16, L <= 24)", (long long)M, d, L);
    const int C = d * (1 + 2 * L), Q = d * (1 + L);
    const unsigned q_magic = ((1u << 24) + Q - 1) / Q, d_magic = ((1u << 24) + d - 1) / d;   // floor(n / Q) = (n * q_magic) >> 24 for n * Q < 2^24
    int R = EMB_ROWS;
    while (R > 1 && (size_t)R * C * sizeof(float) > 64 * 1024) R >>= 1;
    if (L > SW_SINCOS_F32_BANDS)
        hipLaunchKernelGGL(embed_kernel<true>, dim3(nblocks(M, R)), dim3(256), (size_t)R * C * sizeof(float), (hipStream_t)stream,
                           x, M, d, L, R, q_magic, d_magic, out);
    else
        hipLaunchKernelGGL(embed_kernel<false>, dim3(nblocks(M, R)), dim3(256), (size_t)R * C * sizeof(float), (hipStream_t)stream,
                           x, M, d, L, R, q_magic, d_magic, out);
    return sw_check(hipGetLastError(), "embed launch");
}

// ---- raw2outputs (ray.py:155-198): one wave per ray, 64 samples per sweep ------------------------
// Loads: raw as one float4 per lane (1 KiB per wave instruction), z one dword per lane; the next sample's depth comes from the
// lane above (DPP), only lane 63 loads it.  The exclusive cumprod runs in double like ATen's CPU cumprod, on the DPP path
// (wave_dpp.h: this kernel is VALU-issue bound - 3 sigmoids and an exp per sample - so a scan step must not cost eight
// instructions and two LDS round trips); the transmittance carried from sweep to sweep is wave-uniform.
__global__ void __launch_bounds__(256) raw2outputs_kernel(const float* raw, const float* zv, const float* rd, const float* noise,
                                                          int64_t N, int S, int white, float* rgb_map, float* disp, float* acc,
                                                          float* weights, float* depth) {
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= N) return;
    const float dx = rd[ray * 3], dy = rd[ray * 3 + 1], dz = rd[ray * 3 + 2];
    const float dnorm = sqrtf(dx * dx + dy * dy + dz * dz);
    const float* zr = zv + ray * S;
    const float4* rr = reinterpret_cast<const float4*>(raw) + ray * S;
    const float* nr = noise ? noise + ray * S : nullptr;
    float* wr = weights ? weights + ray * S : nullptr;
    float pr = 0.f, pg = 0.f, pb = 0.f, pd = 0.f, pa = 0.f;
    double Tc = 1.0;                                      // wave-uniform
    for (int base = 0; base < S; base += 64) {
        const int s = base + lane;
        const bool live = s < S;
        const int sc = live ? s : S - 1;
        const float4 r4 = rr[sc];
        const float z = zr[sc];
        const float z_edge = (lane == 63 && s + 1 < S) ? zr[s + 1] : 0.f;
        const float zn = wave_from_above_f32(z, z_edge);          // a cross-lane read: never under a lane-dependent branch
        const float dist = comp_dist(s + 1 < S, zn, z, dnorm);
        float sg = r4.w;
        if (nr) sg += nr[sc];
        const float alpha = comp_alpha(sg, dist, live);
        const float w = alpha * comp_transmittance(excl_cumprod_dpp64(comp_survival(alpha)), Tc);
        if (live && wr) wr[s] = w;
        comp_accumulate(w, r4.x, r4.y, r4.z, z, pr, pg, pb, pd, pa);
    }
    pr = wave_sum_to_last_f32(pr); pg = wave_sum_to_last_f32(pg); pb = wave_sum_to_last_f32(pb);
    pd = wave_sum_to_last_f32(pd); pa = wave_sum_to_last_f32(pa);
    if (lane == 63) comp_write_maps(pr, pg, pb, pd, pa, white, ray, rgb_map, disp, acc, depth);
}

extern "C" int swnerf_raw2outputs(const float* raw, const float* z_vals, const float* rays_d, const float* noise, int64_t N, int S,
                                  int white_bkgd, float* rgb_map, float* disp_map, float* acc_map, float* weights,
                                  float* depth_map, void* stream) {
    if (S == 1) return sw_fail(SWNERF_E_UNSUPP, "raw2outputs: S=1 is degenerate in the reference (ray.py:170-171 builds an EMPTY dists tensor); need S>=2");
    if (N == 0 && S >= 2) return 0;
    if (!raw || !z_vals || !rays_d || N < 0 || S < 2) return sw_fail(SWNERF_E_ARG, "raw2outputs: bad arguments (N=%lld S=%d)", (long long)N, S);
    hipLaunchKernelGGL(raw2outputs_kernel, dim3(nblocks(N, 4)), dim3(256), 0, (hipStream_t)stream, raw, z_vals, rays_d, noise, N, S,
                       white_bkgd, rgb_map, disp_map, acc_map, weights, depth_map);
    return sw_check(hipGetLastError(), "raw2outputs launch");
}

// ---- sample_pdf (ray.py:96-153) [+ sort(cat[z_vals, samples]), nerf/run.py:400] -------------------
// One wave per ray, four rays per workgroup, each wave in its own LDS slice (no block barrier anywhere): the operands are staged
// into LDS with coalesced loads, then the wave-level routines of resample.h run - the code of the fused render pass, bit for bit.
// Slice layout (floats): w[nb-1 -> nbp] | bins[nbp] | cdf[nbp] | z[sort_s] | samples[sort_n]   (nbp = nb rounded up to 4)
#define SP_MAX_BINS 1024
#define SP_MAX_SORT 2048
__global__ void __launch_bounds__(256) sample_pdf_kernel(const float* bins, const float* wts, int64_t N, int nb, int ns,
                                                         const float* u_in, float* samples, const float* zv, int S,
                                                         float* z_sorted, float* z_std, int sort_s, int sort_n, int slice) {
    extern __shared__ __attribute__((aligned(16))) float sp_lds[];
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= N) return;                                  // wave-uniform
    const int nbp = (nb + 3) & ~3;
    float* w = sp_lds + (threadIdx.x >> 6) * slice;
    float* b = w + nbp;
    float* cdf = b + nbp;
    float* z = cdf + nbp;
    float* smp = z + sort_s;
    for (int i = lane; i < nb - 1; i += 64) w[i] = wts[ray * (nb - 1) + i];
    for (int i = lane; i < nb; i += 64) b[i] = bins[ray * nb + i];
    if (z_sorted) for (int i = lane; i < S; i += 64) z[i] = zv[ray * S + i];
    wave_lds_sync();
    const double sm = wave_sample_pdf(w, nb, ArrayBins{b}, u_in ? u_in + ray * ns : nullptr, ns, cdf, smp, lane);
    for (int m = lane; m < ns; m += 64) samples[ray * ns + m] = smp[m];      // in draw order (ray.py:150-151), before any sort
    if (z_std) {
        const float sd = wave_zstd(sm, smp, ns, lane);
        if (lane == 0) z_std[ray] = sd;
    }
    if (z_sorted) wave_rank_merge(z, S, sort_s, smp, ns, sort_n, z_sorted + ray * (S + ns), lane);
}

extern "C" int swnerf_sample_pdf(const float* bins, const float* weights, int64_t N, int nb, int n_samples, const float* u,
                                 float* samples, const float* z_vals, int S, float* z_sorted, float* z_std, void* stream) {
    if (N == 0 && nb >= 2 && n_samples >= 1) return 0;
    if (!bins || !weights || !samples || N < 0 || nb < 2 || n_samples < 1)
        return sw_fail(SWNERF_E_ARG, "sample_pdf: bad arguments (N=%lld nb=%d n_samples=%d)", (long long)N, nb, n_samples);
    if (nb > SP_MAX_BINS) return sw_fail(SWNERF_E_UNSUPP, "sample_pdf: at most %d bins", SP_MAX_BINS);
    if (n_samples > SP_MAX_SORT) return sw_fail(SWNERF_E_UNSUPP, "sample_pdf: at most %d samples per ray", SP_MAX_SORT);
    int sort_s = 0, sort_n = 2;
    while (sort_n < n_samples) sort_n <<= 1;               // the sample buffer doubles as the fallback sort's power-of-two pad
    if (z_sorted) {
        if (!z_vals || S < 1 || S + n_samples > SP_MAX_SORT) return sw_fail(SWNERF_E_UNSUPP, "sample_pdf: sort needs z_vals and S+n_samples <= %d", SP_MAX_SORT);
        sort_s = 2;
        while (sort_s < S) sort_s <<= 1;
    }
    if (N == 0) return 0;
    const int nbp = (nb + 3) & ~3;
    const int slice = 3 * nbp + sort_s + sort_n;
    const size_t lds = (size_t)4 * slice * sizeof(float);  // <= 4 x (3 x 1024 + 2048 + 2048) x 4 B = 112 KiB
    hipLaunchKernelGGL(sample_pdf_kernel, dim3(nblocks(N, 4)), dim3(256), lds, (hipStream_t)stream, bins, weights, N, nb, n_samples, u,
                       samples, z_vals, S, z_sorted, z_std, sort_s, sort_n, slice);
    return sw_check(hipGetLastError(), "sample_pdf launch");
}
