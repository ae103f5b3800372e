// metrics_kernels.hip - image-quality metrics of rendered frames against ground truth: MSE / PSNR and two SSIM variants,
// batched over [N, H, W, 3] fp32 HWC frames (what render_path returns).  The reference scores a model with
// skimage.metrics (nerf/run.py calculate_metrics :49-61) and with the SSIM class of d_nerf/metrics.ipynb; neither package is
// available on the GPU stack.  Four launches on the caller's stream, no host synchronisation, no atomics, fixed
// reduction orders (results are bit-identical from run to run):
//   stats        grid (SB, N): per block min / max of gt and pred (NaN propagates like np.max) and the fp64 sum of the
//                squared fp32 differences; 16-byte loads where pred and gt share an alignment
//   stats finish one workgroup: per image MSE, data range R, PSNR, C1 = (0.01 R)^2, C2 = (0.03 R)^2
//   ssim         grid (tiles, N): one workgroup per (image, 64 x 16 output tile); input tile + halo of both images in LDS;
//                one thread per (output column, channel) walks down the tile: horizontal window sums of x, y, x^2, y^2,
//                xy from LDS, vertical sums in a register ring, then the per-pixel S; window sums and S in fp64
//                (x*y of two floats is exact in fp64); an fp64 partial per block, optionally the S map
//   ssim finish  one workgroup: per image the tile partials in tile order / (3 Ho Wo)
// Both modes reduce over valid windows only: skimage's crop by (7-1)/2 on each side leaves exactly the pixels whose 7x7
// window lies inside the image, so its `reflect` padding never reaches the mean.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/swnerf.h"
#include "host_util.h"

#define MT_STATS_THREADS 256
#define MT_TW 64                       // output columns per SSIM tile
#define MT_TH 16                       // output rows per SSIM tile
#define MT_SSIM_THREADS (MT_TW * 3)    // one thread per (output column, channel)
#define MT_MAX_SB 64                   // stats blocks per image at most
#define MT_MAX_GRID_Y 65535

struct MtDims {
    int64_t n, h, w, m;                // m = h * w * 3 floats per image
    int64_t ho, wo, tx, tiles;         // valid-window output size, tiles per output row, tiles per image
    int sb, win;                       // stats blocks per image; window size
};

struct MtWeights { double g[11]; };    // 1-D window weights (GAUSS11 only)

struct MtWs { double* sse; float* mm; double* cc; double* part; };

static inline int64_t mt_round256(int64_t b) { return (b + 255) & ~(int64_t)255; }

static MtDims mt_dims(int64_t n, int64_t h, int64_t w, int mode) {
    MtDims d{};
    d.n = n; d.h = h; d.w = w; d.m = h * w * 3;
    d.win = mode == SWNERF_SSIM_GAUSS11 ? 11 : 7;
    d.ho = h - d.win + 1; d.wo = w - d.win + 1;
    d.tx = (d.wo + MT_TW - 1) / MT_TW;
    d.tiles = d.tx * ((d.ho + MT_TH - 1) / MT_TH);
    const int64_t sb = (d.m + 4 * MT_STATS_THREADS * 16 - 1) / (4 * MT_STATS_THREADS * 16);
    d.sb = (int)(sb < 1 ? 1 : (sb > MT_MAX_SB ? MT_MAX_SB : sb));
    return d;
}

// workspace: sse double [N*SB] | min/max float [N*SB*4] | C1, C2 double [N*2] | SSIM tile partials double [N*tiles]
static MtWs mt_ws(void* ws, const MtDims& d) {
    char* p = (char*)ws;
    MtWs w;
    w.sse = (double*)p;   p += mt_round256(8 * d.n * d.sb);
    w.mm = (float*)p;     p += mt_round256(16 * d.n * d.sb);
    w.cc = (double*)p;    p += mt_round256(16 * d.n);
    w.part = (double*)p;
    return w;
}

__device__ __forceinline__ float mt_nanmax(float m, float v) { return (m != m) ? m : ((v != v || v > m) ? v : m); }
__device__ __forceinline__ float mt_nanmin(float m, float v) { return (m != m) ? m : ((v != v || v < m) ? v : m); }
// np.clip(pred, 0, 1): NaN stays NaN
__device__ __forceinline__ float mt_clip(float p, int clip) { return clip ? (p < 0.f ? 0.f : (p > 1.f ? 1.f : p)) : p; }

struct MtStat { double sse; float gmn, gmx, pmn, pmx; };

__device__ __forceinline__ void mt_add(MtStat& s, float p, float g, int clip) {
    p = mt_clip(p, clip);
    const float e = p - g;
    s.sse += (double)e * (double)e;
    s.gmn = mt_nanmin(s.gmn, g); s.gmx = mt_nanmax(s.gmx, g);
    s.pmn = mt_nanmin(s.pmn, p); s.pmx = mt_nanmax(s.pmx, p);
}

__device__ __forceinline__ void mt_merge(MtStat& a, const MtStat& b) {
    a.sse += b.sse;
    a.gmn = mt_nanmin(a.gmn, b.gmn); a.gmx = mt_nanmax(a.gmx, b.gmx);
    a.pmn = mt_nanmin(a.pmn, b.pmn); a.pmx = mt_nanmax(a.pmx, b.pmx);
}

__device__ __forceinline__ MtStat mt_shfl_xor(const MtStat& s, int o) {
    MtStat r;
    r.sse = __shfl_xor(s.sse, o, 64);
    r.gmn = __shfl_xor(s.gmn, o, 64); r.gmx = __shfl_xor(s.gmx, o, 64);
    r.pmn = __shfl_xor(s.pmn, o, 64); r.pmx = __shfl_xor(s.pmx, o, 64);
    return r;
}

// 16-byte loads need pred and gt at the same offset from a 16-byte boundary; head / tail scalars around the float4 body
__device__ __forceinline__ void mt_split(const float* p, const float* g, int64_t len, int64_t& head, int64_t& nv) {
    if ((((uintptr_t)p ^ (uintptr_t)g) & 15) != 0) { head = len; nv = 0; return; }
    head = (int64_t)(((16 - ((uintptr_t)p & 15)) & 15) >> 2);
    if (head > len) head = len;
    nv = (len - head) >> 2;
}

__global__ __launch_bounds__(MT_STATS_THREADS) void mt_stats_kernel(MtDims d, const float* __restrict__ pred,
                                                                    const float* __restrict__ gt, int clip, MtWs ws) {
    __shared__ MtStat red[MT_STATS_THREADS / 64];
    const int t = threadIdx.x, b = blockIdx.x;
    const int64_t stride = (int64_t)d.sb * MT_STATS_THREADS;
    for (int64_t n = blockIdx.y; n < d.n; n += gridDim.y) {
        const float* P = pred + n * d.m;
        const float* G = gt + n * d.m;
        int64_t head, nv;
        mt_split(P, G, d.m, head, nv);
        const int64_t tail0 = head + 4 * nv;
        MtStat s{0.0, INFINITY, -INFINITY, INFINITY, -INFINITY};
        const int64_t i0 = (int64_t)b * MT_STATS_THREADS + t;
        for (int64_t k = i0; k < nv; k += stride) {
            const float4 p4 = *reinterpret_cast<const float4*>(P + head + 4 * k);
            const float4 g4 = *reinterpret_cast<const float4*>(G + head + 4 * k);
            mt_add(s, p4.x, g4.x, clip); mt_add(s, p4.y, g4.y, clip);
            mt_add(s, p4.z, g4.z, clip); mt_add(s, p4.w, g4.w, clip);
        }
        for (int64_t i = i0; i < head; i += stride) mt_add(s, P[i], G[i], clip);
        for (int64_t i = tail0 + i0; i < d.m; i += stride) mt_add(s, P[i], G[i], clip);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mt_merge(s, mt_shfl_xor(s, o));
        if ((t & 63) == 0) red[t >> 6] = s;
        __syncthreads();
        if (t == 0) {
            MtStat a = red[0];
            for (int q = 1; q < MT_STATS_THREADS / 64; ++q) mt_merge(a, red[q]);
            const int64_t slot = n * d.sb + b;
            ws.sse[slot] = a.sse;
            ws.mm[4 * slot + 0] = a.gmn; ws.mm[4 * slot + 1] = a.gmx;
            ws.mm[4 * slot + 2] = a.pmn; ws.mm[4 * slot + 3] = a.pmx;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void mt_stats_finish_kernel(MtDims d, MtWs ws, int range_mode, double fixed_range,
                                                              double* mse, double* psnr, double* range) {
    __shared__ float rmn[4], rmx[4];
    const int t = threadIdx.x;
    float pmn = INFINITY, pmx = -INFINITY;                   // pred over the whole batch (SWNERF_RANGE_PRED_RULE)
    for (int64_t n = t; n < d.n; n += 256) {
        for (int b = 0; b < d.sb; ++b) {
            pmn = mt_nanmin(pmn, ws.mm[4 * (n * d.sb + b) + 2]);
            pmx = mt_nanmax(pmx, ws.mm[4 * (n * d.sb + b) + 3]);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        pmn = mt_nanmin(pmn, __shfl_xor(pmn, o, 64));
        pmx = mt_nanmax(pmx, __shfl_xor(pmx, o, 64));
    }
    if ((t & 63) == 0) { rmn[t >> 6] = pmn; rmx[t >> 6] = pmx; }
    __syncthreads();
    pmn = rmn[0]; pmx = rmx[0];
    for (int q = 1; q < 4; ++q) { pmn = mt_nanmin(pmn, rmn[q]); pmx = mt_nanmax(pmx, rmx[q]); }
    // metrics.ipynb SSIM: max_val = 255 if max(pred) > 128 else 1, min_val = -1 if min(pred) < -0.5 else 0 (NaN: 1, 0)
    const double rule = (pmx > 128.f ? 255.0 : 1.0) - (pmn < -0.5f ? -1.0 : 0.0);
    for (int64_t n = t; n < d.n; n += 256) {
        double sse = 0.0;
        float gmn = INFINITY, gmx = -INFINITY;
        for (int b = 0; b < d.sb; ++b) {
            const int64_t slot = n * d.sb + b;
            sse += ws.sse[slot];
            gmn = mt_nanmin(gmn, ws.mm[4 * slot]);
            gmx = mt_nanmax(gmx, ws.mm[4 * slot + 1]);
        }
        // gt.max() - gt.min() is a float32 subtraction in the reference (nerf/run.py:56)
        const double R = range_mode == SWNERF_RANGE_FIXED ? fixed_range : (range_mode == SWNERF_RANGE_GT ? (double)(gmx - gmn) : rule);
        const double e = sse / (double)d.m;
        mse[n] = e;
        range[n] = R;
        psnr[n] = 10.0 * log10((R * R) / e);
        ws.cc[2 * n] = (0.01 * R) * (0.01 * R);
        ws.cc[2 * n + 1] = (0.03 * R) * (0.03 * R);
    }
}

template <int WIN, int GAUSS>
__global__ __launch_bounds__(MT_SSIM_THREADS) void mt_ssim_kernel(MtDims d, const float* __restrict__ pred,
                                                                  const float* __restrict__ gt, int clip, MtWs ws,
                                                                  MtWeights wt, float* __restrict__ map) {
    constexpr int IW = MT_TW + WIN - 1, IH = MT_TH + WIN - 1, LD = IW * 3;
    __shared__ float sx[IH * LD];
    __shared__ float sy[IH * LD];
    __shared__ double red[MT_SSIM_THREADS / 64];
    const int t = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int64_t ty = tile / d.tx, tx = tile - ty * d.tx;
    const int64_t y0 = ty * MT_TH, x0 = tx * MT_TW;
    const int rows = (int)(d.h - y0 < IH ? d.h - y0 : IH);   // input rows / columns of this tile that exist
    const int cols = (int)(d.w - x0 < IW ? d.w - x0 : IW);
    const int len = cols * 3;
    const int c = t / 3, ch = t - 3 * (t / 3);
    const bool active = x0 + c < d.wo;                       // its window then ends inside `cols`
    constexpr double inv = GAUSS ? 1.0 : 1.0 / (double)(WIN * WIN);
    constexpr double cov_norm = GAUSS ? 1.0 : (double)(WIN * WIN) / (double)(WIN * WIN - 1);
    for (int64_t n = blockIdx.y; n < d.n; n += gridDim.y) {
        const float* P = pred + n * d.m;
        const float* G = gt + n * d.m;
        // stage rows y0 .. y0+rows-1, columns x0 .. x0+cols-1 of both images; per row: item 0 = the scalar head, items
        // 1..nv = float4s, item nv+1 = the scalar tail (a row has at most len/4 float4s, so kmax items cover every row)
        const int kmax = (len >> 2) + 2;
        for (int idx = t; idx < rows * kmax; idx += MT_SSIM_THREADS) {
            const int r = idx / kmax, k = idx - r * kmax;
            const int64_t off = ((y0 + r) * d.w + x0) * 3;
            const float* pr = P + off;
            const float* gr = G + off;
            float* lx = sx + r * LD;
            float* ly = sy + r * LD;
            int64_t head, nv;
            mt_split(pr, gr, len, head, nv);
            if (k == 0) {
                for (int j = 0; j < head; ++j) { lx[j] = mt_clip(pr[j], clip); ly[j] = gr[j]; }
            } else if (k <= nv) {
                const int j = (int)head + 4 * (k - 1);
                const float4 p4 = *reinterpret_cast<const float4*>(pr + j);
                const float4 g4 = *reinterpret_cast<const float4*>(gr + j);
                lx[j] = mt_clip(p4.x, clip); lx[j + 1] = mt_clip(p4.y, clip); lx[j + 2] = mt_clip(p4.z, clip); lx[j + 3] = mt_clip(p4.w, clip);
                ly[j] = g4.x; ly[j + 1] = g4.y; ly[j + 2] = g4.z; ly[j + 3] = g4.w;
            } else if (k == nv + 1) {
                for (int j = (int)(head + 4 * nv); j < len; ++j) { lx[j] = mt_clip(pr[j], clip); ly[j] = gr[j]; }
            }
        }
        __syncthreads();
        double sum = 0.0;
        if (active) {
            const double C1 = ws.cc[2 * n], C2 = ws.cc[2 * n + 1];
            double acc[WIN][5];                              // acc[k]: output row r - (WIN-1) + k
#pragma unroll
            for (int k = 0; k < WIN; ++k)
#pragma unroll
                for (int q = 0; q < 5; ++q) acc[k][q] = 0.0;
            for (int r = 0; r < rows; ++r) {
                const float* rx = sx + r * LD + 3 * c + ch;
                const float* ry = sy + r * LD + 3 * c + ch;
                double h[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int j = 0; j < WIN; ++j) {
                    const double xv = (double)rx[3 * j], yv = (double)ry[3 * j];
                    if (GAUSS) {
                        const double g = wt.g[j];
                        h[0] += g * xv; h[1] += g * yv; h[2] += g * (xv * xv); h[3] += g * (yv * yv); h[4] += g * (xv * yv);
                    } else {
                        h[0] += xv; h[1] += yv; h[2] += xv * xv; h[3] += yv * yv; h[4] += xv * yv;
                    }
                }
#pragma unroll
                for (int k = 0; k < WIN; ++k)
#pragma unroll
                    for (int q = 0; q < 5; ++q) acc[k][q] += GAUSS ? wt.g[WIN - 1 - k] * h[q] : h[q];
                if (r >= WIN - 1) {
                    const double ux = acc[0][0] * inv, uy = acc[0][1] * inv;
                    const double vx = cov_norm * (acc[0][2] * inv - ux * ux);
                    const double vy = cov_norm * (acc[0][3] * inv - uy * uy);
                    const double vxy = cov_norm * (acc[0][4] * inv - ux * uy);
                    const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2;
                    const double B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
                    const double S = (A1 * A2) / (B1 * B2);
                    sum += S;
                    if (map) map[((n * d.ho + y0 + (r - (WIN - 1))) * d.wo + x0 + c) * 3 + ch] = (float)S;
                }
#pragma unroll
                for (int k = 0; k < WIN - 1; ++k)
#pragma unroll
                    for (int q = 0; q < 5; ++q) acc[k][q] = acc[k + 1][q];
#pragma unroll
                for (int q = 0; q < 5; ++q) acc[WIN - 1][q] = 0.0;
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if ((t & 63) == 0) red[t >> 6] = sum;
        __syncthreads();
        if (t == 0) ws.part[n * d.tiles + tile] = red[0] + red[1] + red[2];
        __syncthreads();                                     // LDS is restaged for the next image
    }
}

__global__ __launch_bounds__(256) void mt_ssim_finish_kernel(MtDims d, MtWs ws, double* ssim) {
    const double cnt = 3.0 * (double)d.ho * (double)d.wo;
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < d.n; n += (int64_t)gridDim.x * 256) {
        double s = 0.0;
        for (int64_t k = 0; k < d.tiles; ++k) s += ws.part[n * d.tiles + k];
        ssim[n] = s / cnt;
    }
}

static int mt_check(int64_t n, int64_t h, int64_t w, int mode) {
    if (mode != SWNERF_SSIM_SKIMAGE && mode != SWNERF_SSIM_GAUSS11)
        return sw_fail(SWNERF_E_ARG, "image_metrics: unknown SSIM mode %d", mode);
    const int win = mode == SWNERF_SSIM_GAUSS11 ? 11 : 7;
    if (n < 0) return sw_fail(SWNERF_E_ARG, "image_metrics: negative image count %lld", (long long)n);
    if (h < win || w < win)
        return sw_fail(SWNERF_E_ARG, "image_metrics: a %lld x %lld image is smaller than the %d x %d SSIM window",
                       (long long)h, (long long)w, win, win);
    if (h > (1 << 20) || w > (1 << 20)) return sw_fail(SWNERF_E_ARG, "image_metrics: image side above 2^20");
    return 0;
}

extern "C" size_t swnerf_metrics_workspace_bytes(int64_t n, int64_t h, int64_t w, int mode) {
    const int win = mode == SWNERF_SSIM_GAUSS11 ? 11 : 7;
    if (n <= 0 || h < win || w < win || (mode != SWNERF_SSIM_SKIMAGE && mode != SWNERF_SSIM_GAUSS11)) return 0;
    const MtDims d = mt_dims(n, h, w, mode);
    return (size_t)(mt_round256(8 * n * d.sb) + mt_round256(16 * n * d.sb) + mt_round256(16 * n) + mt_round256(8 * n * d.tiles));
}

extern "C" int swnerf_image_metrics(const float* pred, const float* gt, int64_t n, int64_t h, int64_t w, int mode,
                                    int range_mode, double fixed_range, int clip_pred, void* workspace, double* mse,
                                    double* psnr, double* range, double* ssim, float* ssim_map, void* stream) {
    int rc = mt_check(n, h, w, mode);
    if (rc) return rc;
    if (range_mode != SWNERF_RANGE_FIXED && range_mode != SWNERF_RANGE_GT && range_mode != SWNERF_RANGE_PRED_RULE)
        return sw_fail(SWNERF_E_ARG, "image_metrics: unknown data-range source %d", range_mode);
    if (n == 0) return 0;
    if (!pred || !gt || !workspace || !mse || !psnr || !range || !ssim) return sw_fail(SWNERF_E_ARG, "image_metrics: NULL pointer");
    if (((uintptr_t)pred & 3) || ((uintptr_t)gt & 3)) return sw_fail(SWNERF_E_ARG, "image_metrics: operands must be 4-byte aligned");
    const MtDims d = mt_dims(n, h, w, mode);
    const MtWs ws = mt_ws(workspace, d);
    MtWeights wt{};
    if (mode == SWNERF_SSIM_GAUSS11) {                      // metrics.ipynb SSIM.gaussian(11, 1.5): normalised 1-D weights
        double s = 0.0;
        for (int i = 0; i < 11; ++i) { wt.g[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); s += wt.g[i]; }
        for (int i = 0; i < 11; ++i) wt.g[i] /= s;
    }
    hipStream_t st = (hipStream_t)stream;
    const unsigned gy = (unsigned)(n < MT_MAX_GRID_Y ? n : MT_MAX_GRID_Y);
    hipLaunchKernelGGL(mt_stats_kernel, dim3(d.sb, gy), dim3(MT_STATS_THREADS), 0, st, d, pred, gt, clip_pred ? 1 : 0, ws);
    rc = sw_check(hipGetLastError(), "mt_stats launch");
    if (rc) return rc;
    hipLaunchKernelGGL(mt_stats_finish_kernel, dim3(1), dim3(256), 0, st, d, ws, range_mode, fixed_range, mse, psnr, range);
    rc = sw_check(hipGetLastError(), "mt_stats_finish launch");
    if (rc) return rc;
    if (mode == SWNERF_SSIM_GAUSS11)
        hipLaunchKernelGGL((mt_ssim_kernel<11, 1>), dim3((unsigned)d.tiles, gy), dim3(MT_SSIM_THREADS), 0, st, d, pred, gt,
                           clip_pred ? 1 : 0, ws, wt, ssim_map);
    else
        hipLaunchKernelGGL((mt_ssim_kernel<7, 0>), dim3((unsigned)d.tiles, gy), dim3(MT_SSIM_THREADS), 0, st, d, pred, gt,
                           clip_pred ? 1 : 0, ws, wt, ssim_map);
    rc = sw_check(hipGetLastError(), "mt_ssim launch");
    if (rc) return rc;
    const unsigned fb = (unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(mt_ssim_finish_kernel, dim3(fb), dim3(256), 0, st, d, ws, ssim);
    return sw_check(hipGetLastError(), "mt_ssim_finish launch");
}
