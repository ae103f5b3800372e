// batch_kernels.hip - the data side of a training step for gfx950 (MI355X): the ray batch of nerf/run.py:598-681 and
// d_nerf/run_dnerf.py:648-683 drawn, computed, packed and paired with its target pixels in ONE launch, and the photometric
// loss of :689-696 with its gradient in one more.  DESIGN.md 6i.
//
// The reference draws `np.random.choice(H*W, N_rand, replace=False)` on the host (a permutation of every pixel index per step)
// or keeps a shuffled [N*H*W, 3, 3] table of every training ray on the device (use_batching).  Here a batch is the image of
// k0 .. k0+n under a keyed permutation of [0, domain): sampling without replacement with no table and no host work, and a whole
// epoch of use_batching is the permutation walked from 0 to domain.
#include <hip/hip_runtime.h>
#include "../../include/swnerf.h"
#include "host_util.h"
#include "ray_rows.h"

// ---- the keyed permutation --------------------------------------------------------------------------------------------
// A balanced Feistel network on 2 * hb bits (2^(2 hb) >= n, hb as small as that allows, at least 1) with SW_PERM_ROUNDS rounds;
// round function: the 32-bit integer hash below of (half ^ round key), round key r = the high word of mix64(key + (r + 1) * golden).
// A Feistel network is a bijection of [0, 2^(2 hb)) whatever the round function; cycle walking (apply it again while the result
// is >= n) restricts it to a bijection of [0, n).  swnerf/batching.py perm_index_np is the same arithmetic in numpy: the definition.
#define SW_PERM_ROUNDS 6

__host__ __device__ __forceinline__ uint64_t perm_mix64(uint64_t z) {          // the splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__host__ __device__ __forceinline__ uint32_t perm_hash32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__host__ __device__ __forceinline__ int perm_half_bits(int64_t n) {
    int hb = 1;
    while (((int64_t)1 << (2 * hb)) < n) ++hb;
    return hb;
}

struct PermKey { uint32_t rk[SW_PERM_ROUNDS]; int hb; int64_t n; };

static PermKey perm_key(uint64_t key, int64_t n) {
    PermKey P;
    for (int r = 0; r < SW_PERM_ROUNDS; ++r) P.rk[r] = (uint32_t)(perm_mix64(key + (uint64_t)(r + 1) * 0x9E3779B97F4A7C15ull) >> 32);
    P.hb = perm_half_bits(n);
    P.n = n;
    return P;
}

__device__ __forceinline__ int64_t perm_index(const PermKey& P, int64_t k) {
    const uint32_t mask = (1u << P.hb) - 1u;
    const int64_t domain = (int64_t)1 << (2 * P.hb);
    int64_t x = k;
    // the orbit of a point of [0, n) under a bijection of [0, domain) returns to [0, n) before it has visited more than the
    // domain - n points outside it: at most domain - n + 1 applications
    for (int64_t walk = 0; walk < domain - P.n + 1; ++walk) {
        uint32_t l = (uint32_t)(x >> P.hb) & mask, r = (uint32_t)x & mask;
#pragma unroll
        for (int i = 0; i < SW_PERM_ROUNDS; ++i) {
            const uint32_t f = perm_hash32(r ^ P.rk[i]) & mask;
            const uint32_t nl = r;
            r = l ^ f;
            l = nl;
        }
        x = ((int64_t)l << P.hb) | (int64_t)r;
        if (x < P.n) break;
    }
    return x;
}

__global__ void __launch_bounds__(256) perm_indices_kernel(PermKey P, int64_t k0, int64_t count, int64_t* out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) out[i] = perm_index(P, k0 + i);
}

#define SW_PERM_MAX_N ((int64_t)1 << 40)

extern "C" int swnerf_perm_indices(uint64_t key, int64_t n, int64_t k0, int64_t count, int64_t* out, void* stream) {
    if (n < 1 || n >= SW_PERM_MAX_N) return sw_fail(SWNERF_E_ARG, "perm_indices: n %lld outside 1 .. 2^40 - 1", (long long)n);
    if (k0 < 0 || count < 0 || k0 + count > n)
        return sw_fail(SWNERF_E_ARG, "perm_indices: k0 %lld + count %lld must lie in [0, n = %lld]", (long long)k0, (long long)count, (long long)n);
    if (count == 0) return 0;
    if (!out) return sw_fail(SWNERF_E_ARG, "perm_indices: NULL pointer");
    hipLaunchKernelGGL(perm_indices_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, perm_key(key, n), k0, count, out);
    return sw_check(hipGetLastError(), "perm_indices launch");
}

// ---- the training batch -----------------------------------------------------------------------------------------------
struct BatchDev {
    const void* images; int u8, ch; int64_t n_images; int H, W;
    const float* c2w; const float* times; const int64_t* i_train; int64_t n_train;
    int y0, x0, h, w;
    Cam cam;                         // intrinsics only; the pose comes from the table per ray
    float near, far; int cols, ndc; float sx, sy; int white;
    PermKey perm; int64_t k0, n; const int64_t* ids_in;
    float* ray_batch; float* target; int64_t* ids_out;
};

// a pixel channel as the loaders hand it over: bytes / 255. evaluated in double, then float32 (imageio -> np.float32)
__device__ __forceinline__ float px_f32(const BatchDev& P, int64_t e) {
    if (P.u8) return (float)((double)reinterpret_cast<const unsigned char*>(P.images)[e] / 255.);
    return reinterpret_cast<const float*>(P.images)[e];
}

__global__ void __launch_bounds__(256) train_batch_kernel(BatchDev P) {
    __shared__ __attribute__((aligned(16))) float rows[256 * 12];
    const int t = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * 256, i = i0 + t;
    if (i < P.n) {
        const int64_t domain = P.n_train * P.h * P.w;
        const int64_t id = P.ids_in ? P.ids_in[i] : perm_index(P.perm, P.k0 + i);
        const int64_t hw = (int64_t)P.h * P.w;
        const int64_t slot = id / hw, rem = id - slot * hw;
        const int64_t img = (id >= 0 && id < domain) ? P.i_train[slot] : -1;
        float* o = rows + t * P.cols;
        float tg[3];
        if (img < 0 || img >= P.n_images) {
            // an id outside the window or a training index outside the image table (a caller's error the host cannot see
            // without reading device memory): the row and its target are NaN, nothing is read
            const float nan = __builtin_nanf("");
            for (int c = 0; c < P.cols; ++c) o[c] = nan;
            tg[0] = tg[1] = tg[2] = nan;
        } else {
            const int y = P.y0 + (int)(rem / P.w), x = P.x0 + (int)(rem % P.w);
            Cam c = P.cam;
            cam_pose(c, P.c2w + img * 12);
            float d0, d1, d2;
            ray_dir(c, (float)x, (float)y, d0, d1, d2);
            pack_row(o, P.cols, c.t[0], c.t[1], c.t[2], d0, d1, d2, P.near, P.far, P.cols == 12 ? P.times[img] : 0.f, P.ndc, P.sx, P.sy);
            const int64_t e = ((img * P.H + y) * P.W + x) * P.ch;
            tg[0] = px_f32(P, e); tg[1] = px_f32(P, e + 1); tg[2] = px_f32(P, e + 2);
            if (P.ch == 4 && P.white) {
                // images[..., :3] * images[..., -1:] + (1. - images[..., -1:]) (nerf/run.py:469-472): three roundings per channel
                const float a = px_f32(P, e + 3), na = 1.f - a;
                tg[0] = tg[0] * a + na; tg[1] = tg[1] * a + na; tg[2] = tg[2] * a + na;
            }
        }
        P.target[i * 3] = tg[0]; P.target[i * 3 + 1] = tg[1]; P.target[i * 3 + 2] = tg[2];
        if (P.ids_out) P.ids_out[i] = id;
    }
    __syncthreads();
    rows_to_global(rows, P.ray_batch, i0, P.n, P.cols, t);
}

extern "C" int swnerf_train_batch(const void* images, int images_u8, int channels, int64_t n_images, int H, int W,
                                  const float* c2w, const float* times, const int64_t* i_train, int64_t n_train,
                                  int y0, int x0, int h, int w, double fx, double fy, double cx, double cy, int focal_branch,
                                  double near, double far, int cols, int ndc, double ndc_focal, int white_bkgd,
                                  uint64_t key, int64_t k0, int64_t n, const int64_t* ids_in,
                                  float* ray_batch, float* target, int64_t* ids_out, void* stream) {
    if (cols != 8 && cols != 11 && cols != 12) return sw_fail(SWNERF_E_ARG, "train_batch: rows of %d columns (8, 11 or 12)", cols);
    if (channels != 3 && channels != 4) return sw_fail(SWNERF_E_ARG, "train_batch: images of %d channels (3 or 4)", channels);
    if (n_images < 1 || n_train < 1 || H < 1 || W < 1)
        return sw_fail(SWNERF_E_ARG, "train_batch: empty image table (n_images=%lld n_train=%lld H=%d W=%d)", (long long)n_images, (long long)n_train, H, W);
    if (h < 1 || w < 1 || y0 < 0 || x0 < 0 || (int64_t)y0 + h > H || (int64_t)x0 + w > W)
        return sw_fail(SWNERF_E_ARG, "train_batch: empty window or window outside the image (y0=%d x0=%d h=%d w=%d of %d x %d)", y0, x0, h, w, H, W);
    const int64_t hw = (int64_t)h * w;
    if (n_train >= SW_PERM_MAX_N / hw) return sw_fail(SWNERF_E_ARG, "train_batch: n_train * h * w must stay below 2^40");
    const int64_t domain = n_train * hw;
    if (n < 0 || k0 < 0) return sw_fail(SWNERF_E_ARG, "train_batch: negative n or k0");
    if (!ids_in && k0 + n > domain)
        return sw_fail(SWNERF_E_ARG, "train_batch: k0 %lld + n %lld exceeds the domain n_train * h * w = %lld", (long long)k0, (long long)n, (long long)domain);
    if (!images || !c2w || !i_train) return sw_fail(SWNERF_E_ARG, "train_batch: NULL table (images, c2w or i_train)");
    if (cols == 12 && !times) return sw_fail(SWNERF_E_ARG, "train_batch: rows of 12 columns need the frame-time table (times is NULL)");
    if (n == 0) return 0;
    if (!ray_batch || !target) return sw_fail(SWNERF_E_ARG, "train_batch: NULL output pointer");
    BatchDev P = {};
    P.images = images; P.u8 = images_u8 ? 1 : 0; P.ch = channels; P.n_images = n_images; P.H = H; P.W = W;
    P.c2w = c2w; P.times = times; P.i_train = i_train; P.n_train = n_train;
    P.y0 = y0; P.x0 = x0; P.h = h; P.w = w;
    cam_intrinsics(P.cam, H, W, fx, fy, cx, cy, focal_branch);
    P.near = (float)near; P.far = (float)far; P.cols = cols; P.ndc = ndc ? 1 : 0;
    P.sx = ndc ? ndc_scale(W, ndc_focal) : 0.f; P.sy = ndc ? ndc_scale(H, ndc_focal) : 0.f; P.white = white_bkgd ? 1 : 0;
    P.perm = perm_key(key, domain); P.k0 = k0; P.n = n; P.ids_in = ids_in;
    P.ray_batch = ray_batch; P.target = target; P.ids_out = ids_out;
    hipLaunchKernelGGL(train_batch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P);
    return sw_check(hipGetLastError(), "train_batch launch");
}

// ---- the photometric loss (nerf/run.py:689-696: img2mse(rgb, target) + img2mse(rgb0, target)) ---------------------------
// ONE workgroup, as swnerf_fit2d_loss: thread t adds the squares of elements t, t + 1024, ... in fp64, the 1024 partial sums are
// added in a fixed tree - equal bits on every run.  sums = the two sums of squares; losses = [mean + mean0, mean, mean0], each
// formed in fp64 and rounded once; d_rgb / d_rgb0 = 2 (x - target) / (3 N), formed in fp64 and rounded once.
__global__ void __launch_bounds__(1024) photo_loss_kernel(const float* rgb, const float* rgb0, const float* tgt, int64_t N, double* sums,
                                                          float* losses, float* d_rgb, float* d_rgb0) {
    __shared__ double red[2][1024];
    const int t = threadIdx.x;
    const int64_t n = 3 * N;
    const double scale = 2.0 / (double)n;
    double s = 0.0, s0 = 0.0;
    for (int64_t e = t; e < n; e += 1024) {
        const double tv = (double)tgt[e], d = (double)rgb[e] - tv;
        s += d * d;
        if (d_rgb) d_rgb[e] = (float)(d * scale);
        if (rgb0) {
            const double d0 = (double)rgb0[e] - tv;
            s0 += d0 * d0;
            if (d_rgb0) d_rgb0[e] = (float)(d0 * scale);
        }
    }
    red[0][t] = s; red[1][t] = s0;
    __syncthreads();
    for (int w = 512; w >= 1; w >>= 1) {
        if (t < w) { red[0][t] += red[0][t + w]; red[1][t] += red[1][t + w]; }
        __syncthreads();
    }
    if (t == 0) {
        sums[0] = red[0][0]; sums[1] = red[1][0];
        if (losses) {
            const double m = red[0][0] / (double)n, m0 = red[1][0] / (double)n;
            losses[0] = (float)(m + m0); losses[1] = (float)m; losses[2] = (float)m0;
        }
    }
}

extern "C" int swnerf_photo_loss(const float* rgb, const float* rgb0, const float* target, int64_t N, double* sums, float* losses,
                                 float* d_rgb, float* d_rgb0, void* stream) {
    if (N < 1 || N > ((int64_t)1 << 32)) return sw_fail(SWNERF_E_ARG, "photo_loss: N %lld outside 1 .. 2^32", (long long)N);
    if (!rgb || !target || !sums) return sw_fail(SWNERF_E_ARG, "photo_loss: NULL pointer");
    if (d_rgb0 && !rgb0) return sw_fail(SWNERF_E_ARG, "photo_loss: d_rgb0 without rgb0");
    hipLaunchKernelGGL(photo_loss_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, rgb, rgb0, target, N, sums, losses, d_rgb, d_rgb0);
    return sw_check(hipGetLastError(), "photo_loss launch");
}
