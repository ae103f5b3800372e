// patch_kernels.hip - the data and the loss of one joint iteration of the MultiRes D-NeRF runner (multires_dnerf.py:909-996) for
// gfx950 (MI355X), two launches.  DESIGN.md 6g "Training".
//   patch_batch    for EVERY level of the pyramid at once: the rays of the level's patch of frame img_i as packed 12-column rows,
//                  the same patch of that level of the pyramid, and the level-0 patch of the full image.  The reference builds the
//                  rays of a whole frame per level and slices the patch out of them.
//   multires_loss  the per-level MSEs (rgb and rgb0), the patches reconstructed through the pyramid, the MSE of the reconstruction
//                  against the full-image patch, their sum, and the gradient of that sum with respect to every rgb / rgb0.
// The levels travel as ONE by-value kernel argument (as the tensor list of optim_kernels.hip): nothing is uploaded per step.
// A patch is clipped to its level, as a slice is: ph = min(patch, H - y), pw = min(patch, W - x).
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/swnerf.h"
#include "host_util.h"
#include "ray_rows.h"
#include "pyramid_interp.h"

#define PB_THREADS 256

// ---- patch_batch ------------------------------------------------------------------------------------------------------
struct PatchLevel {
    const float* pyr; float* rows; float* target;
    int H, W, y, x, ph, pw;
    int block0, pad_;                 // the first block of this level in the grid
    Cam cam;                          // intrinsics only; the pose is read from the table
};

struct PatchDev {
    PatchLevel lv[SWNERF_PATCH_MAX_LEVELS];
    int n_levels, pad_;
    const float* images; float* full_patch;
    const float* c2w; const float* times;
    int64_t img;
    float near, far;
};
static_assert(sizeof(PatchDev) <= 4096 - 256, "the descriptor and the implicit kernel arguments must fit the 4 KB argument block");

__global__ void __launch_bounds__(PB_THREADS) patch_batch_kernel(const PatchDev P) {
    __shared__ __attribute__((aligned(16))) float rows[PB_THREADS * 12];
    const int t = threadIdx.x;
    int l = 0;
    while (l + 1 < P.n_levels && (int)blockIdx.x >= P.lv[l + 1].block0) ++l;
    const PatchLevel& L = P.lv[l];
    const int64_t n = (int64_t)L.ph * L.pw;
    const int64_t i0 = (int64_t)((int)blockIdx.x - L.block0) * PB_THREADS, i = i0 + t;
    if (i < n) {
        const int py = L.y + (int)(i / L.pw), px = L.x + (int)(i % L.pw);
        Cam c = L.cam;
        cam_pose(c, P.c2w + P.img * 12);
        float d0, d1, d2;
        ray_dir(c, (float)px, (float)py, d0, d1, d2);
        pack_row(rows + t * 12, 12, c.t[0], c.t[1], c.t[2], d0, d1, d2, P.near, P.far, P.times[P.img], 0, 0.f, 0.f);
        const int64_t e = ((P.img * L.H + py) * L.W + px) * 3;
        L.target[i * 3] = L.pyr[e]; L.target[i * 3 + 1] = L.pyr[e + 1]; L.target[i * 3 + 2] = L.pyr[e + 2];
        if (l == 0) {                                            // level 0 has the size of the full image
            P.full_patch[i * 3] = P.images[e]; P.full_patch[i * 3 + 1] = P.images[e + 1]; P.full_patch[i * 3 + 2] = P.images[e + 2];
        }
    }
    __syncthreads();
    rows_to_global(rows, L.rows, i0, n, 12, t);
}

static inline int patch_clip(int patch, int side, int corner) { return patch < side - corner ? patch : side - corner; }

extern "C" int swnerf_patch_batch(int n_levels, const float* const* pyr_images, const int* level_hw, const double* focal,
                                  const int* corner, const int* patch, const float* images, int64_t n_images, const float* c2w,
                                  const float* times, int64_t img_i, double near, double far, float* const* ray_batches,
                                  float* const* targets, float* full_patch, void* stream) {
    if (n_levels < 1 || n_levels > SWNERF_PATCH_MAX_LEVELS)
        return sw_fail(SWNERF_E_ARG, "patch_batch: %d levels; 1..%d are built", n_levels, SWNERF_PATCH_MAX_LEVELS);
    if (!pyr_images || !level_hw || !focal || !corner || !patch || !ray_batches || !targets)
        return sw_fail(SWNERF_E_ARG, "patch_batch: NULL host array");
    if (!images || !c2w || !times || !full_patch) return sw_fail(SWNERF_E_ARG, "patch_batch: NULL table (images, c2w or times) or full_patch");
    if (n_images < 1 || img_i < 0 || img_i >= n_images)
        return sw_fail(SWNERF_E_ARG, "patch_batch: frame %lld of %lld", (long long)img_i, (long long)n_images);
    PatchDev P = {};
    int blocks = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int H = level_hw[2 * l], W = level_hw[2 * l + 1], y = corner[2 * l], x = corner[2 * l + 1];
        if (H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20)) return sw_fail(SWNERF_E_ARG, "patch_batch: level %d is %d x %d", l, H, W);
        if (patch[l] < 1 || patch[l] > (1 << 12)) return sw_fail(SWNERF_E_ARG, "patch_batch: level %d patch size %d outside 1..4096", l, patch[l]);
        if (y < 0 || x < 0 || y >= H || x >= W) return sw_fail(SWNERF_E_ARG, "patch_batch: level %d corner (%d, %d) outside its %d x %d image", l, y, x, H, W);
        if (!(focal[l] > 0.)) return sw_fail(SWNERF_E_ARG, "patch_batch: level %d focal %g", l, focal[l]);
        if (!pyr_images[l] || !ray_batches[l] || !targets[l]) return sw_fail(SWNERF_E_ARG, "patch_batch: level %d has a NULL pointer", l);
        PatchLevel& L = P.lv[l];
        L.pyr = pyr_images[l]; L.rows = ray_batches[l]; L.target = targets[l];
        L.H = H; L.W = W; L.y = y; L.x = x; L.ph = patch_clip(patch[l], H, y); L.pw = patch_clip(patch[l], W, x);
        L.block0 = blocks;
        cam_intrinsics(L.cam, H, W, focal[l], focal[l], 0., 0., 1);
        blocks += (L.ph * L.pw + PB_THREADS - 1) / PB_THREADS;
    }
    P.n_levels = n_levels; P.images = images; P.full_patch = full_patch; P.c2w = c2w; P.times = times; P.img = img_i;
    P.near = (float)near; P.far = (float)far;
    hipLaunchKernelGGL(patch_batch_kernel, dim3((unsigned)blocks), dim3(PB_THREADS), 0, (hipStream_t)stream, P);
    return sw_check(hipGetLastError(), "patch_batch launch");
}

// ---- multires_loss ----------------------------------------------------------------------------------------------------
// ONE workgroup of 1024 threads does the levels in sequence (at most 32^2 + 16^2 + 8^2 + 4^2 pixels in the reference):
//   1  per level: the sums of squares of rgb - target and rgb0 - target in fp64 (thread t adds elements t, t + 1024, ...; the 1024
//      partial sums are added in a fixed tree, as in swnerf_photo_loss), and the level's own gradient 2 (x - target) / (3 ph pw),
//      formed in fp64 and rounded once
//   2  the reconstruction r = rgb_{L-1}, r = rgb_l + up(r) for l = L-2 .. 0, ping-ponged between two LDS images; `up` is
//      py_up_pixel, the arithmetic of swnerf_pyramid_up_axpy (equal sizes: the copy that kernel makes)
//   3  the sum of squares of r - full in fp64 and g = 2 (r - full) / (3 ph_0 pw_0)
//   4  with add_global: d_rgb_0 += g, then g = up^T(g) (py_adjoint_pixel, the gather of swnerf_pyramid_up_adjoint) and d_rgb_l += g
//      level by level, again between the two LDS images; fp32 additions, as autograd accumulates them
// No atomics, no dependence on timing: equal bits on every run.
#define ML_THREADS 1024
#define ML_IMG (3 * SWNERF_PATCH_MAX_SIDE * SWNERF_PATCH_MAX_SIDE)

struct LossLevel { const float* rgb; const float* rgb0; const float* target; float* d_rgb; float* d_rgb0; int ph, pw; };

struct LossDev {
    LossLevel lv[SWNERF_PATCH_MAX_LEVELS];
    int n_levels, add_global;
    const float* full; float* losses; float* recon;
};

__device__ __forceinline__ void ml_reduce(double (*red)[ML_THREADS], int t) {
    __syncthreads();
    for (int w = ML_THREADS / 2; w >= 1; w >>= 1) {
        if (t < w) { red[0][t] += red[0][t + w]; red[1][t] += red[1][t + w]; }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(ML_THREADS) multires_loss_kernel(const LossDev P) {
    __shared__ double red[2][ML_THREADS];
    __shared__ float img[2][ML_IMG];
    __shared__ double mean[2 * SWNERF_PATCH_MAX_LEVELS + 1];
    const int t = threadIdx.x;
    const int nl = P.n_levels;
    // 1: the per-level losses and their own gradients
    for (int l = 0; l < nl; ++l) {
        const LossLevel& L = P.lv[l];
        const int n = 3 * L.ph * L.pw;
        const double scale = 2.0 / (double)n;
        double s = 0.0, s0 = 0.0;
        for (int e = t; e < n; e += ML_THREADS) {
            const double tv = (double)L.target[e], d = (double)L.rgb[e] - tv;
            s += d * d;
            L.d_rgb[e] = (float)(d * scale);
            if (L.rgb0) {
                const double d0 = (double)L.rgb0[e] - tv;
                s0 += d0 * d0;
                L.d_rgb0[e] = (float)(d0 * scale);
            }
        }
        red[0][t] = s; red[1][t] = s0;
        ml_reduce(red, t);
        if (t == 0) { mean[2 * l] = red[0][0] / (double)n; mean[2 * l + 1] = red[1][0] / (double)n; }
        __syncthreads();
    }
    // 2: the reconstruction, coarsest level first
    int cur = 0;
    {
        const LossLevel& L = P.lv[nl - 1];
        for (int e = t; e < 3 * L.ph * L.pw; e += ML_THREADS) img[cur][e] = L.rgb[e];
    }
    __syncthreads();
    for (int l = nl - 2; l >= 0; --l) {
        const LossLevel& L = P.lv[l];
        const int h = P.lv[l + 1].ph, w = P.lv[l + 1].pw, H = L.ph, W = L.pw;
        const bool same = h == H && w == W;
        const float sy = (float)h / (float)H, sx = (float)w / (float)W;
        for (int e = t; e < 3 * H * W; e += ML_THREADS) {
            const int y = e / (3 * W), f = e - y * 3 * W, x = f / 3, c = f - x * 3;
            const float u = same ? img[cur][e] : py_up_pixel<3>(img[cur], w, py_axis(y, sy, h), x, c, sx);
            img[cur ^ 1][e] = L.rgb[e] + 1.f * u;
        }
        cur ^= 1;
        __syncthreads();
    }
    // 3: the global loss and its gradient with respect to the reconstruction
    {
        const int n = 3 * P.lv[0].ph * P.lv[0].pw;
        const double scale = 2.0 / (double)n;
        double s = 0.0;
        for (int e = t; e < n; e += ML_THREADS) {
            const float r = img[cur][e];
            const double d = (double)r - (double)P.full[e];
            s += d * d;
            P.recon[e] = r;
            img[cur ^ 1][e] = (float)(d * scale);
        }
        cur ^= 1;                                                 // img[cur] is now g
        red[0][t] = s; red[1][t] = 0.0;
        ml_reduce(red, t);
        if (t == 0) {
            const double g = red[0][0] / (double)n;
            double total = P.add_global ? g : 0.0;
            for (int l = nl - 1; l >= 0; --l) total += mean[2 * l] + (P.lv[l].rgb0 ? mean[2 * l + 1] : 0.0);
            P.losses[0] = (float)total;
            P.losses[1] = (float)g;
            P.losses[2] = (float)(10.0 * log10(1.0 / g));
            for (int l = 0; l < SWNERF_PATCH_MAX_LEVELS; ++l) {
                P.losses[3 + l] = l < nl ? (float)mean[2 * l] : 0.f;
                P.losses[3 + SWNERF_PATCH_MAX_LEVELS + l] = (l < nl && P.lv[l].rgb0) ? (float)mean[2 * l + 1] : 0.f;
            }
        }
    }
    if (!P.add_global) return;
    // 4: the gradient of the global loss goes down the pyramid
    for (int l = 0; l < nl; ++l) {
        const LossLevel& L = P.lv[l];
        const int n = 3 * L.ph * L.pw;
        for (int e = t; e < n; e += ML_THREADS) L.d_rgb[e] = L.d_rgb[e] + img[cur][e];        // e is this thread's own in step 1 too
        if (l + 1 == nl) break;
        const int H = L.ph, W = L.pw, h = P.lv[l + 1].ph, w = P.lv[l + 1].pw;
        const float sy = (float)h / (float)H, sx = (float)w / (float)W;
        for (int e = t; e < 3 * h * w; e += ML_THREADS) {
            const int i = e / (3 * w), f = e - i * 3 * w, j = f / 3, c = f - j * 3;
            img[cur ^ 1][e] = py_adjoint_pixel<3>(img[cur] + c, H, W, h, w, i, j, sy, sx);
        }
        cur ^= 1;
        __syncthreads();
    }
}

extern "C" int swnerf_multires_loss(int n_levels, const int* patch_hw, const float* const* rgb, const float* const* rgb0,
                                    const float* const* targets, const float* full_patch, int add_global, float* losses,
                                    float* reconstructed, float* const* d_rgb, float* const* d_rgb0, void* stream) {
    if (n_levels < 1 || n_levels > SWNERF_PATCH_MAX_LEVELS)
        return sw_fail(SWNERF_E_ARG, "multires_loss: %d levels; 1..%d are built", n_levels, SWNERF_PATCH_MAX_LEVELS);
    if (!patch_hw || !rgb || !targets || !d_rgb) return sw_fail(SWNERF_E_ARG, "multires_loss: NULL host array");
    if (!full_patch || !losses || !reconstructed) return sw_fail(SWNERF_E_ARG, "multires_loss: NULL pointer (full_patch, losses or reconstructed)");
    LossDev P = {};
    for (int l = 0; l < n_levels; ++l) {
        LossLevel& L = P.lv[l];
        L.ph = patch_hw[2 * l]; L.pw = patch_hw[2 * l + 1];
        if (L.ph < 1 || L.pw < 1 || L.ph > SWNERF_PATCH_MAX_SIDE || L.pw > SWNERF_PATCH_MAX_SIDE)
            return sw_fail(SWNERF_E_ARG, "multires_loss: level %d patch %d x %d outside 1..%d", l, L.ph, L.pw, SWNERF_PATCH_MAX_SIDE);
        L.rgb = rgb[l]; L.target = targets[l]; L.d_rgb = d_rgb[l];
        L.rgb0 = rgb0 ? rgb0[l] : nullptr; L.d_rgb0 = (rgb0 && d_rgb0) ? d_rgb0[l] : nullptr;
        if (!L.rgb || !L.target || !L.d_rgb) return sw_fail(SWNERF_E_ARG, "multires_loss: level %d has a NULL pointer", l);
        if (L.rgb0 && !L.d_rgb0) return sw_fail(SWNERF_E_ARG, "multires_loss: level %d has rgb0 without d_rgb0", l);
    }
    P.n_levels = n_levels; P.add_global = add_global ? 1 : 0; P.full = full_patch; P.losses = losses; P.recon = reconstructed;
    hipLaunchKernelGGL(multires_loss_kernel, dim3(1), dim3(ML_THREADS), 0, (hipStream_t)stream, P);
    return sw_check(hipGetLastError(), "multires_loss launch");
}
