// ray_rows.h - the per-pixel ray arithmetic of get_rays (ray.py:10-38), the NDC warp (ray.py:75-92) and the assembly of one
// ray-batch row [o d near far (t) (viewdirs)] (nerf/run.py:137-158, d_nerf/run_dnerf.py:137-160), written once: the standalone
// kernels of misc_kernels.hip and the training-batch kernel of batch_kernels.hip are the same instructions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct Cam { float fx, fy, cx, cy; float r[9]; float t[3]; };

// intrinsics as get_rays casts them: the focal branch (a Python float) centres at W/2, H/2 evaluated in double
static inline void cam_intrinsics(Cam& c, int H, int W, double fx, double fy, double cx, double cy, int focal_branch) {
    if (focal_branch) { c.fx = (float)fx; c.fy = (float)fx; c.cx = (float)(W * 0.5); c.cy = (float)(H * 0.5); }
    else { c.fx = (float)fx; c.fy = (float)fy; c.cx = (float)cx; c.cy = (float)cy; }
}

// c2w: a [3,4] row-major pose (host or device memory, whichever side calls)
__host__ __device__ __forceinline__ void cam_pose(Cam& c, const float* c2w) {
    for (int i = 0; i < 3; ++i) { for (int k = 0; k < 3; ++k) c.r[i * 3 + k] = c2w[i * 4 + k]; c.t[i] = c2w[i * 4 + 3]; }
}

// direction of the ray through the integer pixel centre (px, py), no +0.5
__device__ __forceinline__ void ray_dir(const Cam& c, float px, float py, float& d0, float& d1, float& d2) {
    const float a = (px - c.cx) / c.fx, b = -(py - c.cy) / c.fy, m = -1.f;
    // sum(dirs[..., None, :] * c2w[:3,:3], -1): products rounded, then added left to right
    d0 = a * c.r[0] + b * c.r[1] + m * c.r[2];
    d1 = a * c.r[3] + b * c.r[4] + m * c.r[5];
    d2 = a * c.r[6] + b * c.r[7] + m * c.r[8];
}

__device__ __forceinline__ void ndc_one(float sx, float sy, float near, float& ox, float& oy, float& oz,
                                        float& dx, float& dy, float& dz) {
    const float t = -(near + oz) / dz;
    ox = ox + t * dx; oy = oy + t * dy; oz = oz + t * dz;
    const float o0 = sx * ox / oz, o1 = sy * oy / oz, o2 = 1.f + 2.f * near / oz;
    const float d0 = sx * (dx / dz - ox / oz), d1 = sy * (dy / dz - oy / oz), d2 = -2.f * near / oz;
    ox = o0; oy = o1; oz = o2; dx = d0; dy = d1; dz = d2;
}

// the python scalars -1./(W/(2.*focal)) are evaluated in double and then cast (ray.py:81-86)
static inline float ndc_scale(int WH, double focal) { return (float)(-1. / (WH / (2. * focal))); }

// one row of `cols` floats: 8 = [o d near far], 11 = ... viewdirs, 12 = ... t viewdirs
__device__ __forceinline__ void pack_row(float* o, int cols, float ox, float oy, float oz, float dx, float dy, float dz,
                                         float near, float far, float ft, int ndc, float sx, float sy) {
    const float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
    const float v0 = dx / nrm, v1 = dy / nrm, v2 = dz / nrm;     // viewdirs BEFORE the NDC warp
    if (ndc) ndc_one(sx, sy, 1.f, ox, oy, oz, dx, dy, dz);       // caller hard-wires near=1. (nerf/run.py:149)
    o[0] = ox; o[1] = oy; o[2] = oz; o[3] = dx; o[4] = dy; o[5] = dz; o[6] = near; o[7] = far;
    if (cols == 8) return;
    int k = 8;
    if (cols == 12) o[k++] = ft;
    o[k] = v0; o[k + 1] = v1; o[k + 2] = v2;
}

// |rays_d| of a row as the compositing scales its dists by it (ray.py:173) - and NaN when any of the row's o, d, near, far or frame
// time (0.f where the row has none) is not finite.  One test per ray: every dist of such a ray is then NaN, and through it every
// weight and every map, as the reference has them; the per-sample code of the passes stays as it is (the hidden ReLU of the
// per-row MLP is maxNum, so `raw` of such a row would come back finite, from the biases).  A finite row keeps its bits.
__device__ __forceinline__ float row_dnorm(float ox, float oy, float oz, float dx, float dy, float dz, float near, float far, float ft) {
    const bool finite = __builtin_isfinite(ox) && __builtin_isfinite(oy) && __builtin_isfinite(oz) && __builtin_isfinite(dx) &&
                        __builtin_isfinite(dy) && __builtin_isfinite(dz) && __builtin_isfinite(near) && __builtin_isfinite(far) &&
                        __builtin_isfinite(ft);
    return finite ? sqrtf(dx * dx + dy * dy + dz * dz) : __builtin_nanf("");
}

// One row of the ray batch as the fused passes read it, once per ray: 8 columns [o d near far], 11 = ... viewdirs, 12 = ... t viewdirs.
// VIEWS = false (the net without view directions) leaves v at 0 and reads no column behind `far`.
struct RayRow { float o[3], d[3], near, far, ft, v[3], dnorm; };
template <bool VIEWS>
__device__ __forceinline__ RayRow ray_row_load(const float* rb, int cols) {
    RayRow r;
    r.o[0] = rb[0]; r.o[1] = rb[1]; r.o[2] = rb[2]; r.d[0] = rb[3]; r.d[1] = rb[4]; r.d[2] = rb[5];
    r.near = rb[6]; r.far = rb[7];
    r.ft = (cols == 12) ? rb[8] : 0.f;
    r.v[0] = VIEWS ? rb[cols - 3] : 0.f; r.v[1] = VIEWS ? rb[cols - 2] : 0.f; r.v[2] = VIEWS ? rb[cols - 1] : 0.f;
    r.dnorm = row_dnorm(r.o[0], r.o[1], r.o[2], r.d[0], r.d[1], r.d[2], r.near, r.far, r.ft);
    return r;
}

// A block's 256 rows, assembled in LDS, leave as 16-byte stores of the block's contiguous 256 * cols floats of the batch (a
// row-per-thread store pattern writes `cols` dwords at a 4 * cols-byte stride: every store instruction touches 22 lines for
// 256 useful bytes).  The last, partial block - and an `out` that is not 16-byte aligned - stores dword-wise.  Call after
// __syncthreads().
__device__ __forceinline__ void rows_to_global(const float* rows, float* out, int64_t i0, int64_t n, int cols, int t) {
    float* dst = out + i0 * cols;                                     // 256 * cols * 4 bytes per block: 16-byte aligned when `out` is
    const int live = (int)min((int64_t)256, n - i0) * cols;
    if (live == 256 * cols && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
        for (int q = t; q < 64 * cols; q += 256) reinterpret_cast<float4*>(dst)[q] = reinterpret_cast<const float4*>(rows)[q];
    } else {
        for (int q = t; q < live; q += 256) dst[q] = rows[q];
    }
}
