// meshrender_kernels.hip - a triangle mesh that is on the device, seen from the project's own cameras: a 64-bit z-buffer filled by
// integer atomicMin, a resolve pass that turns it into colour, depth, disparity, coverage, face id and barycentrics, and the
// comparison of such a render with a reference silhouette and depth map.  The arithmetic is in meshrender_math.h (DESIGN.md 6b "Mesh
// rendering"; tests/meshrender_ref.py replays it); the ray of a pixel is get_rays' (ray_dir of ray_rows.h).
//   raster   memset the z-buffer to all ones | one thread per (view, face) pair, pair = view F + face, grid-stride in whole waves:
//            the pair's pixel box (meshrender_box); a lane whose box holds at most 64 pixels walks it itself; the lanes of the wave
//            with a larger box (__ballot) are taken one at a time by the whole wave, the face broadcast by shuffles, the box spread
//            over the 64 lanes.  A hit is one atomicMin of (depth bits << 32 | face id).  No list, no counter, no second launch.
//            Few pairs are spread over the grid, up to one pair a wave, so that a handful of large faces use the whole chip.
//   resolve  one thread per pixel, grid-stride: decode the face, recompute the hit with the same function, write the outputs
//   compare  one workgroup of 1024 per view: lane sums over pixels l, l + 1024, .., folded in halves (meshrender_math.h)
// Every pixel index is bounded by its box, which meshrender_box clamps to the image; every face index is checked before it is followed.
#include "meshops_common.h"
#include "meshrender_math.h"
#include "ray_rows.h"

#define MR_THREADS 256

static inline bool mr_sizes_ok(int64_t N, int64_t H, int64_t W) {
    if (N < 0 || H < 1 || W < 1 || H > INT32_MAX || W > INT32_MAX) return false;
    const int64_t hw = H * W;                                      // < 2^62
    return hw <= INT32_MAX && (N == 0 || hw <= INT32_MAX / N);
}

extern "C" int64_t swnerf_mesh_render_workspace_bytes(int64_t N, int64_t H, int64_t W) {
    if (!mr_sizes_ok(N, H, W)) return 0;
    return (8 * N * H * W + 255) / 256 * 256 + 256;
}

struct MrScene {
    const float* verts;
    const int32_t* faces;
    const float* c2w;
    int64_t V, F, N;
    int H, W;
    float fx, fy, cx, cy;
};

static inline int mr_scene(const char* what, MrScene& s, const float* verts, const int32_t* faces, int64_t V, int64_t F, const float* c2w, int64_t N, int H,
                           int W, double fx, double fy, double cx, double cy, int focal_branch) {
    int rc = mo_check(what, V, F);
    if (rc) return rc;
    if (!mr_sizes_ok(N, H, W))
        return sw_fail(SWNERF_E_ARG, "%s: N = %lld views of %d x %d: need N >= 0, H, W >= 1 and N H W < 2^31", what, (long long)N, H, W);
    if ((V > 0 && !verts) || (F > 0 && !faces) || (N > 0 && !c2w)) return sw_fail(SWNERF_E_ARG, "%s: NULL verts / faces / c2w", what);
    Cam c;
    cam_intrinsics(c, H, W, fx, fy, cx, cy, focal_branch);
    s = MrScene{verts, faces, c2w, V, F, N, H, W, c.fx, c.fy, c.cx, c.cy};
    return 0;
}

__device__ __forceinline__ Cam mr_cam(const MrScene& s, int64_t n) {
    Cam c;
    c.fx = s.fx; c.fy = s.fy; c.cx = s.cx; c.cy = s.cy;
    cam_pose(c, s.c2w + 12 * n);
    return c;
}

__device__ __forceinline__ void mr_load_face(const MrScene& s, int64_t f, float v[9]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t i = s.faces[3 * f + k];                      // in 0..V-1: meshrender_face_ok passed
#pragma unroll
        for (int q = 0; q < 3; ++q) v[3 * k + q] = s.verts[3 * i + q];
    }
}

// spread = log2 of the threads a pair gets: pair p sits on thread p << spread and the threads between stay idle in the narrow tier
struct MrWindow { float near, far; int cull, spread; };

// pixel (px, py) of view n, inside the image, against one face
__device__ __forceinline__ void mr_test(const MrScene& s, const MrWindow& w, const Cam& cam, const float v[9], uint32_t f, int64_t n, int px, int py,
                                        unsigned long long* __restrict__ z, unsigned long long& hits) {
    float d[3];
    ray_dir(cam, (float)px, (float)py, d[0], d[1], d[2]);
    MeshrenderHit h;
    if (meshrender_hit(v, v + 3, v + 6, cam.t, d, w.near, w.far, w.cull, h)) {
        atomicMin(z + ((n * s.H + py) * (int64_t)s.W + px), (unsigned long long)meshrender_key(h.tf, f));
        ++hits;
    }
}

__global__ __launch_bounds__(MR_THREADS) void mr_raster_kernel(MrScene s, MrWindow w, unsigned long long* __restrict__ z, int64_t* counts) {
    const int lane = threadIdx.x & 63;
    const int64_t P = s.N * s.F, T = P << w.spread, stride = (int64_t)gridDim.x * MR_THREADS;
    unsigned long long nbad = 0, nbehind = 0, nwide = 0, nhits = 0;
    // the loop bound is the same for the 64 lanes of a wave: all of them reach the ballot and the shuffles
    for (int64_t base = (int64_t)blockIdx.x * MR_THREADS + (threadIdx.x & ~63); base < T; base += stride) {
        const int64_t g = base + lane, p = (g & (((int64_t)1 << w.spread) - 1)) ? P : g >> w.spread;
        float v[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        int box[4] = {0, -1, 0, -1};
        int n = 0, f = 0;
        bool narrow = false, wide = false;
        if (p < P) {
            n = (int)(p / s.F);
            f = (int)(p - (int64_t)n * s.F);
            if (!meshrender_face_ok(s.verts, s.faces, f, s.V)) {
                nbad += n == 0;                                    // once per face
            } else {
                mr_load_face(s, f, v);
                const Cam cam = mr_cam(s, n);
                const bool boxes = meshrender_view_boxes(cam.r, cam.fx, cam.fy, s.H, s.W);
                if (meshrender_box(v, v + 3, v + 6, cam.t, cam.r, cam.fx, cam.fy, cam.cx, cam.cy, s.H, s.W, boxes, box) == MESHRENDER_BOX_SKIP) {
                    ++nbehind;
                } else {
                    const int64_t area = meshrender_box_pixels(box);
                    wide = area > MESHRENDER_NARROW_PIXELS;
                    narrow = area > 0 && !wide;
                    nwide += wide;
                }
            }
        }
        if (narrow) {
            const Cam cam = mr_cam(s, n);
            for (int py = box[2]; py <= box[3]; ++py)
                for (int px = box[0]; px <= box[1]; ++px) mr_test(s, w, cam, v, (uint32_t)f, n, px, py, z, nhits);
        }
        unsigned long long todo = __ballot(wide);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            float bv[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) bv[k] = __shfl(v[k], src, 64);
            const int x0 = __shfl(box[0], src, 64), x1 = __shfl(box[1], src, 64), y0 = __shfl(box[2], src, 64), y1 = __shfl(box[3], src, 64);
            const int bn = __shfl(n, src, 64), bf = __shfl(f, src, 64);
            const Cam cam = mr_cam(s, bn);
            const int64_t bw = x1 - x0 + 1, area = bw * (int64_t)(y1 - y0 + 1);
            for (int64_t q = lane; q < area; q += 64) {
                const int64_t row = q / bw;
                mr_test(s, w, cam, bv, (uint32_t)bf, bn, x0 + (int)(q - row * bw), y0 + (int)row, z, nhits);
            }
        }
    }
    unsigned long long* c = (unsigned long long*)counts;          // non-negative totals: the same words as int64
    wave_count(c, nbad);
    wave_count(c + 1, nbehind);
    wave_count(c + 2, nwide);
    wave_count(c + 3, nhits);
}

extern "C" int swnerf_mesh_render_raster(const float* verts, const int32_t* faces, int64_t V, int64_t F, const float* c2w, int64_t N, int H, int W,
                                         double fx, double fy, double cx, double cy, int focal_branch, float near, float far, int cull,
                                         void* workspace, int64_t* counts, void* stream) {
    MrScene s;
    int rc = mr_scene("mesh_render_raster", s, verts, faces, V, F, c2w, N, H, W, fx, fy, cx, cy, focal_branch);
    if (rc) return rc;
    if (!(near >= 0.f) || !(far > near)) return sw_fail(SWNERF_E_ARG, "mesh_render_raster: need 0 <= near < far, got near = %g, far = %g", (double)near, (double)far);
    if (cull < MESHRENDER_CULL_NONE || cull > MESHRENDER_CULL_FRONT) return sw_fail(SWNERF_E_ARG, "mesh_render_raster: unknown cull mode %d", cull);
    if (!counts) return sw_fail(SWNERF_E_ARG, "mesh_render_raster: NULL counts");
    hipStream_t st = (hipStream_t)stream;
    rc = sw_check(hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), st), "mesh_render_raster memset");
    const int64_t pixels = N * H * W;
    if (rc || pixels == 0) return rc;
    if (!workspace) return sw_fail(SWNERF_E_ARG, "mesh_render_raster: NULL workspace");
    rc = sw_check(hipMemsetAsync(workspace, 0xFF, 8 * pixels, st), "mesh_render_raster memset");
    if (rc || F == 0) return rc;
    // Few pairs - a decimated mesh, a handful of large faces - are spread over more waves, up to one pair a wave, as long as the grid
    // stays within one grid-stride round: the wave tier works on one wide pair at a time, and 1000 image-sized triangles on
    // consecutive lanes would keep 16 waves busy.  Which thread holds a pair changes no result.
    int spread = 0;
    while (spread < 6 && ((N * F) << (spread + 1)) <= (int64_t)MO_MAX_GRID * MR_THREADS) ++spread;
    hipLaunchKernelGGL(mr_raster_kernel, dim3(mo_blocks((N * F) << spread)), dim3(MR_THREADS), 0, st, s, MrWindow{near, far, cull, spread},
                       (unsigned long long*)workspace, counts);
    return sw_check(hipGetLastError(), "mesh_render_raster launch");
}

struct MrOut {
    const float *normals, *colors;
    float *rgb, *depth, *disp, *acc, *bary;
    int32_t* face;
    float bg[3];
    int shading;
};

__global__ __launch_bounds__(MR_THREADS) void mr_resolve_kernel(MrScene s, MrOut o, const unsigned long long* __restrict__ z) {
    const int64_t pixels = s.N * s.H * s.W, hw = (int64_t)s.H * s.W;
    for (int64_t i = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * MR_THREADS) {
        const unsigned long long key = z[i];
        const int64_t f = (int64_t)(key & 0xFFFFFFFFull);
        float rgb[3] = {o.bg[0], o.bg[1], o.bg[2]}, bary[3] = {0.f, 0.f, 0.f}, t = 0.f, disp = 0.f, acc = 0.f;
        int32_t id = -1;
        // a word that is not a hit of this mesh (written by nobody, or a workspace of another call) is a miss: nothing is followed
        if (key != MESHRENDER_EMPTY && f < s.F && meshrender_face_ok(s.verts, s.faces, f, s.V)) {
            const int64_t n = i / hw, r = i - n * hw;
            const int py = (int)(r / s.W), px = (int)(r - (int64_t)py * s.W);
            const Cam cam = mr_cam(s, n);
            float v[9], d[3];
            mr_load_face(s, f, v);
            ray_dir(cam, (float)px, (float)py, d[0], d[1], d[2]);
            MeshrenderHit h;
            meshrender_hit(v, v + 3, v + 6, cam.t, d, 0.f, 0.f, MESHRENDER_CULL_NONE, h);        // the same U, V, W, det, t: the window is the raster's
            id = (int32_t)f;
            t = h.tf;
            disp = (float)(1.0 / (double)h.tf);
            acc = 1.f;
            bary[0] = (float)(h.U / h.det); bary[1] = (float)(h.V / h.det); bary[2] = (float)(h.W / h.det);
            if (o.rgb) {
                const int64_t a = s.faces[3 * f], b = s.faces[3 * f + 1], c = s.faces[3 * f + 2];
                const float *col = o.colors, *nor = o.normals;
                meshrender_shade(o.shading, h, col ? col + 3 * a : nullptr, col ? col + 3 * b : nullptr, col ? col + 3 * c : nullptr,
                                 nor ? nor + 3 * a : nullptr, nor ? nor + 3 * b : nullptr, nor ? nor + 3 * c : nullptr, d, rgb);
            }
        }
        o.face[i] = id;
        if (o.depth) o.depth[i] = t;
        if (o.disp) o.disp[i] = disp;
        if (o.acc) o.acc[i] = acc;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (o.bary) o.bary[3 * i + k] = bary[k];
            if (o.rgb) o.rgb[3 * i + k] = rgb[k];
        }
    }
}

extern "C" int swnerf_mesh_render_resolve(const float* verts, const int32_t* faces, const float* normals, const float* colors, int64_t V, int64_t F,
                                          const float* c2w, int64_t N, int H, int W, double fx, double fy, double cx, double cy, int focal_branch,
                                          int shading, const float* background, const void* workspace, float* rgb, float* depth, float* disp,
                                          float* acc, int32_t* face, float* bary, void* stream) {
    MrScene s;
    int rc = mr_scene("mesh_render_resolve", s, verts, faces, V, F, c2w, N, H, W, fx, fy, cx, cy, focal_branch);
    if (rc) return rc;
    if (shading < MESHRENDER_SHADE_COLORS || shading > MESHRENDER_SHADE_HEADLIGHT) return sw_fail(SWNERF_E_ARG, "mesh_render_resolve: unknown shading mode %d", shading);
    if (rgb && shading == MESHRENDER_SHADE_COLORS && !colors && F > 0) return sw_fail(SWNERF_E_ARG, "mesh_render_resolve: shading by colours needs vertex colours");
    if (rgb && shading != MESHRENDER_SHADE_COLORS && !normals && F > 0) return sw_fail(SWNERF_E_ARG, "mesh_render_resolve: shading by normals needs vertex normals");
    if (rgb && !background) return sw_fail(SWNERF_E_ARG, "mesh_render_resolve: rgb needs a background colour");
    const int64_t pixels = N * H * W;
    if (pixels == 0) return 0;
    if (!workspace || !face) return sw_fail(SWNERF_E_ARG, "mesh_render_resolve: NULL workspace / face");
    MrOut o{normals, colors, rgb, depth, disp, acc, bary, face, {0.f, 0.f, 0.f}, shading};
    for (int k = 0; k < 3 && background; ++k) o.bg[k] = background[k];
    hipLaunchKernelGGL(mr_resolve_kernel, dim3(mo_blocks(pixels)), dim3(MR_THREADS), 0, (hipStream_t)stream, s, o, (const unsigned long long*)workspace);
    return sw_check(hipGetLastError(), "mesh_render_resolve launch");
}

struct MrCompare {
    const float *acc, *depth, *ref_depth;
    const void* alpha;
    int alpha_u8;
    int64_t stride, offset, hw;
};

// covered by the reference: alpha above half of full scale (a byte: >= 128); without an alpha, a reference depth above 0
__device__ __forceinline__ bool mr_ref_covered(const MrCompare& c, int64_t i) {
    if (!c.alpha) return c.ref_depth[i] > 0.f;
    const int64_t e = i * c.stride + c.offset;
    return c.alpha_u8 ? ((const uint8_t*)c.alpha)[e] >= 128 : ((const float*)c.alpha)[e] > 0.5f;
}

__global__ __launch_bounds__(MESHRENDER_CMP_LANES) void mr_compare_kernel(MrCompare c, int64_t* counts, double* sums) {
    __shared__ double red[3][MESHRENDER_CMP_LANES];
    __shared__ unsigned long long cnt[4][MESHRENDER_CMP_LANES];
    const int t = threadIdx.x;
    const int64_t n = blockIdx.x;
    double s1 = 0.0, s2 = 0.0, sn = 0.0;
    unsigned long long ni = 0, nu = 0, nm = 0, nr = 0;
    for (int64_t q = t; q < c.hw; q += MESHRENDER_CMP_LANES) {
        const int64_t i = n * c.hw + q;
        const bool m = c.acc[i] > 0.5f, r = mr_ref_covered(c, i);
        ni += m && r; nu += m || r; nm += m; nr += r;
        if (m && r && c.depth && c.ref_depth) {
            const double d = (double)c.depth[i] - (double)c.ref_depth[i];
            s1 += fabs(d);
            s2 += d * d;
            sn += 1.0;
        }
    }
    red[0][t] = s1; red[1][t] = s2; red[2][t] = sn;
    cnt[0][t] = ni; cnt[1][t] = nu; cnt[2][t] = nm; cnt[3][t] = nr;
    __syncthreads();
    for (int w = MESHRENDER_CMP_LANES / 2; w >= 1; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int k = 0; k < 3; ++k) red[k][t] += red[k][t + w];
#pragma unroll
            for (int k = 0; k < 4; ++k) cnt[k][t] += cnt[k][t + w];
        }
        __syncthreads();
    }
    if (t < 3) sums[3 * n + t] = red[t][0];
    if (t < 4) counts[4 * n + t] = (int64_t)cnt[t][0];
}

extern "C" int swnerf_mesh_view_compare(const float* acc, const float* depth, const void* ref_alpha, int alpha_u8, int64_t alpha_stride,
                                        int64_t alpha_offset, const float* ref_depth, int64_t N, int64_t H, int64_t W, int64_t* counts, double* sums,
                                        void* stream) {
    if (!mr_sizes_ok(N, H, W))
        return sw_fail(SWNERF_E_ARG, "mesh_view_compare: N = %lld views of %lld x %lld: need N >= 0, H, W >= 1 and N H W < 2^31", (long long)N, (long long)H, (long long)W);
    if (N == 0) return 0;
    if (!acc || !counts || !sums) return sw_fail(SWNERF_E_ARG, "mesh_view_compare: NULL acc / counts / sums");
    if (!ref_alpha && !ref_depth) return sw_fail(SWNERF_E_ARG, "mesh_view_compare: needs a reference alpha or a reference depth");
    if (ref_alpha && (alpha_stride < 1 || alpha_offset < 0 || alpha_offset >= alpha_stride))
        return sw_fail(SWNERF_E_ARG, "mesh_view_compare: alpha stride %lld / offset %lld: need stride >= 1 and 0 <= offset < stride", (long long)alpha_stride,
                       (long long)alpha_offset);
    MrCompare c{acc, depth, ref_depth, ref_alpha, alpha_u8 ? 1 : 0, alpha_stride, alpha_offset, H * W};
    hipLaunchKernelGGL(mr_compare_kernel, dim3((unsigned)N), dim3(MESHRENDER_CMP_LANES), 0, (hipStream_t)stream, c, counts, sums);
    return sw_check(hipGetLastError(), "mesh_view_compare launch");
}
