// view_ws.h - the workspace of the deferred colour branch of the static fp32 inference pass (swnerf_render_pass_ws): its layout,
// shared by phase A (render_pass.h render_pass_kernel<false>) and phases B and C (colour_kernels.hip).
//
// A sample's colour enters the outputs as w.c with w = alpha.T, and alpha = 1 - exp(-relu(sigma).dist) is exactly 0 for every
// sample with sigma <= 0: the view layer and the rgb head of such a row (512 of a tile's 8192 MFMAs + the tail) are multiplied
// by an exact zero.  With a workspace the launch evaluates them on the LIVE rows only - alpha != 0 (NaN counts), and sample 0 of
// the ray as a canary, so that a non-finite view/rgb weight, bias or direction still reaches rgb_map - packed 32 to a view
// segment ACROSS rays.  A view segment needs a row's ReLU'd h7 and its direction and no per-ray state, and the columns of an
// MFMA are independent, so which rows share a segment changes no bit.  Three kernels on one stream:
//   A  render_pass_kernel<false> (render_pass.h): trunk, sigma head, density compositing, resampling and every per-sample output
//      as ever.  A tile whose rows are certain to fit the ray's region of the workspace (decided BEFORE the trunk, so that layer
//      7's last prefetches go to the head of the next tile: WStream.cont) stashes its live rows' h7 and leaves the view segment
//      out; any other tile runs it in line on its own rows.  Per ray the region also takes w[S], the raw colours c[3][S] (0 for
//      dead and for stashed rows), the sample index of every stashed row and acc, the launch header their count.  No rgb_map.
//   B  colour_rows_kernel (colour_kernels.hip): persistent waves; segment g = stashed rows 32g .. 32g+31 of the launch in ray
//      order, located through the prefix of the rays' counts (colour_scan_kernel in front of it).  Each lane loads its row,
//      forms gamma(d) of the row's ray and runs the 4 x 9 view layer from the blob's views-loop stream and the rgb head
//      (mlp_kernels.h views_mean with rows read instead of computed: the sum order of DIR + VIEWSH), then scatters the raw
//      colour to c[.][sample] of its ray.
//   C  colour_maps_kernel (same unit): one wave per ray forms the colour sums as the tile loop does in line - lane j takes sample
//      32 t + j, tiles ascending - and writes rgb_map.
// The same operations in the same order, so the outputs are the in-line launch's bit for bit whenever the colours left out were
// finite.
//
// Workspace (floats; ViewWs below):  launch header | n_rays regions of `per_ray`
//   header: int off[n_rays + 1] (A: a ray's count; the scan: their exclusive prefix; padded to 4) | int segray[8 n_rays] (the ray
//           that holds row 32g)
//   region: float acc, 3 pad | w[Sp] | c[3][Sp] | int sample[R] | rows [g 32][h 2][slot R][4]                  (Sp = S up to 4)
// rows: register group g of lane (slot, h)'s B operand - ONE store instruction writes adjacent 16-byte cells for adjacent slots.
// R follows from the workspace's size (at most Sp: then every tile stashes); n_rays x 64 x 256 floats is the accepted minimum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SW_DEFER_SMAX 240
#define SW_DEFER_WS_FLOATS (64 * 256)            // least workspace floats per ray
#define SW_DEFER_SEGS_PER_RAY ((SW_DEFER_SMAX + 31) / 32)

struct ViewWs {
    float* base;            // NULL = the launch runs the colour branch in line
    int64_t hdr, per_ray;   // floats: launch header, one ray's region
    int rows, sp;           // R, Sp
};

static inline int64_t view_ws_hdr(int64_t n_rays) { return ((n_rays + 1 + 3) & ~(int64_t)3) + SW_DEFER_SEGS_PER_RAY * n_rays; }
// floats with which every tile of every ray stashes
static inline int64_t view_ws_full(int64_t n_rays, int S) {
    const int64_t sp = (S + 3) & ~3;
    return view_ws_hdr(n_rays) + n_rays * (4 + 4 * sp + 257 * sp);
}
static inline ViewWs view_ws_layout(float* base, int64_t floats, int64_t n_rays, int S) {
    ViewWs v = {};
    v.base = base;
    v.sp = (S + 3) & ~3;
    v.hdr = view_ws_hdr(n_rays);
    const int64_t avail = n_rays > 0 ? ((floats - v.hdr) / n_rays) & ~(int64_t)3 : 0;
    int64_t r = ((avail - 4 - 4 * v.sp) / 257) & ~(int64_t)3;
    if (r > v.sp) r = v.sp;
    v.rows = r > 0 ? (int)r : 0;
    v.per_ray = 4 + 4 * (int64_t)v.sp + 257 * (int64_t)v.rows;
    return v;
}
__device__ __forceinline__ int* vw_off(const ViewWs& v) { return reinterpret_cast<int*>(v.base); }
__device__ __forceinline__ int* vw_segray(const ViewWs& v, int64_t n_rays) { return reinterpret_cast<int*>(v.base) + ((n_rays + 1 + 3) & ~(int64_t)3); }
__device__ __forceinline__ float* vw_ray(const ViewWs& v, int64_t ray) { return v.base + v.hdr + ray * v.per_ray; }
__device__ __forceinline__ float* vw_w(float* reg) { return reg + 4; }
__device__ __forceinline__ float* vw_c(const ViewWs& v, float* reg) { return reg + 4 + v.sp; }
__device__ __forceinline__ int* vw_sample(const ViewWs& v, float* reg) { return reinterpret_cast<int*>(reg + 4 + 4 * v.sp); }
// this lane's cell of register group 0 of `slot`; group g is g * vw_group_stride() floats further on
__device__ __forceinline__ float* vw_row(const ViewWs& v, float* reg, int slot, int h) { return reg + 4 + 4 * v.sp + v.rows + (h * v.rows + slot) * 4; }
__device__ __forceinline__ int vw_group_stride(const ViewWs& v) { return 8 * v.rows; }
