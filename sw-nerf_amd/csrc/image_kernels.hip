// image_kernels.hip - the image half of the dataset loaders (dataloader/*.py: imageio.imread of 8-bit PNGs, cv2.resize with
// INTER_AREA), DESIGN.md 6k.  Two entry points, one launch each on the caller's stream, no workspace, no atomics on global memory:
//   png_unfilter  undoes the five PNG row filters of n equally sized images.  A filtered byte depends on the unfiltered byte bpp
//                 to its left (a), the one above (b) and the one above-left (c), so the work is parallel across images, across
//                 the bpp byte lanes of a pixel and along a skewed wavefront of rows: one workgroup per image, thread r owns row
//                 band * IMG_ROWS + r of a band of IMG_ROWS rows and unfilters pixel x = s - r (all bpp bytes) at step s.  a
//                 stays in registers, c is the previous step's b, and b is the pixel thread r - 1 put into LDS one step earlier
//                 (two buffers, one barrier per step); the first row of a later band reads b from `out`, where the last thread
//                 of the band before stored it.  Rows of different filter types share the one uniform loop.  Every thread
//                 reaches every barrier: a thread whose row is >= H or whose x is outside 0..W-1 idles INSIDE the loop, and the
//                 trip counts depend on H, W and IMG_ROWS only.  A type byte above 4 is recorded (the smallest such row per image,
//                 through an LDS minimum) and the row copied; nothing is read or written outside the two operands.
//                 filtered rows are 1 + W * bpp bytes, so nothing is aligned: every load from `filtered` is a byte load; `out`
//                 is stored as one 32-bit word per pixel only when bpp == 4 and `out` is 4-byte aligned, else byte by byte.
//   area_resize   dst[n,h,w,c] fp32 = the area mean of src[n,H,W,c] (uint8 or fp32) over [i H/h, (i+1) H/h) x [j W/w, (j+1) W/w).
//                 Integer factors: one thread per destination PIXEL sums its fy x fx block in fp64 in row-major order and divides
//                 once (RGBA bytes: one 32-bit load per source pixel when src is 4-byte aligned).  Other sizes: one thread per
//                 destination FLOAT; the overlap of source cell y with the destination interval, in units of 1/h, is the integer
//                 min((i+1) H, (y+1) h) - max(i H, y h) - no rounding decides which cells are touched, so no index leaves the image.
// All element offsets are 64-bit.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include "../../include/swnerf.h"
#include "host_util.h"

#define IMG_ROWS 256                    // rows of a band == threads of an unfilter workgroup
#define IMG_THREADS 256                 // resize
#define IMG_MAX_BLOCKS (1 << 20)        // above this many blocks a kernel strides over its work
#define IMG_MAX_SIDE (1 << 20)

// ---- png_unfilter ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ int img_paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

template <int BPP, bool WORD>
__global__ __launch_bounds__(IMG_ROWS) void png_unfilter_kernel(const uint8_t* __restrict__ filtered, int64_t n, int H, int W,
                                                                uint8_t* out, int32_t* __restrict__ status) {
    __shared__ uint32_t above[2][IMG_ROWS];          // the pixel each thread unfiltered in the previous / this step
    __shared__ int first_bad;
    const int r = threadIdx.x;
    const int64_t row_in = 1 + (int64_t)W * BPP, row_out = (int64_t)W * BPP;
    const int bands = (H + IMG_ROWS - 1) / IMG_ROWS;
    const int steps = W + IMG_ROWS - 1;
    for (int64_t img = blockIdx.x; img < n; img += gridDim.x) {             // uniform over the workgroup
        const uint8_t* F = filtered + img * (int64_t)H * row_in;
        uint8_t* O = out + img * (int64_t)H * row_out;
        if (r == 0) first_bad = INT_MAX;
        __syncthreads();
        for (int band = 0; band < bands; ++band) {
            const int row = band * IMG_ROWS + r;
            const bool live = row < H;
            int ft = 0;
            if (live) {
                ft = F[(int64_t)row * row_in];
                if (ft > 4) {
                    atomicMin(&first_bad, row);
                    ft = 0;
                }
            }
            const uint8_t* Frow = F + (int64_t)(live ? row : 0) * row_in + 1;
            uint8_t* Orow = O + (int64_t)(live ? row : 0) * row_out;
            const uint8_t* Oup = Orow - row_out;                             // read only when row > 0 and r == 0
            uint32_t a = 0, c = 0;
            for (int s = 0; s < steps; ++s) {
                const int x = s - r;
                if (live && x >= 0 && x < W) {
                    uint32_t b = 0;
                    if (row > 0) {
                        if (r > 0) {
                            b = above[(s & 1) ^ 1][r - 1];
                        } else {
#pragma unroll
                            for (int k = 0; k < BPP; ++k) b |= (uint32_t)Oup[(int64_t)x * BPP + k] << (8 * k);
                        }
                    }
                    uint32_t cur = 0;
#pragma unroll
                    for (int k = 0; k < BPP; ++k) {
                        const int f = Frow[(int64_t)x * BPP + k];
                        const int ak = (a >> (8 * k)) & 255, bk = (b >> (8 * k)) & 255, ck = (c >> (8 * k)) & 255;
                        const int pred = ft == 0 ? 0 : ft == 1 ? ak : ft == 2 ? bk : ft == 3 ? ((ak + bk) >> 1) : img_paeth(ak, bk, ck);
                        cur |= (uint32_t)((f + pred) & 255) << (8 * k);
                    }
                    if (WORD) {
                        *reinterpret_cast<uint32_t*>(Orow + (int64_t)x * 4) = cur;
                    } else {
#pragma unroll
                        for (int k = 0; k < BPP; ++k) Orow[(int64_t)x * BPP + k] = (uint8_t)(cur >> (8 * k));
                    }
                    above[s & 1][r] = cur;
                    a = cur;
                    c = b;
                }
                __syncthreads();                                            // also orders the stores to `out` for the next band's row 0
            }
        }
        if (r == 0) status[img] = first_bad == INT_MAX ? 0 : 1 + first_bad;
        __syncthreads();                                                    // first_bad is reset for the next image after this
    }
}

// ---- area_resize -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float img_byte(uint32_t u) { return (float)((double)u / 255.); }

template <bool U8>
__device__ __forceinline__ double img_value(const void* src, int64_t e) {
    return U8 ? (double)img_byte(static_cast<const uint8_t*>(src)[e]) : (double)static_cast<const float*>(src)[e];
}

// integer factors fy = H / h, fx = W / w: one thread per destination pixel
template <int C, bool U8, bool WORD>
__global__ __launch_bounds__(IMG_THREADS) void area_block_kernel(const void* __restrict__ src, int64_t n, int H, int W, int h, int w,
                                                                 float* __restrict__ dst) {
    const int fy = H / h, fx = W / w;
    const int64_t total = n * (int64_t)h * w;
    const double scale = (double)fy * (double)fx;
    for (int64_t p = (int64_t)blockIdx.x * IMG_THREADS + threadIdx.x; p < total; p += (int64_t)gridDim.x * IMG_THREADS) {
        const int64_t rowi = p / w;
        const int j = (int)(p - rowi * w);
        const int64_t img = rowi / h;
        const int i = (int)(rowi - img * h);
        double acc[C];
#pragma unroll
        for (int k = 0; k < C; ++k) acc[k] = 0.;
        for (int dy = 0; dy < fy; ++dy) {
            const int64_t base = ((img * H + (int64_t)i * fy + dy) * W + (int64_t)j * fx) * C;
            for (int dx = 0; dx < fx; ++dx) {
                const int64_t e = base + (int64_t)dx * C;
                if (WORD) {                                                  // C == 4 bytes, src 4-byte aligned
                    const uint32_t q = *reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(src) + e);
#pragma unroll
                    for (int k = 0; k < C; ++k) acc[k] += (double)img_byte((q >> (8 * k)) & 255u);
                } else {
#pragma unroll
                    for (int k = 0; k < C; ++k) acc[k] += img_value<U8>(src, e + k);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < C; ++k) dst[p * C + k] = (float)(acc[k] / scale);
    }
}

// any h <= H, w <= W: one thread per destination float
template <bool U8>
__global__ __launch_bounds__(IMG_THREADS) void area_general_kernel(const void* __restrict__ src, int64_t n, int H, int W, int C, int h,
                                                                   int w, float* __restrict__ dst) {
    const int rowlen = w * C;
    const int64_t total = n * (int64_t)h * rowlen;
    const double norm = (double)H * (double)W;
    for (int64_t e = (int64_t)blockIdx.x * IMG_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * IMG_THREADS) {
        const int64_t rowi = e / rowlen;
        const int f = (int)(e - rowi * rowlen);
        const int64_t img = rowi / h;
        const int i = (int)(rowi - img * h);
        const int j = f / C, k = f - j * C;
        // in units of 1/h (rows) and 1/w (columns): destination [i H, (i+1) H), source cell y covers [y h, (y+1) h)
        const int64_t ylo = (int64_t)i * H, yhi = ylo + H, xlo = (int64_t)j * W, xhi = xlo + W;
        const int y0 = (int)(ylo / h), y1 = (int)((yhi + h - 1) / h);        // y1 <= H, x1 <= W
        const int x0 = (int)(xlo / w), x1 = (int)((xhi + w - 1) / w);
        double acc = 0.;
        for (int y = y0; y < y1; ++y) {
            const int64_t oy = min(yhi, ((int64_t)y + 1) * h) - max(ylo, (int64_t)y * h);
            double rowsum = 0.;
            for (int x = x0; x < x1; ++x) {
                const int64_t ox = min(xhi, ((int64_t)x + 1) * w) - max(xlo, (int64_t)x * w);
                rowsum += (double)ox * img_value<U8>(src, ((img * H + y) * W + x) * C + k);
            }
            acc += (double)oy * rowsum;
        }
        dst[e] = (float)(acc / norm);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------
static int img_check_size(const char* who, int64_t n, int64_t h, int64_t w) {
    if (n < 0) return sw_fail(SWNERF_E_ARG, "%s: negative image count %lld", who, (long long)n);
    if (h < 1 || w < 1 || h > IMG_MAX_SIDE || w > IMG_MAX_SIDE)
        return sw_fail(SWNERF_E_ARG, "%s: image size %lld x %lld outside 1..2^20", who, (long long)h, (long long)w);
    return 0;
}

static unsigned img_blocks(int64_t items, int per_block) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b > IMG_MAX_BLOCKS ? IMG_MAX_BLOCKS : b));
}

extern "C" int swnerf_png_unfilter(const uint8_t* filtered, int64_t n, int64_t H, int64_t W, int bpp, uint8_t* out, int32_t* status,
                                   void* stream) {
    int rc = img_check_size("png_unfilter", n, H, W);
    if (rc) return rc;
    if (bpp != 3 && bpp != 4) return sw_fail(SWNERF_E_ARG, "png_unfilter: %d bytes per pixel; 3 (RGB) and 4 (RGBA) are built", bpp);
    if (n == 0) return 0;
    if (!filtered || !out || !status) return sw_fail(SWNERF_E_ARG, "png_unfilter: NULL pointer");
    if ((uintptr_t)status & 3) return sw_fail(SWNERF_E_ARG, "png_unfilter: status must be 4-byte aligned");
    const unsigned blocks = img_blocks(n, 1);
    hipStream_t st = (hipStream_t)stream;
    if (bpp == 3) hipLaunchKernelGGL((png_unfilter_kernel<3, false>), dim3(blocks), dim3(IMG_ROWS), 0, st, filtered, n, (int)H, (int)W, out, status);
    else if ((uintptr_t)out & 3) hipLaunchKernelGGL((png_unfilter_kernel<4, false>), dim3(blocks), dim3(IMG_ROWS), 0, st, filtered, n, (int)H, (int)W, out, status);
    else hipLaunchKernelGGL((png_unfilter_kernel<4, true>), dim3(blocks), dim3(IMG_ROWS), 0, st, filtered, n, (int)H, (int)W, out, status);
    return sw_check(hipGetLastError(), "png_unfilter launch");
}

template <bool U8, bool WORD>
static void img_launch_block(int c, unsigned blocks, hipStream_t st, const void* src, int64_t n, int H, int W, int h, int w, float* dst) {
    switch (c) {
    case 1: hipLaunchKernelGGL((area_block_kernel<1, U8, false>), dim3(blocks), dim3(IMG_THREADS), 0, st, src, n, H, W, h, w, dst); break;
    case 2: hipLaunchKernelGGL((area_block_kernel<2, U8, false>), dim3(blocks), dim3(IMG_THREADS), 0, st, src, n, H, W, h, w, dst); break;
    case 3: hipLaunchKernelGGL((area_block_kernel<3, U8, false>), dim3(blocks), dim3(IMG_THREADS), 0, st, src, n, H, W, h, w, dst); break;
    default: hipLaunchKernelGGL((area_block_kernel<4, U8, WORD>), dim3(blocks), dim3(IMG_THREADS), 0, st, src, n, H, W, h, w, dst); break;
    }
}

extern "C" int swnerf_area_resize(const void* src, int src_u8, int64_t n, int64_t H, int64_t W, int c, int64_t h, int64_t w, float* dst,
                                  void* stream) {
    int rc = img_check_size("area_resize", n, H, W);
    if (rc) return rc;
    if (c < 1 || c > 4) return sw_fail(SWNERF_E_ARG, "area_resize: %d channels; 1..4 are built", c);
    if (h < 1 || w < 1 || h > H || w > W)
        return sw_fail(SWNERF_E_ARG, "area_resize: %lld x %lld -> %lld x %lld is not a down-scale (the area mean is defined for 1 <= h <= H, 1 <= w <= W)",
                       (long long)H, (long long)W, (long long)h, (long long)w);
    if (n == 0) return 0;
    if (!src || !dst) return sw_fail(SWNERF_E_ARG, "area_resize: NULL pointer");
    if (((uintptr_t)dst & 3) || (!src_u8 && ((uintptr_t)src & 3))) return sw_fail(SWNERF_E_ARG, "area_resize: float operands must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (H % h == 0 && W % w == 0) {
        const unsigned blocks = img_blocks(n * h * w, IMG_THREADS);
        if (!src_u8) img_launch_block<false, false>(c, blocks, st, src, n, (int)H, (int)W, (int)h, (int)w, dst);
        else if (c == 4 && !((uintptr_t)src & 3)) img_launch_block<true, true>(c, blocks, st, src, n, (int)H, (int)W, (int)h, (int)w, dst);
        else img_launch_block<true, false>(c, blocks, st, src, n, (int)H, (int)W, (int)h, (int)w, dst);
    } else {
        const unsigned blocks = img_blocks(n * h * w * c, IMG_THREADS);
        if (src_u8) hipLaunchKernelGGL((area_general_kernel<true>), dim3(blocks), dim3(IMG_THREADS), 0, st, src, n, (int)H, (int)W, c, (int)h, (int)w, dst);
        else hipLaunchKernelGGL((area_general_kernel<false>), dim3(blocks), dim3(IMG_THREADS), 0, st, src, n, (int)H, (int)W, c, (int)h, (int)w, dst);
    }
    return sw_check(hipGetLastError(), "area_resize launch");
}
