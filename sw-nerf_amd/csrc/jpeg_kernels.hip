// jpeg_kernels.hip - baseline JPEG frames of the dataset loaders (the LLFF scenes' camera files, the pictures of
// 2d_pos_encoding): the host parses markers and decodes the Huffman stream (jpeg_host.h, no GPU call), the device does what is
// parallel, with libjpeg's default integer arithmetic (jpeg_math.h) so that the pixels equal imageio.imread's byte for byte.
// DESIGN.md 6k "JPEG".  swnerf_jpeg_decode is two launches on the caller's stream, no atomics, no host synchronisation:
//   jpeg_idct_kernel    one lane per 8 x 8 block: 128 bytes of int16 coefficients and the 128 bytes of the component's
//                       quantisation table come in as eight 16-byte loads each, the 64 values stay in registers through both
//                       1-D passes (every index is a compile-time constant), and the block leaves as eight 8-byte row stores
//                       into the component's plane; neighbouring lanes hold neighbouring blocks, so their stores to one plane
//                       row are adjacent.  No LDS.
//   jpeg_pixels_kernel  one lane per 4 horizontal pixels: a 4-byte luma load, the chroma taps of the triangle filter (the 2-D
//                       halo reaches into neighbouring MCUs, which is why this is a second kernel), colour conversion, and 12 or
//                       16 bytes stored as words when the address allows, byte by byte otherwise (an unaligned `out`, RGB rows
//                       whose width is no multiple of 4, the last pixels of a row).
// Planes are padded to whole MCUs; samples beyond ceil(W h / hmax) columns or ceil(H v / vmax) rows are never read.
// All element offsets are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/swnerf.h"
#include "host_util.h"
#include "jpeg_host.h"

#define JPEG_THREADS 256
#define JPEG_MAX_BLOCKS (1 << 20)       // above this many workgroups a kernel strides over its work

static_assert(SWNERF_JPEG_444 == JPEG_444 && SWNERF_JPEG_422 == JPEG_422 && SWNERF_JPEG_420 == JPEG_420, "swnerf.h and jpeg_math.h disagree");
static_assert(SWNERF_JPEG_INFO_LEN >= 6, "jpeg_header fills six entries");

// ---- dequantise + inverse DCT ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_idct_kernel(const int16_t* __restrict__ coef, const uint16_t* __restrict__ qt, int64_t n,
                                                                 int ncomp, int bx0, int by0, int bx1, int by1, uint8_t* __restrict__ planes) {
    const int64_t B0 = (int64_t)bx0 * by0, B1 = (int64_t)bx1 * by1, B = B0 + (ncomp == 3 ? 2 * B1 : 0);
    const int64_t total = n * B;
    for (int64_t g = (int64_t)blockIdx.x * JPEG_THREADS + threadIdx.x; g < total; g += (int64_t)gridDim.x * JPEG_THREADS) {
        const int64_t img = g / B;
        int64_t rem = g - img * B;                                              // block within the image: planes follow each other
        int comp = 0, pbx = bx0;
        int64_t plane_off = 0;
        if (rem >= B0) {
            comp = 1 + (int)((rem - B0) / B1);
            plane_off = B0 + (comp - 1) * B1;
            rem -= plane_off;
            pbx = bx1;
        }
        const int byi = (int)(rem / pbx), bxi = (int)(rem - (int64_t)byi * pbx);
        const uint4* C = reinterpret_cast<const uint4*>(coef + g * 64);
        const uint4* Q = reinterpret_cast<const uint4*>(qt + (img * ncomp + comp) * 64);
        int32_t v[64];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint4 c = C[k], q = Q[k];
            const uint32_t cw[4] = {c.x, c.y, c.z, c.w}, qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[8 * k + 2 * j] = jpeg_mul((int32_t)(int16_t)(cw[j] & 0xFFFFu), (int32_t)(qw[j] & 0xFFFFu));
                v[8 * k + 2 * j + 1] = jpeg_mul((int32_t)(int16_t)(cw[j] >> 16), (int32_t)(qw[j] >> 16));
            }
        }
        jpeg_idct_block(v);
        const int64_t stride = (int64_t)pbx * 8;
        uint8_t* P = planes + (img * B + plane_off) * 64 + (int64_t)byi * 8 * stride + (int64_t)bxi * 8;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            uint2 w;
            w.x = (uint32_t)v[8 * r] | (uint32_t)v[8 * r + 1] << 8 | (uint32_t)v[8 * r + 2] << 16 | (uint32_t)v[8 * r + 3] << 24;
            w.y = (uint32_t)v[8 * r + 4] | (uint32_t)v[8 * r + 5] << 8 | (uint32_t)v[8 * r + 6] << 16 | (uint32_t)v[8 * r + 7] << 24;
            *reinterpret_cast<uint2*>(P + r * stride) = w;
        }
    }
}

// ---- up-sampling + colour -------------------------------------------------------------------------------------------------
template <int NCOMP, int SAMPLING, int COUT>
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_pixels_kernel(const uint8_t* __restrict__ planes, int64_t n, int H, int W, int bx0, int by0,
                                                                   int bx1, int by1, uint8_t* __restrict__ out, int out_words) {
    const int64_t B0 = (int64_t)bx0 * by0, B1 = (int64_t)bx1 * by1, B = B0 + (NCOMP == 3 ? 2 * B1 : 0);
    const int Wq = (W + 3) >> 2;
    const int64_t total = n * (int64_t)H * Wq;
    const int64_t ys = (int64_t)bx0 * 8, cs = (int64_t)bx1 * 8;                 // row strides of the luma and chroma planes
    const int dw = SAMPLING == JPEG_444 ? W : (W + 1) >> 1, dh = SAMPLING == JPEG_420 ? (H + 1) >> 1 : H;
    for (int64_t t = (int64_t)blockIdx.x * JPEG_THREADS + threadIdx.x; t < total; t += (int64_t)gridDim.x * JPEG_THREADS) {
        const int64_t rowi = t / Wq;
        const int x0 = (int)(t - rowi * Wq) * 4;
        const int64_t img = rowi / H;
        const int y = (int)(rowi - img * H);
        const uint8_t* Y = planes + img * B * 64;
        const uint32_t yw = *reinterpret_cast<const uint32_t*>(Y + y * ys + x0);   // within the padded row: bx0 * 8 >= x0 + 4
        const int live = min(4, W - x0);
        uint8_t px[4 * COUT];
        if (NCOMP == 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint8_t s = (uint8_t)(yw >> (8 * j));
                px[j * COUT] = px[j * COUT + 1] = px[j * COUT + 2] = s;
                if (COUT == 4) px[j * COUT + 3] = 255;
            }
        } else {
            const uint8_t* Cb = Y + B0 * 64;
            const uint8_t* Cr = Cb + B1 * 64;
            const int cy = SAMPLING == JPEG_420 ? y >> 1 : y;
            const int64_t near = cy * cs, far = SAMPLING == JPEG_420 ? jpeg_far_row(y, dh) * cs : 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = min(x0 + j, W - 1);                               // lanes past the row's end repeat its last pixel, unstored
                int cb, cr;
                if (SAMPLING == JPEG_444) {
                    cb = Cb[near + x];
                    cr = Cr[near + x];
                } else if (SAMPLING == JPEG_422) {
                    cb = jpeg_up_h2v1(Cb + near, dw, x);
                    cr = jpeg_up_h2v1(Cr + near, dw, x);
                } else {
                    cb = jpeg_up_h2v2(Cb + near, Cb + far, dw, x);
                    cr = jpeg_up_h2v2(Cr + near, Cr + far, dw, x);
                }
                int r, g, b;
                jpeg_ycc_to_rgb((int)((yw >> (8 * j)) & 255u), cb, cr, &r, &g, &b);
                px[j * COUT] = (uint8_t)r;
                px[j * COUT + 1] = (uint8_t)g;
                px[j * COUT + 2] = (uint8_t)b;
                if (COUT == 4) px[j * COUT + 3] = 255;
            }
        }
        const int64_t e = ((img * H + y) * (int64_t)W + x0) * COUT;
        if (out_words && live == 4 && (e & 3) == 0) {
#pragma unroll
            for (int k = 0; k < COUT; ++k)
                reinterpret_cast<uint32_t*>(out + e)[k] = (uint32_t)px[4 * k] | (uint32_t)px[4 * k + 1] << 8 | (uint32_t)px[4 * k + 2] << 16 | (uint32_t)px[4 * k + 3] << 24;
        } else {
#pragma unroll
            for (int k = 0; k < 4 * COUT; ++k)
                if (k < live * COUT) out[e + k] = px[k];
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static unsigned jpeg_grid(int64_t items) {
    const int64_t b = (items + JPEG_THREADS - 1) / JPEG_THREADS;
    return (unsigned)(b < 1 ? 1 : (b > JPEG_MAX_BLOCKS ? JPEG_MAX_BLOCKS : b));
}

static int jpeg_check_geometry(const char* who, int64_t H, int64_t W, int ncomp, int sampling) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535) return sw_fail(SWNERF_E_ARG, "%s: image size %lld x %lld outside 1..65535", who, (long long)H, (long long)W);
    if (ncomp != 1 && ncomp != 3) return sw_fail(SWNERF_E_ARG, "%s: %d components; 1 and 3 are built", who, ncomp);
    if (sampling != JPEG_444 && sampling != JPEG_422 && sampling != JPEG_420) return sw_fail(SWNERF_E_ARG, "%s: sampling %d is none of SWNERF_JPEG_444 / 422 / 420", who, sampling);
    if (ncomp == 1 && sampling != JPEG_444) return sw_fail(SWNERF_E_ARG, "%s: a single component is SWNERF_JPEG_444", who);
    return 0;
}

extern "C" int64_t swnerf_jpeg_coef_count(int64_t H, int64_t W, int ncomp, int sampling) {
    if (jpeg_check_geometry("jpeg_coef_count", H, W, ncomp, sampling)) return 0;
    int bx[2], by[2];
    return 64 * jpeg_blocks(H, W, ncomp, sampling, bx, by);
}

static int jpeg_status(int rc) { return rc == JPEG_OK ? 0 : rc == JPEG_UNSUPP ? SWNERF_E_UNSUPP : SWNERF_E_DATA; }

extern "C" int swnerf_jpeg_header(const uint8_t* data, int64_t len, int32_t* info, uint16_t* qt) {
    if (!data || len < 0 || !info || !qt) return sw_fail(SWNERF_E_ARG, "jpeg_header: NULL pointer or negative length");
    jpeg_info o;
    const int rc = jpeg_parse(data, len, &o, sw_errbuf(), SW_ERRBUF_LEN);
    if (rc != JPEG_OK) return jpeg_status(rc);
    const int32_t v[6] = {o.H, o.W, o.ncomp, o.sampling, o.restart, (int32_t)(o.scan > 0x7fffffff ? 0x7fffffff : o.scan)};
    memset(info, 0, SWNERF_JPEG_INFO_LEN * sizeof(int32_t));
    memcpy(info, v, sizeof(v));
    memset(qt, 0, SWNERF_JPEG_QT_LEN * sizeof(uint16_t));
    memcpy(qt, o.qt, (size_t)o.ncomp * 64 * sizeof(uint16_t));
    return 0;
}

extern "C" int swnerf_jpeg_entropy(const uint8_t* data, int64_t len, int16_t* coef, int64_t coef_count) {
    if (!data || len < 0 || !coef) return sw_fail(SWNERF_E_ARG, "jpeg_entropy: NULL pointer or negative length");
    jpeg_info o;
    int rc = jpeg_parse(data, len, &o, sw_errbuf(), SW_ERRBUF_LEN);
    if (rc != JPEG_OK) return jpeg_status(rc);
    if (coef_count != o.blocks * 64)
        return sw_fail(SWNERF_E_ARG, "jpeg_entropy: the file has %lld coefficients, the buffer %lld", (long long)(o.blocks * 64), (long long)coef_count);
    return jpeg_status(jpeg_entropy(data, len, &o, coef, sw_errbuf(), SW_ERRBUF_LEN));
}

template <int NCOMP, int SAMPLING>
static void jpeg_launch_pixels(int cout, unsigned blocks, hipStream_t st, const uint8_t* planes, int64_t n, int H, int W, const int* bx,
                               const int* by, uint8_t* out, int words) {
    if (cout == 3) hipLaunchKernelGGL((jpeg_pixels_kernel<NCOMP, SAMPLING, 3>), dim3(blocks), dim3(JPEG_THREADS), 0, st, planes, n, H, W, bx[0], by[0], bx[1], by[1], out, words);
    else hipLaunchKernelGGL((jpeg_pixels_kernel<NCOMP, SAMPLING, 4>), dim3(blocks), dim3(JPEG_THREADS), 0, st, planes, n, H, W, bx[0], by[0], bx[1], by[1], out, words);
}

extern "C" int swnerf_jpeg_decode(const int16_t* coef, const uint16_t* qt, int64_t n, int64_t H, int64_t W, int ncomp, int sampling,
                                  int channels_out, uint8_t* scratch_planes, uint8_t* out, void* stream) {
    int rc = jpeg_check_geometry("jpeg_decode", H, W, ncomp, sampling);
    if (rc) return rc;
    if (n < 0) return sw_fail(SWNERF_E_ARG, "jpeg_decode: negative image count %lld", (long long)n);
    if (channels_out != 3 && channels_out != 4) return sw_fail(SWNERF_E_ARG, "jpeg_decode: %d output channels; 3 (RGB) and 4 (RGBA, alpha 255) are built", channels_out);
    if (n == 0) return 0;
    if (!coef || !qt || !scratch_planes || !out) return sw_fail(SWNERF_E_ARG, "jpeg_decode: NULL pointer");
    if (((uintptr_t)coef & 15) || ((uintptr_t)qt & 15) || ((uintptr_t)scratch_planes & 7))
        return sw_fail(SWNERF_E_ARG, "jpeg_decode: coef and qt must be 16-byte aligned, scratch_planes 8-byte aligned");
    int bx[2], by[2];
    const int64_t B = jpeg_blocks(H, W, ncomp, sampling, bx, by);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(jpeg_grid(n * B)), dim3(JPEG_THREADS), 0, st, coef, qt, n, ncomp, bx[0], by[0], bx[1], by[1], scratch_planes);
    rc = sw_check(hipGetLastError(), "jpeg_decode idct launch");
    if (rc) return rc;
    const unsigned blocks = jpeg_grid(n * H * ((W + 3) / 4));
    const int words = ((uintptr_t)out & 3) == 0;
    if (ncomp == 1) jpeg_launch_pixels<1, JPEG_444>(channels_out, blocks, st, scratch_planes, n, (int)H, (int)W, bx, by, out, words);
    else if (sampling == JPEG_444) jpeg_launch_pixels<3, JPEG_444>(channels_out, blocks, st, scratch_planes, n, (int)H, (int)W, bx, by, out, words);
    else if (sampling == JPEG_422) jpeg_launch_pixels<3, JPEG_422>(channels_out, blocks, st, scratch_planes, n, (int)H, (int)W, bx, by, out, words);
    else jpeg_launch_pixels<3, JPEG_420>(channels_out, blocks, st, scratch_planes, n, (int)H, (int)W, bx, by, out, words);
    return sw_check(hipGetLastError(), "jpeg_decode pixels launch");
}
