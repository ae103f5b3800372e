// jpeg_enc_kernels.hip - baseline JPEG frames of the render videos (the reference's imageio.mimwrite of to8b(rgbs)): the device
// does what is parallel, with libjpeg's default integer arithmetic (jpeg_enc_math.h), the host writes the markers and the
// Huffman stream (jpeg_enc_host.h, no GPU call), so the file equals libjpeg's byte for byte.  DESIGN.md 6k "JPEG encode".
// swnerf_jpeg_encode is two launches on the caller's stream, no atomics, no host synchronisation - the decoder run backwards:
//   jpeg_planes_kernel  one lane per 4 horizontal samples of a padded component plane: to8b, colour conversion, chroma
//                       down-sampling and edge replication (source rows and columns clamped to the frame), one 4-byte store.
//                       The planes have the geometry of the decoder's scratch_planes.
//   jpeg_fdct_kernel    one lane per 8 x 8 block: eight 8-byte row loads, the 64 values stay in registers through both 1-D passes
//                       (every index is a compile-time constant), quantisation by integer division, eight 16-byte stores of
//                       int16 coefficients in natural order; neighbouring lanes hold neighbouring blocks.  A block wholly outside
//                       the component's real blocks is not transformed: its lane sums the block whose DC it repeats (the DC of a
//                       block is the plain sum of its centred samples) and stores zeros behind it.  No LDS.
// The bodies of both kernels are the lane functions of jpeg_enc_math.h, which plain g++ compiles too.
// All element offsets are 64-bit; above JPEG_MAX_BLOCKS workgroups a kernel strides over its work.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/swnerf.h"
#include "host_util.h"
#include "jpeg_enc_host.h"
#include "jpeg_enc_math.h"

#define JPEG_THREADS 256
#define JPEG_MAX_BLOCKS (1 << 20)

// ---- to8b + colour + down-sampling + edges --------------------------------------------------------------------------------
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_planes_kernel(const void* __restrict__ frames, int src_u8, int cin, float divisor, int64_t n,
                                                                   int H, int W, int ncomp, int sampling, int bx0, int by0, int bx1, int by1,
                                                                   uint8_t* __restrict__ planes) {
    const int64_t B0 = (int64_t)bx0 * by0, B1 = (int64_t)bx1 * by1, B = B0 + (ncomp == 3 ? 2 * B1 : 0);
    const int64_t total = n * B * 16;                                           // quads of samples: 64 / 4 per block
    for (int64_t t = (int64_t)blockIdx.x * JPEG_THREADS + threadIdx.x; t < total; t += (int64_t)gridDim.x * JPEG_THREADS)
        jpeg_enc_planes_lane(t, frames, src_u8, cin, divisor, H, W, ncomp, sampling, bx0, by0, bx1, by1, planes);
}

// ---- forward DCT + quantise ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_fdct_kernel(const uint8_t* __restrict__ planes, const uint16_t* __restrict__ qt, int64_t n, int H, int W,
                                                                 int ncomp, int bx0, int by0, int bx1, int by1, int16_t* __restrict__ coef) {
    const int64_t B0 = (int64_t)bx0 * by0, B1 = (int64_t)bx1 * by1, B = B0 + (ncomp == 3 ? 2 * B1 : 0);
    const int64_t total = n * B;
    for (int64_t g = (int64_t)blockIdx.x * JPEG_THREADS + threadIdx.x; g < total; g += (int64_t)gridDim.x * JPEG_THREADS)
        jpeg_enc_fdct_lane(g, planes, qt, H, W, ncomp, bx0, by0, bx1, by1, coef);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static unsigned jpeg_enc_grid(int64_t items) {
    const int64_t b = (items + JPEG_THREADS - 1) / JPEG_THREADS;
    return (unsigned)(b < 1 ? 1 : (b > JPEG_MAX_BLOCKS ? JPEG_MAX_BLOCKS : b));
}

static int jpeg_enc_check_geometry(const char* who, int64_t H, int64_t W, int ncomp, int sampling) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535) return sw_fail(SWNERF_E_ARG, "%s: image size %lld x %lld outside 1..65535", who, (long long)H, (long long)W);
    if (ncomp != 1 && ncomp != 3) return sw_fail(SWNERF_E_ARG, "%s: %d components; 1 and 3 are built", who, ncomp);
    if (sampling != JPEG_444 && sampling != JPEG_422 && sampling != JPEG_420) return sw_fail(SWNERF_E_ARG, "%s: sampling %d is none of SWNERF_JPEG_444 / 422 / 420", who, sampling);
    if (ncomp == 1 && sampling != JPEG_444) return sw_fail(SWNERF_E_ARG, "%s: a single component is SWNERF_JPEG_444", who);
    return 0;
}

extern "C" int swnerf_jpeg_quant_tables(int quality, uint16_t* qt) {
    if (!qt) return sw_fail(SWNERF_E_ARG, "jpeg_quant_tables: NULL pointer");
    jpeg_quant_tables(quality, qt);
    return 0;
}

extern "C" int64_t swnerf_jpeg_file_bound(int64_t H, int64_t W, int ncomp, int sampling) {
    if (jpeg_enc_check_geometry("jpeg_file_bound", H, W, ncomp, sampling)) return 0;
    return jpeg_enc_file_bound(H, W, ncomp, sampling);
}

extern "C" int64_t swnerf_jpeg_write(const int16_t* coef, int64_t coef_count, const uint16_t* qt, int64_t H, int64_t W, int ncomp, int sampling,
                                     uint8_t* out, int64_t cap) {
    const int rc = jpeg_enc_check_geometry("jpeg_write", H, W, ncomp, sampling);
    if (rc) return rc;
    if (!coef || !qt || cap < 0 || (!out && cap > 0)) return sw_fail(SWNERF_E_ARG, "jpeg_write: NULL pointer or negative capacity");
    int bx[2], by[2];
    const int64_t want = 64 * jpeg_blocks(H, W, ncomp, sampling, bx, by);
    if (coef_count != want) return sw_fail(SWNERF_E_ARG, "jpeg_write: the geometry has %lld coefficients, the buffer %lld", (long long)want, (long long)coef_count);
    for (int k = 0; k < (ncomp == 3 ? 128 : 64); ++k)
        if (qt[k] < 1 || qt[k] > 255) return sw_fail(SWNERF_E_ARG, "jpeg_write: quantisation table entry %d is %d, outside 1..255 (baseline tables are 8-bit)", k, (int)qt[k]);
    const int64_t got = jpeg_enc_write(coef, qt, (int)H, (int)W, ncomp, sampling, out, cap);
    if (got == JPEG_ENC_SHORT) return sw_fail(SWNERF_E_ARG, "jpeg_write: the file does not fit into %lld bytes (jpeg_file_bound gives %lld)", (long long)cap, (long long)jpeg_enc_file_bound(H, W, ncomp, sampling));
    if (got == JPEG_ENC_RANGE) return sw_fail(SWNERF_E_DATA, "jpeg_write: a coefficient outside what baseline Huffman codes express (DC difference above 11 bits or AC above 10)");
    return got;
}

extern "C" int swnerf_jpeg_encode(const void* frames, int src_u8, int64_t n, int64_t H, int64_t W, int channels_in, float divisor, const uint16_t* qt,
                                  int ncomp, int sampling, uint8_t* scratch_planes, int16_t* coef, void* stream) {
    int rc = jpeg_enc_check_geometry("jpeg_encode", H, W, ncomp, sampling);
    if (rc) return rc;
    if (n < 0) return sw_fail(SWNERF_E_ARG, "jpeg_encode: negative frame count %lld", (long long)n);
    if (channels_in != 1 && channels_in != 3 && channels_in != 4) return sw_fail(SWNERF_E_ARG, "jpeg_encode: %d input channels; 1, 3 and 4 (alpha ignored) are built", channels_in);
    if (ncomp == 1 && channels_in != 1) return sw_fail(SWNERF_E_ARG, "jpeg_encode: a single component needs 1 input channel, got %d", channels_in);
    if (n == 0) return 0;
    if (!frames || !qt || !scratch_planes || !coef) return sw_fail(SWNERF_E_ARG, "jpeg_encode: NULL pointer");
    if (((uintptr_t)coef & 15) || ((uintptr_t)qt & 15) || ((uintptr_t)scratch_planes & 7) || (!src_u8 && ((uintptr_t)frames & 3)))
        return sw_fail(SWNERF_E_ARG, "jpeg_encode: coef and qt must be 16-byte aligned, scratch_planes 8-byte aligned, float frames 4-byte aligned");
    int bx[2], by[2];
    const int64_t B = jpeg_blocks(H, W, ncomp, sampling, bx, by);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_planes_kernel, dim3(jpeg_enc_grid(n * B * 16)), dim3(JPEG_THREADS), 0, st, frames, src_u8 != 0, channels_in, divisor, n, (int)H, (int)W,
                       ncomp, sampling, bx[0], by[0], bx[1], by[1], scratch_planes);
    rc = sw_check(hipGetLastError(), "jpeg_encode planes launch");
    if (rc) return rc;
    hipLaunchKernelGGL(jpeg_fdct_kernel, dim3(jpeg_enc_grid(n * B)), dim3(JPEG_THREADS), 0, st, (const uint8_t*)scratch_planes, qt, n, (int)H, (int)W, ncomp, bx[0],
                       by[0], bx[1], by[1], coef);
    return sw_check(hipGetLastError(), "jpeg_encode fdct launch");
}
