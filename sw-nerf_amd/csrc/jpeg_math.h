// jpeg_math.h - the arithmetic of a baseline JPEG decode after the entropy stage, written once for the device kernels
// (jpeg_kernels.hip) and for plain host C++ (g++ compiles this header; the host test decodes whole files by looping these
// functions).  Every stage is the integer arithmetic of libjpeg's default decode (DESIGN.md 6k "JPEG"), so the pixels equal
// imageio.imread's byte for byte:
//   dequantise    coef * q
//   inverse DCT   the "islow" form: 13-bit constants, columns first descaled by 11 bits, then rows descaled by 18, + 128, clamp
//   up-sampling   the "fancy" triangle filter for 2:1 horizontal and 2:1 both ways; plain replication when the chroma plane is
//                 at most 2 samples wide
//   colour        the 16-bit fixed-point YCbCr -> RGB
// Products and sums are formed as uint32_t and shifted as int32_t: a crafted file gives defined, if meaningless, pixels;
// nothing wraps for a file a conforming encoder writes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ __forceinline__
#else
#define JPEG_HD static inline
#endif

#define JPEG_444 0       // luma sampled 1 x 1 (also: a single component)
#define JPEG_422 1       // luma 2 x 1: chroma has half the columns
#define JPEG_420 2       // luma 2 x 2: chroma has half the columns and half the rows

JPEG_HD int32_t jpeg_mul(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }
JPEG_HD int32_t jpeg_add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
JPEG_HD int32_t jpeg_sub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
JPEG_HD int32_t jpeg_shl13(int32_t a) { return (int32_t)((uint32_t)a << 13); }
JPEG_HD int32_t jpeg_descale(int32_t x, int n) { return jpeg_add(x, (int32_t)1 << (n - 1)) >> n; }
JPEG_HD int jpeg_clamp255(int32_t x) { return x < 0 ? 0 : (x > 255 ? 255 : (int)x); }

// one 1-D pass over i[0..7] -> o[0..7], each output descaled by `shift` bits
JPEG_HD void jpeg_idct_1d(const int32_t* i, int32_t* o, int shift) {
    int32_t z1 = jpeg_mul(jpeg_add(i[2], i[6]), 4433);
    const int32_t t2 = jpeg_sub(z1, jpeg_mul(i[6], 15137)), t3 = jpeg_add(z1, jpeg_mul(i[2], 6270));
    const int32_t t0 = jpeg_shl13(jpeg_add(i[0], i[4])), t1 = jpeg_shl13(jpeg_sub(i[0], i[4]));
    const int32_t t10 = jpeg_add(t0, t3), t13 = jpeg_sub(t0, t3), t11 = jpeg_add(t1, t2), t12 = jpeg_sub(t1, t2);
    int32_t o0 = i[7], o1 = i[5], o2 = i[3], o3 = i[1];
    z1 = jpeg_add(o0, o3);
    int32_t z2 = jpeg_add(o1, o2), z3 = jpeg_add(o0, o2), z4 = jpeg_add(o1, o3);
    const int32_t z5 = jpeg_mul(jpeg_add(z3, z4), 9633);
    o0 = jpeg_mul(o0, 2446);
    o1 = jpeg_mul(o1, 16819);
    o2 = jpeg_mul(o2, 25172);
    o3 = jpeg_mul(o3, 12299);
    z1 = jpeg_mul(z1, -7373);
    z2 = jpeg_mul(z2, -20995);
    z3 = jpeg_add(jpeg_mul(z3, -16069), z5);
    z4 = jpeg_add(jpeg_mul(z4, -3196), z5);
    o0 = jpeg_add(o0, jpeg_add(z1, z3));
    o1 = jpeg_add(o1, jpeg_add(z2, z4));
    o2 = jpeg_add(o2, jpeg_add(z2, z3));
    o3 = jpeg_add(o3, jpeg_add(z1, z4));
    o[0] = jpeg_descale(jpeg_add(t10, o3), shift);
    o[1] = jpeg_descale(jpeg_add(t11, o2), shift);
    o[2] = jpeg_descale(jpeg_add(t12, o1), shift);
    o[3] = jpeg_descale(jpeg_add(t13, o0), shift);
    o[4] = jpeg_descale(jpeg_sub(t13, o0), shift);
    o[5] = jpeg_descale(jpeg_sub(t12, o1), shift);
    o[6] = jpeg_descale(jpeg_sub(t11, o2), shift);
    o[7] = jpeg_descale(jpeg_sub(t10, o3), shift);
}

// v[64]: the dequantised coefficients of one block, natural order (row u, column v at 8 u + v) -> the 64 samples 0..255 in
// place.  Every index is a compile-time constant once the loops are unrolled, so on the device v stays in registers.
JPEG_HD void jpeg_idct_block(int32_t* v) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        int32_t in[8], out[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = v[8 * r + c];
        jpeg_idct_1d(in, out, 11);
#pragma unroll
        for (int r = 0; r < 8; ++r) v[8 * r + c] = out[r];
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        int32_t out[8];
        jpeg_idct_1d(v + 8 * r, out, 18);
#pragma unroll
        for (int c = 0; c < 8; ++c) v[8 * r + c] = jpeg_clamp255(jpeg_add(out[c], 128));
    }
}

// 2:1 horizontal: output column x of a chroma row of dw samples
JPEG_HD int jpeg_up_h2v1(const uint8_t* row, int dw, int x) {
    const int i = x >> 1;
    if (dw <= 2) return row[i];
    if (x & 1) return i == dw - 1 ? row[i] : (3 * row[i] + row[i + 1] + 2) >> 2;
    return i == 0 ? row[i] : (3 * row[i] + row[i - 1] + 1) >> 2;
}

// 2:1 both ways: near = the chroma row y >> 1, far = the row above it for an even output row y and the row below it for an odd
// one (the caller passes `near` again at the top and bottom edges); output column x
JPEG_HD int jpeg_up_h2v2(const uint8_t* near, const uint8_t* far, int dw, int x) {
    const int i = x >> 1;
    if (dw <= 2) return near[i];
    const int s = 3 * near[i] + far[i];
    if (x & 1) return i == dw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * near[i + 1] + far[i + 1] + 7) >> 4;
    return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
}

// the chroma row that goes with `near` for output row y of a plane of dh rows (JPEG_420)
JPEG_HD int jpeg_far_row(int y, int dh) {
    const int r = y >> 1;
    if (y & 1) return r == dh - 1 ? r : r + 1;
    return r == 0 ? r : r - 1;
}

JPEG_HD void jpeg_ycc_to_rgb(int y, int cb, int cr, int* r, int* g, int* b) {
    cb -= 128;
    cr -= 128;
    *r = jpeg_clamp255(y + ((91881 * cr + 32768) >> 16));
    *g = jpeg_clamp255(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    *b = jpeg_clamp255(y + ((116130 * cb + 32768) >> 16));
}

// geometry of the coefficient planes: component 0 has bx[0] x by[0] blocks, the chroma components bx[1] x by[1]; both are padded
// to whole MCUs.  -> blocks of one image over all components
JPEG_HD int64_t jpeg_blocks(int64_t H, int64_t W, int ncomp, int sampling, int* bx, int* by) {
    const int hs = (ncomp == 3 && sampling != JPEG_444) ? 2 : 1, vs = (ncomp == 3 && sampling == JPEG_420) ? 2 : 1;
    const int mx = (int)((W + 8 * hs - 1) / (8 * hs)), my = (int)((H + 8 * vs - 1) / (8 * vs));
    bx[0] = mx * hs;
    by[0] = my * vs;
    bx[1] = mx;
    by[1] = my;
    return (int64_t)bx[0] * by[0] + (ncomp == 3 ? 2 * (int64_t)bx[1] * by[1] : 0);
}
