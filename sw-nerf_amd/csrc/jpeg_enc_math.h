// jpeg_enc_math.h - the arithmetic of a baseline JPEG encode before the entropy stage, written once for the device kernels
// (jpeg_enc_kernels.hip) and for plain host C++ (g++ compiles this header; the host test encodes whole frames by looping these
// functions).  Every stage is the integer arithmetic of libjpeg's default encoder (DESIGN.md 6k "JPEG encode"), so the
// coefficients - and with jpeg_enc_host.h the file - equal what libjpeg writes for the same pixels, quality and sampling:
//   to8b          (uint8)(255.0f * clamp(x [/ divisor], 0, 1)), truncated; NaN gives 0; bytes pass through
//   colour        the 16-bit fixed-point RGB -> YCbCr of jccolor
//   down-sampling jcsample without smoothing: 2:1 horizontal (a + b + bias) >> 1, 2:1 both ways (a + b + c + d + bias) >> 2, the
//                 bias alternating with the output column; columns are replicated at full resolution BEFORE the averaging, rows
//                 only up to a multiple of the vertical factor; the rest of a plane's padded rows repeat its last row AFTER it
//   forward DCT   jfdctint ("islow"): 13-bit constants, rows first (scaled up by 2 bits), then columns (descaled by 2 + 13 bits)
//   quantise      jcdctmgr: sign(c) * ((|c| + (8 q >> 1)) / (8 q)), truncating division
//   dummy blocks  jccoefct: a block wholly outside the component's real blocks is not transformed - all AC 0, the DC of the block
//                 it continues
// jpeg_enc_planes_lane / jpeg_enc_fdct_lane at the end are the whole bodies of the two kernels, index arithmetic, loads and
// stores included: the host test runs them over buffers that end where the data ends.
#pragma once
#include "jpeg_math.h"

// one sample of the render as a byte
JPEG_HD int jpeg_to8b(float x, float divisor) {
    if (divisor != 0.0f) {
#if defined(__HIP_DEVICE_COMPILE__)
        x = __fdiv_rn(x, divisor);                                              // correctly rounded, as numpy's x / divisor
#else
        x = x / divisor;
#endif
    }
    const float c = x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f;                    // a NaN fails the first comparison: 0
    return (int)(255.0f * c);
}

// R, G, B of pixel `p` (an index over n * H * W) of frames with `cin` channels (1: R = G = B; 3; 4: alpha ignored)
JPEG_HD void jpeg_enc_pixel(const void* frames, int src_u8, int cin, int64_t p, float divisor, int* r, int* g, int* b) {
    if (src_u8) {
        const uint8_t* s = (const uint8_t*)frames + p * cin;
        *r = s[0];
        *g = cin == 1 ? s[0] : s[1];
        *b = cin == 1 ? s[0] : s[2];
    } else {
        const float* s = (const float*)frames + p * cin;
        *r = jpeg_to8b(s[0], divisor);
        *g = cin == 1 ? *r : jpeg_to8b(s[1], divisor);
        *b = cin == 1 ? *r : jpeg_to8b(s[2], divisor);
    }
}

// component `comp` (0 Y, 1 Cb, 2 Cr) of an RGB triple
JPEG_HD int jpeg_rgb_to_ycc(int r, int g, int b, int comp) {
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16;
}

// The sample at row y, column x of the PADDED plane of component `comp` of image `img`.  ncomp == 1 stores the (single) input
// channel as Y.  Source rows and columns are clamped to the image, which is the replication of libjpeg's edge expansion: a
// 4:2:0 chroma row past the last one repeats the last DOWN-SAMPLED row (whose second source row is row H - 1 again when H is odd).
JPEG_HD int jpeg_enc_plane_sample(const void* frames, int src_u8, int cin, float divisor, int64_t img, int H, int W, int ncomp, int sampling,
                                  int comp, int y, int x) {
    const int64_t base = img * H * (int64_t)W;
    int r, g, b;
    if (comp == 0 || sampling == JPEG_444) {
        const int sy = y < H ? y : H - 1, sx = x < W ? x : W - 1;
        jpeg_enc_pixel(frames, src_u8, cin, base + (int64_t)sy * W + sx, divisor, &r, &g, &b);
        return ncomp == 1 ? r : jpeg_rgb_to_ycc(r, g, b, comp);
    }
    const int x0 = 2 * x < W ? 2 * x : W - 1, x1 = 2 * x + 1 < W ? 2 * x + 1 : W - 1;
    if (sampling == JPEG_422) {
        const int sy = y < H ? y : H - 1;
        jpeg_enc_pixel(frames, src_u8, cin, base + (int64_t)sy * W + x0, divisor, &r, &g, &b);
        int s = jpeg_rgb_to_ycc(r, g, b, comp);
        jpeg_enc_pixel(frames, src_u8, cin, base + (int64_t)sy * W + x1, divisor, &r, &g, &b);
        s += jpeg_rgb_to_ycc(r, g, b, comp);
        return (s + (x & 1)) >> 1;
    }
    const int ch = (H + 1) >> 1, cy = y < ch ? y : ch - 1;
    const int y0 = 2 * cy, y1 = 2 * cy + 1 < H ? 2 * cy + 1 : H - 1;
    int s = 0;
    jpeg_enc_pixel(frames, src_u8, cin, base + (int64_t)y0 * W + x0, divisor, &r, &g, &b);
    s += jpeg_rgb_to_ycc(r, g, b, comp);
    jpeg_enc_pixel(frames, src_u8, cin, base + (int64_t)y0 * W + x1, divisor, &r, &g, &b);
    s += jpeg_rgb_to_ycc(r, g, b, comp);
    jpeg_enc_pixel(frames, src_u8, cin, base + (int64_t)y1 * W + x0, divisor, &r, &g, &b);
    s += jpeg_rgb_to_ycc(r, g, b, comp);
    jpeg_enc_pixel(frames, src_u8, cin, base + (int64_t)y1 * W + x1, divisor, &r, &g, &b);
    s += jpeg_rgb_to_ycc(r, g, b, comp);
    return (s + 1 + (x & 1)) >> 2;
}

// one 1-D pass over d[0..7] in place.  ROWS: out0 / out4 scaled up by 2 bits and the rest descaled by 11; otherwise (columns)
// out0 / out4 descaled by 2 and the rest by 15.
template <bool ROWS>
JPEG_HD void jpeg_fdct_1d(int32_t* d) {
    const int s = ROWS ? 11 : 15;
    const int32_t t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int32_t t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = ROWS ? (int32_t)((uint32_t)(t10 + t11) << 2) : jpeg_descale(t10 + t11, 2);
    d[4] = ROWS ? (int32_t)((uint32_t)(t10 - t11) << 2) : jpeg_descale(t10 - t11, 2);
    int32_t z1 = (t12 + t13) * 4433;
    d[2] = jpeg_descale(z1 + t13 * 6270, s);
    d[6] = jpeg_descale(z1 - t12 * 15137, s);
    z1 = t4 + t7;
    int32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int32_t z5 = (z3 + z4) * 9633;
    const int32_t m4 = t4 * 2446, m5 = t5 * 16819, m6 = t6 * 25172, m7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7] = jpeg_descale(m4 + z1 + z3, s);
    d[5] = jpeg_descale(m5 + z2 + z4, s);
    d[3] = jpeg_descale(m6 + z2 + z3, s);
    d[1] = jpeg_descale(m7 + z1 + z4, s);
}

// v[64]: the samples 0..255 of one block, row-major -> its coefficients (8 x the true DCT) in natural order, in place.  Every
// index is a compile-time constant once the loops are unrolled, so on the device v stays in registers.  Nothing overflows:
// |v - 128| <= 128 keeps every intermediate below 2^29.
JPEG_HD void jpeg_fdct_block(int32_t* v) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
#pragma unroll
        for (int c = 0; c < 8; ++c) v[8 * r + c] -= 128;
        jpeg_fdct_1d<true>(v + 8 * r);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        int32_t col[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) col[r] = v[8 * r + c];
        jpeg_fdct_1d<false>(col);
#pragma unroll
        for (int r = 0; r < 8; ++r) v[8 * r + c] = col[r];
    }
}

// q: the table entry 1..255 (0 is taken for 1: nothing divides by zero)
JPEG_HD int32_t jpeg_quantise(int32_t c, int32_t q) {
    const int32_t d = 8 * (q > 0 ? q : 1), a = c < 0 ? -c : c, r = (a + (d >> 1)) / d;
    return c < 0 ? -r : r;
}

// Where block (byi, bxi) of a padded plane of pbx blocks per row takes its samples from: itself when it is one of the rbx x rby
// real blocks (-> 1), otherwise (-> 0) the real block whose quantised DC it repeats: the last real block of its row; for a row
// below the last real one, the block above it in the right-hand column of its MCU (hs blocks wide), or the last real block of
// that row when that column is itself outside.
JPEG_HD int jpeg_enc_source_block(int byi, int bxi, int rby, int rbx, int hs, int* sy, int* sx) {
    *sy = byi;
    *sx = bxi;
    if (byi < rby && bxi < rbx) return 1;
    if (byi >= rby) {
        *sy = rby - 1;
        *sx = bxi / hs * hs + hs - 1;
    }
    if (*sx >= rbx) *sx = rbx - 1;
    return 0;
}

// 8- and 16-byte words of the lane functions below: the device's vector types, plain aligned structs for g++
#if defined(__HIPCC__)
typedef uint2 jpeg_w2;
typedef uint4 jpeg_w4;
#else
struct alignas(8) jpeg_w2 { uint32_t x, y; };
struct alignas(16) jpeg_w4 { uint32_t x, y, z, w; };
#endif

// Lane t of the planes kernel: 4 horizontal samples of a padded plane, t in [0, n * blocks * 16).  Reads `frames` inside the
// frame of image t / (blocks * 16) only; writes the 4 bytes at quad t of `planes`.
JPEG_HD void jpeg_enc_planes_lane(int64_t t, const void* __restrict__ frames, int src_u8, int cin, float divisor, int H, int W, int ncomp, int sampling, int bx0,
                                  int by0, int bx1, int by1, uint8_t* __restrict__ planes) {
    const int64_t B0 = (int64_t)bx0 * by0, B1 = (int64_t)bx1 * by1, B = B0 + (ncomp == 3 ? 2 * B1 : 0);
    const int64_t img = t / (B * 16);
    int64_t rem = t - img * B * 16;                                         // quad within the image: planes follow each other
    int comp = 0, pbx = bx0;
    int64_t plane_off = 0;
    if (rem >= B0 * 16) {
        comp = 1 + (int)((rem - B0 * 16) / (B1 * 16));
        plane_off = B0 + (comp - 1) * B1;
        rem -= plane_off * 16;
        pbx = bx1;
    }
    const int qrow = pbx * 2;                                               // quads of one plane row
    const int y = (int)(rem / qrow), x0 = (int)(rem - (int64_t)y * qrow) * 4;
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        w |= (uint32_t)jpeg_enc_plane_sample(frames, src_u8, cin, divisor, img, H, W, ncomp, sampling, comp, y, x0 + j) << (8 * j);
    *reinterpret_cast<uint32_t*>(planes + (img * B + plane_off) * 64 + (int64_t)y * (pbx * 8) + x0) = w;
}

// Lane g of the FDCT kernel: block g of [n][blocks].  Reads 64 bytes of `planes` inside the plane the block belongs to and the
// 128 bytes of its component's table; writes the 128 bytes of block g of `coef`.
JPEG_HD void jpeg_enc_fdct_lane(int64_t g, const uint8_t* __restrict__ planes, const uint16_t* __restrict__ qt, int H, int W, int ncomp, int bx0, int by0, int bx1, int by1,
                                int16_t* __restrict__ coef) {
    const int64_t B0 = (int64_t)bx0 * by0, B1 = (int64_t)bx1 * by1, B = B0 + (ncomp == 3 ? 2 * B1 : 0);
    const int hs = bx0 / bx1, vs = by0 / by1;
    const int64_t img = g / B;
    int64_t rem = g - img * B;
    int comp = 0, pbx = bx0, wc = W, hc = H, mcu_w = hs;
    int64_t plane_off = 0;
    if (rem >= B0) {
        comp = 1 + (int)((rem - B0) / B1);
        plane_off = B0 + (comp - 1) * B1;
        rem -= plane_off;
        pbx = bx1;
        wc = (W + hs - 1) / hs;
        hc = (H + vs - 1) / vs;
        mcu_w = 1;
    }
    const int byi = (int)(rem / pbx), bxi = (int)(rem - (int64_t)byi * pbx);
    int sy, sx;
    const int real = jpeg_enc_source_block(byi, bxi, (hc + 7) >> 3, (wc + 7) >> 3, mcu_w, &sy, &sx);
    const int64_t stride = (int64_t)pbx * 8;
    const uint8_t* P = planes + (img * B + plane_off) * 64 + (int64_t)sy * 8 * stride + (int64_t)sx * 8;
    int32_t v[64];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const jpeg_w2 w = *reinterpret_cast<const jpeg_w2*>(P + r * stride);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[8 * r + j] = (int32_t)((w.x >> (8 * j)) & 255u);
            v[8 * r + 4 + j] = (int32_t)((w.y >> (8 * j)) & 255u);
        }
    }
    const jpeg_w4* Q = reinterpret_cast<const jpeg_w4*>(qt + comp * 64);
    if (real) {
        jpeg_fdct_block(v);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const jpeg_w4 q = Q[k];
            const uint32_t qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[8 * k + 2 * j] = jpeg_quantise(v[8 * k + 2 * j], (int32_t)(qw[j] & 0xFFFFu));
                v[8 * k + 2 * j + 1] = jpeg_quantise(v[8 * k + 2 * j + 1], (int32_t)(qw[j] >> 16));
            }
        }
    } else {
        int32_t s = -8192;
#pragma unroll
        for (int k = 0; k < 64; ++k) {
            s += v[k];
            v[k] = 0;
        }
        v[0] = jpeg_quantise(s, (int32_t)(Q[0].x & 0xFFFFu));
    }
    jpeg_w4* C = reinterpret_cast<jpeg_w4*>(coef + g * 64);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        jpeg_w4 c;
        c.x = ((uint32_t)v[8 * k] & 0xFFFFu) | (uint32_t)v[8 * k + 1] << 16;
        c.y = ((uint32_t)v[8 * k + 2] & 0xFFFFu) | (uint32_t)v[8 * k + 3] << 16;
        c.z = ((uint32_t)v[8 * k + 4] & 0xFFFFu) | (uint32_t)v[8 * k + 5] << 16;
        c.w = ((uint32_t)v[8 * k + 6] & 0xFFFFu) | (uint32_t)v[8 * k + 7] << 16;
        C[k] = c;
    }
}
