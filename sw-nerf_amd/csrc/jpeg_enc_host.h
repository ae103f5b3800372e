// jpeg_enc_host.h - the serial half of the JPEG encode, plain C++ with no GPU call and no global state (calls from several
// threads are independent): libjpeg's quality scaling of the Annex K quantisation tables, an upper bound on a file's size, and
// the writer of a baseline JFIF file - markers and the Huffman-coded interleaved scan with the Annex K.3 "typical" tables - from
// int16 coefficient planes in the layout jpeg_entropy() of jpeg_host.h produces.  The bytes are what libjpeg emits by default
// (no restart markers, no optimised tables, no progressive mode).  g++ compiles this header as it is; the library reaches it
// through swnerf_jpeg_quant_tables / swnerf_jpeg_file_bound / swnerf_jpeg_write.
#pragma once
#include "jpeg_host.h"

#define JPEG_ENC_SHORT (-1)              // `cap` bytes do not hold the file
#define JPEG_ENC_RANGE (-2)              // a coefficient no baseline code expresses (DC difference above 11 bits, AC above 10)

// Annex K.1 / K.2, natural order
static const uint8_t jpeg_base_qt[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// Annex K.3: [0] luminance, [1] chrominance; counts of codes of length 1..16, then the symbols in code order
static const uint8_t jpeg_std_dc_counts[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static const uint8_t jpeg_std_dc_symbols[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t jpeg_std_ac_counts[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
static const uint8_t jpeg_std_ac_symbols[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

// qt: [2][64] natural order, luma then chroma: jpeg_set_quality(quality, force_baseline = TRUE)
static inline void jpeg_quant_tables(int quality, uint16_t* qt) {
    quality = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) {
            const int v = (jpeg_base_qt[t][k] * scale + 50) / 100;
            qt[64 * t + k] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
}

// bytes of everything but the entropy-coded segment: SOI 2, APP0 18, DQT 69 per table, SOF0 10 + 3 per component, DHT 33 (DC) and
// 183 (AC) per table pair, SOS 8 + 2 per component, EOI 2
static inline int64_t jpeg_enc_header_bytes(int ncomp) {
    const int tables = ncomp == 3 ? 2 : 1;
    return 2 + 18 + 69 * tables + (10 + 3 * ncomp) + (33 + 183) * tables + (8 + 2 * ncomp) + 2;
}

// An upper bound on the file jpeg_enc_write() makes of this geometry, whatever the coefficients.  Each of a block's 64
// coefficients costs at most 26 bits: a non-zero AC one a code of at most 16 bits and at most 10 value bits; the DC difference a
// code of at most 11 bits and at most 11 value bits; a zero AC coefficient nothing by itself - the ZRL that stands for 16 of them
// has at most 11 bits, the EOB that stands for at least one at most 4.  So a block has at most 64 * 26 bits = 208 bytes; every
// byte of the segment may be 0xFF and is then followed by a stuffed 0x00 (x 2); the final partial byte, padded with 1-bits, may
// be stuffed as well (+ 2).
static inline int64_t jpeg_enc_file_bound(int64_t H, int64_t W, int ncomp, int sampling) {
    int bx[2], by[2];
    return jpeg_enc_header_bytes(ncomp) + 2 * 208 * jpeg_blocks(H, W, ncomp, sampling, bx, by) + 2;
}

struct jpeg_enc_codes {
    uint16_t code[256];
    uint8_t len[256];                    // 0: the table assigns the symbol no code
};

static inline void jpeg_enc_build_codes(const uint8_t* counts, const uint8_t* symbols, jpeg_enc_codes* t) {
    memset(t, 0, sizeof(*t));
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int j = 0; j < counts[l - 1]; ++j, ++k, ++code) {
            t->code[symbols[k]] = (uint16_t)code;
            t->len[symbols[k]] = (uint8_t)l;
        }
        code <<= 1;
    }
}

struct jpeg_enc_out {
    uint8_t* d;
    int64_t p, cap;
    uint64_t acc;                        // the low `n` bits wait to be written, oldest on top
    int n, over;
};

static inline void jpeg_enc_byte(jpeg_enc_out* o, int b) {
    if (o->p < o->cap) o->d[o->p++] = (uint8_t)b;
    else o->over = 1;
}

static inline void jpeg_enc_word(jpeg_enc_out* o, int w) {
    jpeg_enc_byte(o, (w >> 8) & 255);
    jpeg_enc_byte(o, w & 255);
}

// `len` (1..26) bits of `bits`
static inline void jpeg_enc_bits(jpeg_enc_out* o, uint32_t bits, int len) {
    o->acc = (o->acc << len) | (uint64_t)(bits & ((1u << len) - 1));
    o->n += len;
    while (o->n >= 8) {
        const int b = (int)((o->acc >> (o->n - 8)) & 255);
        jpeg_enc_byte(o, b);
        if (b == 0xFF) jpeg_enc_byte(o, 0);
        o->n -= 8;
    }
}

static inline int jpeg_enc_nbits(int v) {
    int n = 0;
    for (v = v < 0 ? -v : v; v; v >>= 1) ++n;
    return n;
}

// one block: the DC difference to `*pred`, then the AC run lengths in zigzag order.  -> 0 or JPEG_ENC_RANGE
static inline int jpeg_enc_block(jpeg_enc_out* o, const int16_t* blk, int* pred, const jpeg_enc_codes* dc, const jpeg_enc_codes* ac) {
    const int diff = (int)blk[0] - *pred;
    *pred = blk[0];
    int s = jpeg_enc_nbits(diff);
    if (s > 11) return JPEG_ENC_RANGE;
    jpeg_enc_bits(o, dc->code[s], dc->len[s]);
    if (s) jpeg_enc_bits(o, (uint32_t)(diff < 0 ? diff - 1 : diff), s);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = blk[jpeg_natural_order[k]];
        if (v == 0) {
            ++run;
            continue;
        }
        for (; run > 15; run -= 16) jpeg_enc_bits(o, ac->code[0xF0], ac->len[0xF0]);
        s = jpeg_enc_nbits(v);
        if (s > 10) return JPEG_ENC_RANGE;
        jpeg_enc_bits(o, ac->code[(run << 4) | s], ac->len[(run << 4) | s]);
        jpeg_enc_bits(o, (uint32_t)(v < 0 ? v - 1 : v), s);
        run = 0;
    }
    if (run) jpeg_enc_bits(o, ac->code[0], ac->len[0]);
    return 0;
}

// coef: jpeg_blocks() * 64 int16 (the layout of jpeg_entropy), qt: [2][64] natural order, entries 1..255 (the chroma table is read
// only for 3 components).  -> the bytes written into out[0..cap), JPEG_ENC_SHORT (out then holds a cut file) or JPEG_ENC_RANGE.
// The caller has checked the geometry (H, W in 1..65535; 1 component at JPEG_444, or 3).
static inline int64_t jpeg_enc_write(const int16_t* coef, const uint16_t* qt, int H, int W, int ncomp, int sampling, uint8_t* out, int64_t cap) {
    int bx[2], by[2];
    jpeg_blocks(H, W, ncomp, sampling, bx, by);
    const int hs = bx[0] / bx[1], vs = by[0] / by[1], tables = ncomp == 3 ? 2 : 1;
    jpeg_enc_out o = {out, 0, cap, 0, 0, 0};
    jpeg_enc_word(&o, 0xFFD8);
    jpeg_enc_word(&o, 0xFFE0);
    jpeg_enc_word(&o, 16);
    static const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (int k = 0; k < 14; ++k) jpeg_enc_byte(&o, jfif[k]);
    for (int t = 0; t < tables; ++t) {
        jpeg_enc_word(&o, 0xFFDB);
        jpeg_enc_word(&o, 67);
        jpeg_enc_byte(&o, t);
        for (int k = 0; k < 64; ++k) jpeg_enc_byte(&o, qt[64 * t + jpeg_natural_order[k]] & 255);
    }
    jpeg_enc_word(&o, 0xFFC0);
    jpeg_enc_word(&o, 8 + 3 * ncomp);
    jpeg_enc_byte(&o, 8);
    jpeg_enc_word(&o, H);
    jpeg_enc_word(&o, W);
    jpeg_enc_byte(&o, ncomp);
    for (int c = 0; c < ncomp; ++c) {
        jpeg_enc_byte(&o, c + 1);
        jpeg_enc_byte(&o, c ? 0x11 : (hs << 4 | vs));
        jpeg_enc_byte(&o, c ? 1 : 0);
    }
    jpeg_enc_codes dc[2], ac[2];
    for (int t = 0; t < tables; ++t) {
        jpeg_enc_build_codes(jpeg_std_dc_counts[t], jpeg_std_dc_symbols, &dc[t]);
        jpeg_enc_build_codes(jpeg_std_ac_counts[t], jpeg_std_ac_symbols[t], &ac[t]);
        jpeg_enc_word(&o, 0xFFC4);
        jpeg_enc_word(&o, 2 + 1 + 16 + 12);
        jpeg_enc_byte(&o, t);
        for (int k = 0; k < 16; ++k) jpeg_enc_byte(&o, jpeg_std_dc_counts[t][k]);
        for (int k = 0; k < 12; ++k) jpeg_enc_byte(&o, jpeg_std_dc_symbols[k]);
        jpeg_enc_word(&o, 0xFFC4);
        jpeg_enc_word(&o, 2 + 1 + 16 + 162);
        jpeg_enc_byte(&o, 0x10 | t);
        for (int k = 0; k < 16; ++k) jpeg_enc_byte(&o, jpeg_std_ac_counts[t][k]);
        for (int k = 0; k < 162; ++k) jpeg_enc_byte(&o, jpeg_std_ac_symbols[t][k]);
    }
    jpeg_enc_word(&o, 0xFFDA);
    jpeg_enc_word(&o, 6 + 2 * ncomp);
    jpeg_enc_byte(&o, ncomp);
    for (int c = 0; c < ncomp; ++c) {
        jpeg_enc_byte(&o, c + 1);
        jpeg_enc_byte(&o, c ? 0x11 : 0x00);
    }
    jpeg_enc_byte(&o, 0);
    jpeg_enc_byte(&o, 63);
    jpeg_enc_byte(&o, 0);
    const int16_t* plane[3] = {coef, coef + (int64_t)bx[0] * by[0] * 64, coef + ((int64_t)bx[0] * by[0] + (int64_t)bx[1] * by[1]) * 64};
    int pred[3] = {0, 0, 0};
    for (int my = 0; my < by[1] && !o.over; ++my)
        for (int mx = 0; mx < bx[1]; ++mx)
            for (int c = 0; c < ncomp; ++c) {
                const int nh = c ? 1 : hs, nv = c ? 1 : vs, pbx = c ? bx[1] : bx[0];
                for (int v = 0; v < nv; ++v)
                    for (int h = 0; h < nh; ++h)
                        if (jpeg_enc_block(&o, plane[c] + ((int64_t)(my * nv + v) * pbx + (mx * nh + h)) * 64, &pred[c], &dc[c ? 1 : 0], &ac[c ? 1 : 0]))
                            return JPEG_ENC_RANGE;
            }
    if (o.n) jpeg_enc_bits(&o, 0x7F, 8 - o.n);                                 // the last partial byte is padded with 1-bits
    jpeg_enc_word(&o, 0xFFD9);
    return o.over ? JPEG_ENC_SHORT : o.p;
}
