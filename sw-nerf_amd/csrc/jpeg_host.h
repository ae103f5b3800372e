// jpeg_host.h - the serial half of the JPEG route, plain C++ with no GPU call: the marker parse and the Huffman decode of a
// baseline file into int16 coefficient planes (natural order, one [blocks_y][blocks_x][64] plane per component, padded to whole
// MCUs - jpeg_blocks() of jpeg_math.h).  The device does the rest (jpeg_kernels.hip).  g++ compiles this header as it is; the
// library reaches it through swnerf_jpeg_header / swnerf_jpeg_entropy.
//   JPEG_OK       0
//   JPEG_UNSUPP   "not decodable here": anything but 8-bit Huffman-coded, one interleaved scan, 1 component or 3 that libjpeg's
//                 rule takes for YCbCr, luma 1x1 / 2x1 / 2x2 with chroma 1x1 - and a header that cannot be read.  Not an error:
//                 the caller hands the file to another decoder.
//   JPEG_CORRUPT  the entropy segment of an accepted file is truncated, uses an unassigned code, runs a coefficient index past
//                 63 or lacks the RSTn it should have.  libjpeg's "pad with zeros and warn" is not copied.
// No read goes past data + len, no write outside the caller's buffer, and nothing is kept between calls: calls from several
// threads are independent.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "jpeg_math.h"

#define JPEG_OK 0
#define JPEG_UNSUPP 1
#define JPEG_CORRUPT 2
#define JPEG_FAST_BITS 9

static const uint8_t jpeg_natural_order[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct jpeg_huff {
    int defined;
    uint8_t counts[17];                  // codes of length 1..16
    uint8_t symbols[256];
    int32_t maxcode[18];                 // largest code of length l, -1 when there is none; [17] ends the search
    int32_t valoff[17];                  // symbols[code + valoff[l]]
    uint16_t fast[1 << JPEG_FAST_BITS];  // (length << 8) | symbol for codes of at most JPEG_FAST_BITS bits, 0 otherwise
};

struct jpeg_info {
    int H, W, ncomp, sampling, restart;
    int bx[2], by[2];                    // blocks of the luma plane and of one chroma plane
    int64_t blocks;                      // of all components: 64 coefficients each
    uint16_t qt[3][64];                  // per component, natural order
    int dc[3], ac[3];                    // table selectors of the scan
    int64_t scan;                        // offset of the first entropy-coded byte
    jpeg_huff huff[2][4];                // [0] DC, [1] AC
};

static inline int jpeg_say(char* err, size_t errlen, int code, const char* msg) {
    if (err && errlen) snprintf(err, errlen, "%s", msg);
    return code;
}

static inline int jpeg_build_huff(jpeg_huff* h) {
    int code = 0, k = 0;
    memset(h->fast, 0, sizeof(h->fast));
    for (int l = 1; l <= 16; ++l) {
        h->valoff[l] = k - code;
        if (h->counts[l]) {
            if (code + h->counts[l] > (1 << l)) return 0;                       // more codes than l bits hold
            for (int j = 0; j < h->counts[l]; ++j, ++k, ++code)
                if (l <= JPEG_FAST_BITS) {
                    const int first = code << (JPEG_FAST_BITS - l);
                    for (int f = 0; f < (1 << (JPEG_FAST_BITS - l)); ++f) h->fast[first + f] = (uint16_t)((l << 8) | h->symbols[k]);
                }
            h->maxcode[l] = code - 1;
        } else {
            h->maxcode[l] = -1;
        }
        code <<= 1;
    }
    h->maxcode[17] = 0x7fffffff;
    h->defined = 1;
    return 1;
}

// The header up to and including SOS.  JPEG_OK or JPEG_UNSUPP (err says why).
static inline int jpeg_parse(const uint8_t* d, int64_t len, jpeg_info* o, char* err, size_t errlen) {
#define JPEG_NO(msg) return jpeg_say(err, errlen, JPEG_UNSUPP, "not decodable here: " msg)
    if (!d || len < 4 || d[0] != 0xFF || d[1] != 0xD8) JPEG_NO("no SOI marker");
    uint16_t qtab[4][64];
    int have_q[4] = {0, 0, 0, 0}, comp_id[3] = {0, 0, 0}, comp_q[3] = {0, 0, 0}, comp_h[3] = {1, 1, 1}, comp_v[3] = {1, 1, 1};
    int jfif = 0, adobe = 0, transform = 0, sof = 0;
    memset(o, 0, sizeof(*o));
    int64_t p = 2;
    for (;;) {
        if (p >= len || d[p] != 0xFF) JPEG_NO("a marker is missing");
        while (p < len && d[p] == 0xFF) ++p;                                    // fill bytes
        if (p >= len) JPEG_NO("the header ends inside a marker");
        const int m = d[p++];
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;                    // TEM, a stray RSTn: no payload
        if (m == 0x00 || m == 0xD8 || m == 0xD9) JPEG_NO("SOI, EOI or a stuffed byte in the header");
        if (p + 2 > len) JPEG_NO("the header is truncated");
        const int64_t L = ((int64_t)d[p] << 8) | d[p + 1];
        if (L < 2 || p + L > len) JPEG_NO("a segment runs past the end of the file");
        const uint8_t* s = d + p + 2;
        const int64_t n = L - 2;
        p += L;
        if (m == 0xE0) {
            if (n >= 5 && !memcmp(s, "JFIF\0", 5)) jfif = 1;
        } else if (m == 0xEE) {
            if (n >= 12 && !memcmp(s, "Adobe", 5)) {
                adobe = 1;
                transform = s[11];
            }
        } else if (m == 0xDB) {
            for (int64_t q = 0; q < n;) {
                const int pq = s[q] >> 4, tq = s[q] & 15;
                const int64_t bytes = 64 * (pq ? 2 : 1);
                if (pq > 1 || tq > 3 || q + 1 + bytes > n) JPEG_NO("a bad quantisation table");
                for (int k = 0; k < 64; ++k)
                    qtab[tq][jpeg_natural_order[k]] = pq ? (uint16_t)((s[q + 1 + 2 * k] << 8) | s[q + 2 + 2 * k]) : s[q + 1 + k];
                have_q[tq] = 1;
                q += 1 + bytes;
            }
        } else if (m == 0xC4) {
            for (int64_t q = 0; q < n;) {
                if (q + 17 > n) JPEG_NO("a bad Huffman table");
                const int tc = s[q] >> 4, th = s[q] & 15;
                if (tc > 1 || th > 3) JPEG_NO("a bad Huffman table");
                jpeg_huff* h = &o->huff[tc][th];
                int total = 0;
                h->counts[0] = 0;
                for (int l = 1; l <= 16; ++l) total += (h->counts[l] = s[q + l]);
                if (total > 256 || q + 17 + total > n) JPEG_NO("a bad Huffman table");
                memset(h->symbols, 0, sizeof(h->symbols));
                memcpy(h->symbols, s + q + 17, (size_t)total);
                if (!jpeg_build_huff(h)) JPEG_NO("a bad Huffman table");
                q += 17 + total;
            }
        } else if (m == 0xC0 || m == 0xC1) {
            if (sof) JPEG_NO("two frame headers");
            if (n < 6) JPEG_NO("a bad frame header");
            if (s[0] != 8) JPEG_NO("sample precision other than 8 bits");
            o->H = (s[1] << 8) | s[2];
            o->W = (s[3] << 8) | s[4];
            o->ncomp = s[5];
            if (o->H < 1 || o->W < 1) JPEG_NO("an empty frame (or a height left to a DNL marker)");
            if (o->ncomp != 1 && o->ncomp != 3) JPEG_NO("neither 1 nor 3 components");
            if (n < 6 + 3 * o->ncomp) JPEG_NO("a bad frame header");
            for (int c = 0; c < o->ncomp; ++c) {
                comp_id[c] = s[6 + 3 * c];
                comp_h[c] = s[7 + 3 * c] >> 4;
                comp_v[c] = s[7 + 3 * c] & 15;
                comp_q[c] = s[8 + 3 * c];
                if (comp_h[c] < 1 || comp_h[c] > 4 || comp_v[c] < 1 || comp_v[c] > 4 || comp_q[c] > 3) JPEG_NO("a bad frame header");
            }
            sof = 1;
        } else if (m >= 0xC2 && m <= 0xCF && m != 0xCC) {                        // 0xC4 was taken above
            JPEG_NO("progressive, lossless, hierarchical or arithmetic coding");
        } else if (m == 0xDD) {
            if (n != 2) JPEG_NO("a bad restart interval");
            o->restart = (s[0] << 8) | s[1];
        } else if (m == 0xDA) {
            if (!sof) JPEG_NO("a scan before the frame header");
            if (n < 1 || s[0] != o->ncomp || n != 4 + 2 * o->ncomp) JPEG_NO("more than one scan");
            for (int c = 0; c < o->ncomp; ++c) {
                if (s[1 + 2 * c] != comp_id[c]) JPEG_NO("scan components out of frame order");
                o->dc[c] = s[2 + 2 * c] >> 4;
                o->ac[c] = s[2 + 2 * c] & 15;
                if (o->dc[c] > 3 || o->ac[c] > 3 || !o->huff[0][o->dc[c]].defined || !o->huff[1][o->ac[c]].defined)
                    JPEG_NO("the scan names a Huffman table the file does not define");
                if (!have_q[comp_q[c]]) JPEG_NO("the frame names a quantisation table the file does not define");
                memcpy(o->qt[c], qtab[comp_q[c]], sizeof(o->qt[c]));
            }
            if (s[1 + 2 * o->ncomp] != 0 || s[2 + 2 * o->ncomp] != 63 || s[3 + 2 * o->ncomp] != 0) JPEG_NO("a spectral selection or successive approximation scan");
            break;
        }
        // every other segment (APPn, COM, DAC, ...) is skipped
    }
    o->sampling = JPEG_444;
    if (o->ncomp == 3) {
        // libjpeg's colour-space rule: JFIF means YCbCr; else Adobe's transform flag decides; else ids 'R','G','B' mean RGB
        if (!jfif && ((adobe && transform == 0) || (!adobe && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B')))
            JPEG_NO("components coded as RGB");
        if (comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1) JPEG_NO("chroma sampled other than 1x1");
        if (comp_h[0] == 1 && comp_v[0] == 1) o->sampling = JPEG_444;
        else if (comp_h[0] == 2 && comp_v[0] == 1) o->sampling = JPEG_422;
        else if (comp_h[0] == 2 && comp_v[0] == 2) o->sampling = JPEG_420;
        else JPEG_NO("luma sampled other than 1x1, 2x1 or 2x2");
    }
    o->blocks = jpeg_blocks(o->H, o->W, o->ncomp, o->sampling, o->bx, o->by);
    o->scan = p;
    return JPEG_OK;
#undef JPEG_NO
}

struct jpeg_bits {
    const uint8_t* d;
    int64_t p, len;
    uint64_t buf;                        // the low `n` bits are the unread bits, oldest on top
    int n;
};

static inline void jpeg_fill(jpeg_bits* b) {
    while (b->n <= 48 && b->p < b->len) {
        const int c = b->d[b->p];
        if (c == 0xFF) {
            if (b->p + 1 >= b->len || b->d[b->p + 1] != 0x00) return;           // a marker (or the end): the segment's bits end here
            b->p += 2;
        } else {
            b->p += 1;
        }
        b->buf = (b->buf << 8) | (uint64_t)c;
        b->n += 8;
    }
}

// the next `k` (1..16) bits without consuming them, zeros past the end of the segment
static inline int jpeg_peek(jpeg_bits* b, int k) {
    if (b->n < k) jpeg_fill(b);
    if (b->n >= k) return (int)((b->buf >> (b->n - k)) & ((1u << k) - 1));
    return (int)((b->buf << (k - b->n)) & ((1u << k) - 1));
}

// -> the symbol, -1: the segment ended, -2: no such code
static inline int jpeg_symbol(jpeg_bits* b, const jpeg_huff* h) {
    const int look = jpeg_peek(b, 16);
    int l, sym;
    const int f = h->fast[look >> (16 - JPEG_FAST_BITS)];
    if (f) {
        l = f >> 8;
        sym = f & 255;
    } else {
        for (l = JPEG_FAST_BITS + 1; (look >> (16 - (l > 16 ? 16 : l))) > h->maxcode[l]; ++l) {}
        if (l > 16) return -2;
        sym = h->symbols[((look >> (16 - l)) + h->valoff[l]) & 255];
    }
    if (l > b->n) return -1;
    b->n -= l;
    return sym;
}

// `s` (1..16) bits as the signed value JPEG's EXTEND gives; *ok = 0 when the segment ended
static inline int jpeg_receive_extend(jpeg_bits* b, int s, int* ok) {
    const int v = jpeg_peek(b, s);
    if (s > b->n) {
        *ok = 0;
        return 0;
    }
    b->n -= s;
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// coef: blocks * 64 int16, written in full (zeros where the file codes none).  JPEG_OK or JPEG_CORRUPT.
static inline int jpeg_entropy(const uint8_t* d, int64_t len, const jpeg_info* o, int16_t* coef, char* err, size_t errlen) {
    memset(coef, 0, (size_t)o->blocks * 64 * sizeof(int16_t));
    const int hs = o->bx[0] / o->bx[1], vs = o->by[0] / o->by[1];
    const int mcus_x = o->bx[1], mcus_y = o->by[1];
    int16_t* plane[3] = {coef, coef + (int64_t)o->bx[0] * o->by[0] * 64, coef + ((int64_t)o->bx[0] * o->by[0] + (int64_t)o->bx[1] * o->by[1]) * 64};
    jpeg_bits b = {d, o->scan, len, 0, 0};
    uint32_t pred[3] = {0, 0, 0};
    int64_t mcu = 0;
    const int64_t mcus = (int64_t)mcus_x * mcus_y;
    for (int my = 0; my < mcus_y; ++my) {
        for (int mx = 0; mx < mcus_x; ++mx, ++mcu) {
            if (o->restart && mcu && mcu % o->restart == 0) {
                b.n = 0;                                                         // the padding bits of the interval
                b.buf = 0;
                while (b.p + 1 < b.len && b.d[b.p] == 0xFF && b.d[b.p + 1] == 0xFF) ++b.p;
                const int want = 0xD0 + (int)((mcu / o->restart - 1) & 7);
                if (b.p + 1 >= b.len || b.d[b.p] != 0xFF || b.d[b.p + 1] != want) {
                    char msg[128];
                    snprintf(msg, sizeof(msg), "corrupt JPEG data: no RST%d marker before MCU %lld of %lld", want - 0xD0, (long long)mcu, (long long)mcus);
                    return jpeg_say(err, errlen, JPEG_CORRUPT, msg);
                }
                b.p += 2;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < o->ncomp; ++c) {
                const int nh = c ? 1 : hs, nv = c ? 1 : vs, pbx = c ? o->bx[1] : o->bx[0];
                const jpeg_huff* hd = &o->huff[0][o->dc[c]];
                const jpeg_huff* ha = &o->huff[1][o->ac[c]];
                for (int v = 0; v < nv; ++v)
                    for (int h = 0; h < nh; ++h) {
                        int16_t* blk = plane[c] + ((int64_t)(my * nv + v) * pbx + (mx * nh + h)) * 64;
                        int ok = 1;
                        const char* what = NULL;
                        int s = jpeg_symbol(&b, hd);
                        if (s < 0) what = s == -1 ? "the entropy-coded segment is truncated" : "an unassigned Huffman code";
                        else if (s > 16) what = "a DC difference of more than 16 bits";
                        else {
                            if (s) pred[c] += (uint32_t)jpeg_receive_extend(&b, s, &ok);
                            blk[0] = (int16_t)pred[c];
                            for (int k = 1; ok && k < 64;) {
                                const int rs = jpeg_symbol(&b, ha);
                                if (rs < 0) {
                                    what = rs == -1 ? "the entropy-coded segment is truncated" : "an unassigned Huffman code";
                                    break;
                                }
                                const int r = rs >> 4;
                                s = rs & 15;
                                if (s == 0) {
                                    if (r != 15) break;                          // end of block
                                    k += 16;
                                    continue;
                                }
                                k += r;
                                if (k > 63) {
                                    what = "a coefficient index past 63";
                                    break;
                                }
                                blk[jpeg_natural_order[k++]] = (int16_t)jpeg_receive_extend(&b, s, &ok);
                            }
                            if (!ok && !what) what = "the entropy-coded segment is truncated";
                        }
                        if (what) {
                            char msg[160];
                            snprintf(msg, sizeof(msg), "corrupt JPEG data: %s (MCU %lld of %lld)", what, (long long)mcu, (long long)mcus);
                            return jpeg_say(err, errlen, JPEG_CORRUPT, msg);
                        }
                    }
            }
        }
    }
    return JPEG_OK;
}
