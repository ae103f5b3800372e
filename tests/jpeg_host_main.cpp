// A stand-alone program around csrc/jpeg_host.h and csrc/jpeg_math.h for tests/test_jpeg_host.py, which builds it with g++
// (AddressSanitizer + UBSan when they link) and runs it: whole files are decoded on the host by looping the functions the device
// kernels are made of.
//   jpeg_host_main check <list>              every line of <list> is "<file.jpg> <file.rgb>" (H * W * 3 expected bytes) or
//                                            "<file.jpg> -" (must be reported not decodable here); exit 1 on any difference
//   jpeg_host_main fuzz <seed> <count> <file.jpg>...   every truncation length and <count> seeded one-byte mutations of each file;
//                                            each decode ends in a status, whichever it is; exit 0
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "jpeg_host.h"

static const int64_t MAX_FUZZ_COEFS = (int64_t)1 << 24;     // a mutated size field may ask for gigabytes: such a decode is not run

static bool read_file(const char* path, std::vector<uint8_t>* out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t n;
    out->clear();
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) out->insert(out->end(), buf, buf + n);
    fclose(f);
    return true;
}

// -> JPEG_OK with rgb [H * W * 3], JPEG_UNSUPP, JPEG_CORRUPT, or -1: larger than max_coefs
static int decode(const uint8_t* d, int64_t len, int64_t max_coefs, std::vector<uint8_t>* rgb, int* H, int* W, char* err, size_t errlen) {
    jpeg_info* o = new jpeg_info;
    std::vector<int16_t> coef;
    std::vector<uint8_t> planes;
    int rc = jpeg_parse(d, len, o, err, errlen);
    if (rc == JPEG_OK && max_coefs && o->blocks * 64 > max_coefs) rc = -1;
    if (rc == JPEG_OK) {
        coef.resize((size_t)o->blocks * 64);
        rc = jpeg_entropy(d, len, o, coef.data(), err, errlen);
    }
    if (rc == JPEG_OK) {
        planes.resize((size_t)o->blocks * 64);
        int64_t blk = 0, off = 0;
        for (int c = 0; c < o->ncomp; ++c) {
            const int bx = o->bx[c ? 1 : 0], by = o->by[c ? 1 : 0];
            for (int j = 0; j < by; ++j)
                for (int i = 0; i < bx; ++i, ++blk) {
                    int32_t v[64];
                    for (int k = 0; k < 64; ++k) v[k] = jpeg_mul(coef[(size_t)blk * 64 + k], o->qt[c][k]);
                    jpeg_idct_block(v);
                    for (int r = 0; r < 8; ++r)
                        for (int q = 0; q < 8; ++q) planes[(size_t)(off + ((int64_t)j * 8 + r) * bx * 8 + i * 8 + q)] = (uint8_t)v[8 * r + q];
                }
            off += (int64_t)bx * by * 64;
        }
        *H = o->H;
        *W = o->W;
        rgb->resize((size_t)o->H * o->W * 3);
        const uint8_t* Y = planes.data();
        const uint8_t* Cb = Y + (int64_t)o->bx[0] * o->by[0] * 64;
        const uint8_t* Cr = Cb + (int64_t)o->bx[1] * o->by[1] * 64;
        const int64_t ys = (int64_t)o->bx[0] * 8, cs = (int64_t)o->bx[1] * 8;
        const int dw = o->sampling == JPEG_444 ? o->W : (o->W + 1) / 2, dh = o->sampling == JPEG_420 ? (o->H + 1) / 2 : o->H;
        for (int y = 0; y < o->H; ++y)
            for (int x = 0; x < o->W; ++x) {
                uint8_t* px = rgb->data() + ((size_t)y * o->W + x) * 3;
                const int lum = Y[y * ys + x];
                if (o->ncomp == 1) {
                    px[0] = px[1] = px[2] = (uint8_t)lum;
                    continue;
                }
                int cb, cr;
                if (o->sampling == JPEG_444) {
                    cb = Cb[y * cs + x];
                    cr = Cr[y * cs + x];
                } else if (o->sampling == JPEG_422) {
                    cb = jpeg_up_h2v1(Cb + y * cs, dw, x);
                    cr = jpeg_up_h2v1(Cr + y * cs, dw, x);
                } else {
                    const int64_t near = (y >> 1) * cs, far = jpeg_far_row(y, dh) * cs;
                    cb = jpeg_up_h2v2(Cb + near, Cb + far, dw, x);
                    cr = jpeg_up_h2v2(Cr + near, Cr + far, dw, x);
                }
                int r, g, b;
                jpeg_ycc_to_rgb(lum, cb, cr, &r, &g, &b);
                px[0] = (uint8_t)r;
                px[1] = (uint8_t)g;
                px[2] = (uint8_t)b;
            }
    }
    delete o;
    return rc;
}

static int check(const char* list) {
    FILE* f = fopen(list, "r");
    if (!f) return 2;
    char a[4096], b[4096], err[256];
    int bad = 0;
    while (fscanf(f, "%4095s %4095s", a, b) == 2) {
        std::vector<uint8_t> data, want, rgb;
        int H = 0, W = 0;
        err[0] = 0;
        if (!read_file(a, &data)) return 2;
        const int rc = decode(data.data(), (int64_t)data.size(), 0, &rgb, &H, &W, err, sizeof(err));
        if (!strcmp(b, "-")) {
            printf("%s: status %d (%s)%s\n", a, rc, err, rc == JPEG_UNSUPP ? "" : "  EXPECTED not decodable here");
            bad += rc != JPEG_UNSUPP;
            continue;
        }
        if (!read_file(b, &want)) return 2;
        size_t diff = 0;
        if (rc == JPEG_OK && rgb.size() == want.size())
            for (size_t k = 0; k < rgb.size(); ++k) diff += rgb[k] != want[k];
        const bool ok = rc == JPEG_OK && rgb.size() == want.size() && diff == 0;
        printf("%s: status %d, %d x %d, %zu of %zu bytes differ%s %s\n", a, rc, H, W, diff, want.size(), ok ? "" : "  MISMATCH", err);
        bad += !ok;
    }
    fclose(f);
    return bad ? 1 : 0;
}

static int fuzz(uint64_t seed, int count, int nfiles, char** files) {
    char err[256];
    for (int k = 0; k < nfiles; ++k) {
        std::vector<uint8_t> data, rgb;
        if (!read_file(files[k], &data)) return 2;
        long tally[4] = {0, 0, 0, 0};
        int H, W;
        for (size_t len = 0; len <= data.size(); ++len) {
            std::vector<uint8_t> cut(data.begin(), data.begin() + len);      // its own allocation: a read past `len` is caught
            const int rc = decode(cut.data(), (int64_t)len, MAX_FUZZ_COEFS, &rgb, &H, &W, err, sizeof(err));
            ++tally[rc < 0 ? 3 : rc];
        }
        printf("%s: %zu truncations: %ld decoded, %ld not decodable here, %ld corrupt, %ld too large\n", files[k], data.size() + 1, tally[0],
               tally[1], tally[2], tally[3]);
        memset(tally, 0, sizeof(tally));
        uint64_t s = seed + 977 * (uint64_t)k;
        for (int i = 0; i < count; ++i) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            const size_t pos = (size_t)((s >> 33) % data.size());
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            std::vector<uint8_t> mut(data);
            mut[pos] = (uint8_t)(s >> 40);
            const int rc = decode(mut.data(), (int64_t)mut.size(), MAX_FUZZ_COEFS, &rgb, &H, &W, err, sizeof(err));
            ++tally[rc < 0 ? 3 : rc];
        }
        printf("%s: %d mutations: %ld decoded, %ld not decodable here, %ld corrupt, %ld too large\n", files[k], count, tally[0], tally[1],
               tally[2], tally[3]);
    }
    return 0;
}

int main(int argc, char** argv) {
#if defined(__SANITIZE_ADDRESS__)
    printf("build: AddressSanitizer + UndefinedBehaviorSanitizer\n");
#else
    printf("build: plain\n");
#endif
    if (argc == 3 && !strcmp(argv[1], "check")) return check(argv[2]);
    if (argc >= 5 && !strcmp(argv[1], "fuzz")) return fuzz(strtoull(argv[2], NULL, 10), atoi(argv[3]), argc - 4, argv + 4);
    fprintf(stderr, "usage: %s check <list> | fuzz <seed> <count> <file.jpg>...\n", argv[0]);
    return 2;
}
