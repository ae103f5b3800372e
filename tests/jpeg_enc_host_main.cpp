// jpeg_enc_host_main.cpp - the JPEG encode on the host, by looping the lane functions the device kernels consist of
// (csrc/jpeg_enc_math.h) over std::vectors that end where the data ends, then the Huffman writer (csrc/jpeg_enc_host.h) with
// `cap` equal to the file bound.  Built by tests/test_jpeg_enc_host.py with g++ under AddressSanitizer and UBSan, so an overrun of
// a frame, plane, coefficient or output buffer is caught here, before anything runs on a GPU.
//   jpeg_enc_host_main check <list>     every line: <pixels> <H> <W> <channels> <u8|f32> <divisor> <components> <sampling> <quality> <expected.jpg>
// For every line: "<expected.jpg>: equal <bytes> (bound <bound>)" or a MISMATCH line; then the writer must refuse cap 0, the real
// size minus one and caps in between without writing past `cap`.  Exit status 0 when every line was equal.
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "jpeg_enc_host.h"
#include "jpeg_enc_math.h"

static std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> v;
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

int main(int argc, char** argv) {
#if defined(__SANITIZE_ADDRESS__)
    printf("build: AddressSanitizer + UBSan\n");
#else
    printf("build: plain\n");
#endif
    if (argc != 3 || std::string(argv[1]) != "check") {
        fprintf(stderr, "usage: %s check <list>\n", argv[0]);
        return 2;
    }
    FILE* list = fopen(argv[2], "r");
    if (!list) return 2;
    char pix[1024], kind[16], want_path[1024];
    int H, W, cin, ncomp, sampling, quality, bad = 0;
    float divisor;
    while (fscanf(list, "%1023s %d %d %d %15s %f %d %d %d %1023s", pix, &H, &W, &cin, kind, &divisor, &ncomp, &sampling, &quality, want_path) == 10) {
        const int u8 = std::string(kind) == "u8";
        const std::vector<uint8_t> frames = slurp(pix), want = slurp(want_path);
        const int64_t per = (int64_t)H * W * cin * (u8 ? 1 : 4);
        if (frames.empty() || (int64_t)frames.size() % per) {
            printf("%s: BAD INPUT SIZE\n", pix);
            return 2;
        }
        const int64_t n = (int64_t)frames.size() / per;
        int bx[2], by[2];
        const int64_t B = jpeg_blocks(H, W, ncomp, sampling, bx, by);
        std::vector<uint16_t> qt2(128);
        jpeg_quant_tables(quality, qt2.data());
        std::vector<uint16_t> qt((size_t)ncomp * 64);                            // the device's table: one per component
        for (int c = 0; c < ncomp; ++c)
            for (int k = 0; k < 64; ++k) qt[64 * c + k] = qt2[64 * (c ? 1 : 0) + k];
        std::vector<uint8_t> planes((size_t)(n * B * 64));
        std::vector<int16_t> coef((size_t)(n * B * 64));
        for (int64_t t = 0; t < n * B * 16; ++t) jpeg_enc_planes_lane(t, frames.data(), u8, cin, divisor, H, W, ncomp, sampling, bx[0], by[0], bx[1], by[1], planes.data());
        for (int64_t g = 0; g < n * B; ++g) jpeg_enc_fdct_lane(g, planes.data(), qt.data(), H, W, ncomp, bx[0], by[0], bx[1], by[1], coef.data());
        const int64_t bound = jpeg_enc_file_bound(H, W, ncomp, sampling);
        std::vector<uint8_t> got;
        int64_t last = 0;
        for (int64_t k = 0; k < n; ++k) {                                      // the expected file holds the n files one after another
            std::vector<uint8_t> out((size_t)bound);
            const int64_t len = jpeg_enc_write(coef.data() + k * B * 64, qt2.data(), H, W, ncomp, sampling, out.data(), bound);
            if (len < 0) {
                printf("%s: WRITE FAILED %lld\n", want_path, (long long)len);
                return 1;
            }
            got.insert(got.end(), out.begin(), out.begin() + len);
            last = len;
            const int64_t caps[6] = {0, 1, len / 3, len / 2, len - 2, len - 1};
            for (int64_t cap : caps) {
                if (cap < 0) continue;
                std::vector<uint8_t> small((size_t)cap);
                if (jpeg_enc_write(coef.data() + k * B * 64, qt2.data(), H, W, ncomp, sampling, small.data(), cap) != JPEG_ENC_SHORT) {
                    printf("%s: cap %lld NOT REFUSED\n", want_path, (long long)cap);
                    ++bad;
                }
            }
            std::vector<uint8_t> exact((size_t)len);
            if (jpeg_enc_write(coef.data() + k * B * 64, qt2.data(), H, W, ncomp, sampling, exact.data(), len) != len) {
                printf("%s: the exact cap REFUSED\n", want_path);
                ++bad;
            }
        }
        if (got == want) {
            printf("%s: equal %lld bytes in %lld file(s) (bound %lld, last file %lld)\n", want_path, (long long)got.size(), (long long)n, (long long)bound, (long long)last);
        } else {
            size_t d = 0;
            while (d < got.size() && d < want.size() && got[d] == want[d]) ++d;
            printf("%s: MISMATCH at byte %zu (%zu bytes, expected %zu)\n", want_path, d, got.size(), want.size());
            ++bad;
        }
    }
    fclose(list);
    printf("%d bad\n", bad);
    return bad ? 1 : 0;
}
