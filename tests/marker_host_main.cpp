// marker_host_main.cpp - a stand-alone program around csrc/marker_math.h: the header's functions looped on the host over exact-size
// heap buffers (so a sanitizer sees any index that leaves the image), in double and in float.
//   marker_host_main mask   in.bin r C out.bin   in.bin = int32 H, W, then H * W grey bytes; out.bin = the H * W mask bytes, the
//                                                window sums formed by brute force with marker_window / marker_dark
//   marker_host_main refine in.bin               in.bin = int32 H, W, m, then H * W grey bytes, then m * 8 int32 coarse corners
//                                                (x0 y0 .. x3 y3, pixel indices); prints per candidate and precision one line
//                                                "d|f payload x0 y0 .. x3 y3" (payload -1: dropped)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "marker_math.h"

static std::vector<unsigned char> slurp(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<unsigned char> b((size_t)n);
    if (n && fread(b.data(), 1, (size_t)n, f) != (size_t)n) { fprintf(stderr, "short read of %s\n", path); exit(2); }
    fclose(f);
    return b;
}

// the serial form of marker_kernels.hip's mk_refine_kernel
template <typename T>
static int refine(const uint8_t* g, int H, int W, const int32_t* corners, T* q) {
    T cx[4], cy[4], px[4 * MARKER_SIDE_POINTS], py[4 * MARKER_SIDE_POINTS], lines[4][4], h[8], cell[36];
    int valid[4 * MARKER_SIDE_POINTS];
    for (int k = 0; k < 4; ++k) {
        cx[k] = (T)corners[2 * k] + (T)0.5;
        cy[k] = (T)corners[2 * k + 1] + (T)0.5;
    }
    for (int pt = 0; pt < 4 * MARKER_SIDE_POINTS; ++pt) {
        px[pt] = py[pt] = (T)0;
        valid[pt] = marker_side_point<T>(g, H, W, cx, cy, pt, &px[pt], &py[pt]) ? 1 : 0;
    }
    for (int k = 0; k < 8; ++k) q[k] = (T)0;
    for (int k = 0; k < 4; ++k)
        if (marker_fit_line<T>(px + k * MARKER_SIDE_POINTS, py + k * MARKER_SIDE_POINTS, valid + k * MARKER_SIDE_POINTS, MARKER_SIDE_POINTS,
                               lines[k]) < MARKER_MIN_LINE_POINTS)
            return -1;
    for (int k = 0; k < 4; ++k)
        if (!marker_intersect<T>(lines[(k + 3) & 3], lines[k], &q[2 * k], &q[2 * k + 1])) return -1;
    marker_square_to_quad<T>(q, h);
    for (int k = 0; k < 8; ++k)
        if (!isfinite(h[k])) return -1;
    for (int k = 0; k < 36; ++k) {
        T x, y;
        marker_cell_point<T>(h, k, &x, &y);
        cell[k] = marker_bilinear<T>(g, H, W, x, y);
    }
    return marker_decode<T>(cell);
}

int main(int argc, char** argv) {
    if (argc >= 6 && !strcmp(argv[1], "mask")) {
        const std::vector<unsigned char> in = slurp(argv[2]);
        const int r = atoi(argv[3]), C = atoi(argv[4]);
        int32_t hw[2];
        memcpy(hw, in.data(), 8);
        const int H = hw[0], W = hw[1];
        if ((size_t)H * W + 8 != in.size()) { fprintf(stderr, "bad size\n"); return 2; }
        uint8_t* g = (uint8_t*)malloc((size_t)H * W);                      // exact size: an overrun is a sanitizer report
        uint8_t* m = (uint8_t*)malloc((size_t)H * W);
        memcpy(g, in.data() + 8, (size_t)H * W);
        for (int i = 0; i < H; ++i)
            for (int j = 0; j < W; ++j) {
                int s = 0, cnt = 0;
                for (int y = i - r; y <= i + r; ++y)
                    for (int x = j - r; x <= j + r; ++x)
                        if (y >= 0 && y < H && x >= 0 && x < W) {
                            s += g[(size_t)y * W + x];
                            ++cnt;
                        }
                if (cnt != marker_window(i, r, H) * marker_window(j, r, W)) { fprintf(stderr, "marker_window wrong at %d %d\n", i, j); return 1; }
                m[(size_t)i * W + j] = marker_dark(g[(size_t)i * W + j], s, cnt, C) ? 1 : 0;
            }
        FILE* f = fopen(argv[5], "wb");
        fwrite(m, 1, (size_t)H * W, f);
        fclose(f);
        free(g);
        free(m);
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "refine")) {
        const std::vector<unsigned char> in = slurp(argv[2]);
        int32_t hdr[3];
        memcpy(hdr, in.data(), 12);
        const int H = hdr[0], W = hdr[1], m = hdr[2];
        if ((size_t)H * W + 12 + (size_t)m * 32 != in.size()) { fprintf(stderr, "bad size\n"); return 2; }
        uint8_t* g = (uint8_t*)malloc((size_t)H * W);
        memcpy(g, in.data() + 12, (size_t)H * W);
        std::vector<int32_t> corners((size_t)m * 8);
        memcpy(corners.data(), in.data() + 12 + (size_t)H * W, (size_t)m * 32);
        for (int k = 0; k < m; ++k) {
            double qd[8];
            float qf[8];
            const int pd = refine<double>(g, H, W, corners.data() + 8 * k, qd);
            const int pf = refine<float>(g, H, W, corners.data() + 8 * k, qf);
            printf("d %d", pd);
            for (int i = 0; i < 8; ++i) printf(" %.17g", qd[i]);
            printf("\nf %d", pf);
            for (int i = 0; i < 8; ++i) printf(" %.9g", (double)qf[i]);
            printf("\n");
        }
        free(g);
        return 0;
    }
    fprintf(stderr, "usage: marker_host_main mask in.bin r C out.bin | refine in.bin\n");
    return 2;
}
