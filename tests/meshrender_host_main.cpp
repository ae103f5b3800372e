// meshrender_host_main.cpp - csrc/meshrender_math.h on the host: renders a mesh through the header's functions - the face check, the
// pixel boxes, the hit rule, the z-buffer key, the shading - over exact-size heap buffers read from a file, so AddressSanitizer sees
// any index that leaves them.  tests/test_meshrender_host.py builds and runs it and compares every output with the numpy replay,
// which has no boxes.  The plumbing (loops in place of the device's lanes, a plain minimum in place of atomicMin) is plain C++.
//   meshrender_host_main <in.bin> <out.bin>
// in:  int32 V, F, N, H, W, cull, shading, has_colors, has_normals, 0 | float32 fx, fy, cx, cy, near, far, background [3] |
//      float32 verts [V,3] | int32 faces [F,3] | float32 colors [V,3] (if has_colors) | float32 normals [V,3] (if has_normals) |
//      float32 c2w [N,3,4]
// out: int64 counts [4] | int32 face [N,H,W] | float32 depth, disp, acc [N,H,W] each | float32 bary [N,H,W,3] | float32 rgb [N,H,W,3]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "meshrender_math.h"

template <typename T>
static T* read_exact(FILE* f, size_t n) {
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (n && fread(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "short read\n");
        exit(2);
    }
    return p;
}

template <typename T>
static T* alloc_exact(size_t n) { return (T*)calloc(n ? n : 1, sizeof(T)); }

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: meshrender_host_main <in.bin> <out.bin>\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t* hd = read_exact<int32_t>(in, 10);
    const int64_t V = hd[0], F = hd[1], N = hd[2];
    const int H = hd[3], W = hd[4], cull = hd[5], shading = hd[6];
    float* fl = read_exact<float>(in, 9);
    const float fx = fl[0], fy = fl[1], cx = fl[2], cy = fl[3], near = fl[4], far = fl[5];
    float* verts = read_exact<float>(in, 3 * V);
    int32_t* faces = read_exact<int32_t>(in, 3 * F);
    float* colors = hd[7] ? read_exact<float>(in, 3 * V) : nullptr;
    float* normals = hd[8] ? read_exact<float>(in, 3 * V) : nullptr;
    float* c2w = read_exact<float>(in, 12 * N);
    fclose(in);

    const int64_t hw = (int64_t)H * W, pixels = N * hw;
    uint64_t* z = alloc_exact<uint64_t>(pixels);
    for (int64_t i = 0; i < pixels; ++i) z[i] = MESHRENDER_EMPTY;
    int64_t counts[4] = {0, 0, 0, 0};

    // raster: every (view, face) pair walks its box
    for (int64_t n = 0; n < N; ++n) {
        float r[9], o[3];
        for (int i = 0; i < 3; ++i) {
            for (int k = 0; k < 3; ++k) r[3 * i + k] = c2w[12 * n + 4 * i + k];
            o[i] = c2w[12 * n + 4 * i + 3];
        }
        const bool boxes = meshrender_view_boxes(r, fx, fy, H, W);
        for (int64_t f = 0; f < F; ++f) {
            if (!meshrender_face_ok(verts, faces, f, V)) {
                counts[0] += n == 0;
                continue;
            }
            const float *p0 = verts + 3 * (int64_t)faces[3 * f], *p1 = verts + 3 * (int64_t)faces[3 * f + 1], *p2 = verts + 3 * (int64_t)faces[3 * f + 2];
            int box[4];
            if (meshrender_box(p0, p1, p2, o, r, fx, fy, cx, cy, H, W, boxes, box) == MESHRENDER_BOX_SKIP) {
                ++counts[1];
                continue;
            }
            counts[2] += meshrender_box_pixels(box) > MESHRENDER_NARROW_PIXELS;
            for (int py = box[2]; py <= box[3]; ++py)
                for (int px = box[0]; px <= box[1]; ++px) {
                    float d[3];
                    meshrender_ray_dir(fx, fy, cx, cy, r, (float)px, (float)py, d);
                    MeshrenderHit h;
                    if (!meshrender_hit(p0, p1, p2, o, d, near, far, cull, h)) continue;
                    const uint64_t key = meshrender_key(h.tf, (uint32_t)f);
                    uint64_t* w = z + (n * H + py) * (int64_t)W + px;
                    if (key < *w) *w = key;
                    ++counts[3];
                }
        }
    }

    // resolve
    int32_t* face = alloc_exact<int32_t>(pixels);
    float *depth = alloc_exact<float>(pixels), *disp = alloc_exact<float>(pixels), *acc = alloc_exact<float>(pixels);
    float *bary = alloc_exact<float>(3 * pixels), *rgb = alloc_exact<float>(3 * pixels);
    for (int64_t i = 0; i < pixels; ++i) {
        face[i] = -1;
        for (int k = 0; k < 3; ++k) rgb[3 * i + k] = fl[6 + k];
        if (z[i] == MESHRENDER_EMPTY) continue;
        const int64_t f = (int64_t)(z[i] & 0xFFFFFFFFull), n = i / hw, rem = i - n * hw;
        const int py = (int)(rem / W), px = (int)(rem - (int64_t)py * W);
        float r[9], o[3], d[3];
        for (int a = 0; a < 3; ++a) {
            for (int k = 0; k < 3; ++k) r[3 * a + k] = c2w[12 * n + 4 * a + k];
            o[a] = c2w[12 * n + 4 * a + 3];
        }
        const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        meshrender_ray_dir(fx, fy, cx, cy, r, (float)px, (float)py, d);
        MeshrenderHit h;
        meshrender_hit(verts + 3 * a, verts + 3 * b, verts + 3 * c, o, d, 0.f, 0.f, MESHRENDER_CULL_NONE, h);
        if (meshrender_key(h.tf, (uint32_t)f) != z[i]) {
            fprintf(stderr, "pixel %lld: the recomputed depth bits differ from the key's\n", (long long)i);
            return 3;
        }
        face[i] = (int32_t)f;
        depth[i] = h.tf;
        disp[i] = (float)(1.0 / (double)h.tf);
        acc[i] = 1.f;
        bary[3 * i] = (float)(h.U / h.det); bary[3 * i + 1] = (float)(h.V / h.det); bary[3 * i + 2] = (float)(h.W / h.det);
        meshrender_shade(shading, h, colors ? colors + 3 * a : nullptr, colors ? colors + 3 * b : nullptr, colors ? colors + 3 * c : nullptr,
                         normals ? normals + 3 * a : nullptr, normals ? normals + 3 * b : nullptr, normals ? normals + 3 * c : nullptr, d, rgb + 3 * i);
    }

    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    fwrite(counts, sizeof(int64_t), 4, out);
    fwrite(face, sizeof(int32_t), pixels, out);
    fwrite(depth, sizeof(float), pixels, out);
    fwrite(disp, sizeof(float), pixels, out);
    fwrite(acc, sizeof(float), pixels, out);
    fwrite(bary, sizeof(float), 3 * pixels, out);
    fwrite(rgb, sizeof(float), 3 * pixels, out);
    fclose(out);
    free(hd); free(fl); free(verts); free(faces); free(colors); free(normals); free(c2w); free(z);
    free(face); free(depth); free(disp); free(acc); free(bary); free(rgb);
    return 0;
}
