// meshops_host_main.cpp - csrc/meshops_math.h on the host: loops the header's functions over exact-size heap buffers read from a
// file, so AddressSanitizer sees any index that leaves them.  tests/test_meshops_host.py builds and runs it.
//   meshops_host_main <in.bin> <out.bin> <s>
// in:  int32 V, F | float32 verts [V,3] | int32 faces [F,3] | int32 offsets [V+1] | int32 items [3F]
// out: float32 smoothed [V,3] (one step with factor s) | float32 normals [V,3] | float64 terms [F,5] | int64 E, boundary, non-manifold
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "meshops_math.h"

template <typename T>
static T* read_exact(FILE* f, size_t n) {
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (n && fread(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "short read\n");
        exit(2);
    }
    return p;
}

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: meshops_host_main <in.bin> <out.bin> <s>\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t* hd = read_exact<int32_t>(in, 2);
    const int64_t V = hd[0], F = hd[1];
    float* P = read_exact<float>(in, 3 * V);
    int32_t* faces = read_exact<int32_t>(in, 3 * F);
    int32_t* offsets = read_exact<int32_t>(in, V + 1);
    int32_t* items = read_exact<int32_t>(in, 3 * F);
    fclose(in);
    const float s = strtof(argv[3], nullptr);

    float* sm = (float*)malloc(V ? 3 * V * sizeof(float) : 1);
    float* nr = (float*)malloc(V ? 3 * V * sizeof(float) : 1);
    double* terms = (double*)malloc(F ? MESHOPS_FACE_TERMS * F * sizeof(double) : 1);
    for (int64_t v = 0; v < V; ++v) {
        meshops_smooth_vertex(P, faces, items, offsets[v], offsets[v + 1], v, V, F, s, sm + 3 * v);
        meshops_vertex_normal(P, faces, items, offsets[v], offsets[v + 1], V, F, nr + 3 * v);
    }
    for (int64_t f = 0; f < F; ++f)
        meshops_face_terms(P + 3 * (int64_t)faces[3 * f], P + 3 * (int64_t)faces[3 * f + 1], P + 3 * (int64_t)faces[3 * f + 2],
                           terms + MESHOPS_FACE_TERMS * f);
    int64_t edges[3] = {0, 0, 0};
    for (int64_t c = 0; c < 3 * F; ++c) {
        const int32_t f = (int32_t)(c / 3), k = (int32_t)(c - 3 * f);
        const int32_t a = faces[c], b = faces[3 * f + (k + 1) % 3];
        const bool from_a = offsets[a + 1] - offsets[a] <= offsets[b + 1] - offsets[b];
        const int32_t x = from_a ? a : b, y = from_a ? b : a;
        const MeshopsEdge e = meshops_edge_scan(faces, items, offsets[x], offsets[x + 1], x, y, F);
        if (e.first != (int32_t)c) continue;
        ++edges[0];
        edges[1] += e.n_xy + e.n_yx == 1;
        edges[2] += e.n_xy + e.n_yx > 2 || e.n_xy >= 2 || e.n_yx >= 2;
    }
    // the key round trip the bounding box relies on
    for (int64_t i = 0; i < 3 * V; ++i)
        if (meshops_key_float(meshops_float_key(P[i])) != P[i]) {
            fprintf(stderr, "float key round trip failed at %lld\n", (long long)i);
            return 3;
        }

    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    fwrite(sm, sizeof(float), 3 * V, out);
    fwrite(nr, sizeof(float), 3 * V, out);
    fwrite(terms, sizeof(double), MESHOPS_FACE_TERMS * F, out);
    fwrite(edges, sizeof(int64_t), 3, out);
    fclose(out);
    free(hd); free(P); free(faces); free(offsets); free(items); free(sm); free(nr); free(terms);
    return 0;
}
