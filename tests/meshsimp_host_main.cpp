// meshsimp_host_main.cpp - the welding / decimation part of csrc/meshops_math.h on the host: clusters, collapses and places a mesh
// with the header's functions over exact-size heap buffers read from a file, so AddressSanitizer sees any index that leaves them.
// tests/test_meshsimp_host.py builds and runs it.  The plumbing around the header (a sort in place of the device's table, counting
// sorts in place of its fill-and-sort lists) is plain C++.
//   meshsimp_host_main <in.bin> <out.bin> <cell> <eps> <placement 0|1|2>
// in:  int32 V, F, has_colors, has_origin | float32 verts [V,3] | int32 faces [F,3] | float32 colors [V,3] (if has_colors) |
//      float32 origin [3] (if has_origin; else the per-axis minimum by meshops_float_key)
// out: int32 clusters, invalid, V', F', degenerate, duplicate | float32 origin [3] | int32 vlabel [V] | float32 verts' [V',3] |
//      int32 faces' [F',3] | float32 colors' [V',3] (if has_colors); with invalid vertices only the six counts are written
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <utility>
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

template <typename T>
static T* alloc_exact(size_t n) { return (T*)calloc(n ? n : 1, sizeof(T)); }

// offsets [V+1], items [n]: the positions i of key[i] == v per v, ascending
static void csr(const int32_t* key, int64_t n, int64_t V, int32_t* offsets, int32_t* items) {
    for (int64_t v = 0; v <= V; ++v) offsets[v] = 0;
    for (int64_t i = 0; i < n; ++i) ++offsets[key[i] + 1];
    for (int64_t v = 0; v < V; ++v) offsets[v + 1] += offsets[v];
    int32_t* cur = alloc_exact<int32_t>(V);
    for (int64_t i = 0; i < n; ++i) items[offsets[key[i]] + cur[key[i]]++] = (int32_t)i;
    free(cur);
}

int main(int argc, char** argv) {
    if (argc != 6) {
        fprintf(stderr, "usage: meshsimp_host_main <in.bin> <out.bin> <cell> <eps> <placement>\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t* hd = read_exact<int32_t>(in, 4);
    const int64_t V = hd[0], F = hd[1];
    const bool has_colors = hd[2] != 0, has_origin = hd[3] != 0;
    float* P = read_exact<float>(in, 3 * V);
    int32_t* faces = read_exact<int32_t>(in, 3 * F);
    float* colors = has_colors ? read_exact<float>(in, 3 * V) : nullptr;
    float* origin = has_origin ? read_exact<float>(in, 3) : alloc_exact<float>(3);
    fclose(in);
    const float h = strtof(argv[3], nullptr);
    const double eps = strtod(argv[4], nullptr);
    const int placement = atoi(argv[5]);

    if (!has_origin && V > 0) {
        uint32_t k[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        for (int64_t i = 0; i < 3 * V; ++i) k[i % 3] = std::min(k[i % 3], meshops_float_key(P[i]));
        for (int q = 0; q < 3; ++q) origin[q] = meshops_key_float(k[q]);
    }

    int32_t counts[6] = {0, 0, 0, 0, 0, 0};
    std::vector<std::pair<uint64_t, int32_t>> keyed;
    for (int64_t v = 0; v < V; ++v) {
        const uint64_t key = meshops_cell_key(P + 3 * v, origin, h, nullptr);
        if (key == MESHOPS_NO_CELL) ++counts[1]; else keyed.push_back({key, (int32_t)v});
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    if (counts[1]) {
        fwrite(counts, sizeof(int32_t), 6, out);
        fclose(out);
        free(hd); free(P); free(faces); free(colors); free(origin);
        return 0;
    }
    std::sort(keyed.begin(), keyed.end());
    int32_t* vlabel = alloc_exact<int32_t>(V);
    for (size_t i = 0, run = 0; i < keyed.size(); ++i) {
        if (i == 0 || keyed[i].first != keyed[i - 1].first) {
            run = i;
            ++counts[0];
        }
        vlabel[keyed[i].second] = keyed[run].second;               // the smallest index of the run: pairs sort by (key, index)
    }

    int32_t* gl = alloc_exact<int32_t>(3 * F);
    for (int64_t c = 0; c < 3 * F; ++c) {
        if (!meshops_index_ok(faces[c], V)) {
            fprintf(stderr, "bad face index\n");
            return 4;
        }
        gl[c] = vlabel[faces[c]];
    }
    int32_t *off = alloc_exact<int32_t>(V + 1), *items = alloc_exact<int32_t>(3 * F);
    int32_t *moff = alloc_exact<int32_t>(V + 1), *mitems = alloc_exact<int32_t>(V);
    csr(gl, 3 * F, V, off, items);
    csr(vlabel, V, V, moff, mitems);

    int32_t *keep = alloc_exact<int32_t>(F), *vmap = alloc_exact<int32_t>(V);
    for (int64_t v = 0; v < V; ++v) vmap[v] = -1;
    for (int64_t f = 0; f < F; ++f) {
        int32_t r[3];
        if (!meshops_collapsed_face(gl + 3 * f, r)) {
            ++counts[4];
            continue;
        }
        int32_t best = r[0], len = off[r[0] + 1] - off[r[0]];
        for (int k = 1; k < 3; ++k) {
            const int32_t n = off[r[k] + 1] - off[r[k]];
            if (n < len) {
                len = n;
                best = r[k];
            }
        }
        if (meshops_face_is_duplicate(gl, items, off[best], off[best + 1], (int32_t)f, r, F)) {
            ++counts[5];
            continue;
        }
        keep[f] = 1;
        ++counts[3];
        for (int k = 0; k < 3; ++k) vmap[r[k]] = 0;
    }
    for (int64_t v = 0; v < V; ++v)
        if (vmap[v] == 0) vmap[v] = counts[2]++;
    const int64_t Vo = counts[2], Fo = counts[3];
    float *vo = alloc_exact<float>(3 * Vo), *co = alloc_exact<float>(3 * Vo);
    int32_t* fo = alloc_exact<int32_t>(3 * Fo);
    for (int64_t f = 0, o = 0; f < F; ++f)
        if (keep[f]) {
            for (int k = 0; k < 3; ++k) fo[3 * o + k] = vmap[gl[3 * f + k]];
            ++o;
        }
    for (int64_t l = 0; l < V; ++l)
        if (vmap[l] >= 0)
            meshops_place_vertex(placement, P, colors, faces, mitems, moff[l], moff[l + 1], items, off[l], off[l + 1], l, V, F, origin, h, eps,
                                 vo + 3 * (int64_t)vmap[l], co + 3 * (int64_t)vmap[l]);

    fwrite(counts, sizeof(int32_t), 6, out);
    fwrite(origin, sizeof(float), 3, out);
    fwrite(vlabel, sizeof(int32_t), V, out);
    fwrite(vo, sizeof(float), 3 * Vo, out);
    fwrite(fo, sizeof(int32_t), 3 * Fo, out);
    if (has_colors) fwrite(co, sizeof(float), 3 * Vo, out);
    fclose(out);
    free(hd); free(P); free(faces); free(colors); free(origin); free(vlabel); free(gl); free(off); free(items); free(moff); free(mitems);
    free(keep); free(vmap); free(vo); free(co); free(fo);
    return 0;
}
