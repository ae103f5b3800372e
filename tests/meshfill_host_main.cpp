// meshfill_host_main.cpp - the hole-filling part of csrc/meshops_math.h on the host: finds the boundary half-edges, traces the loops
// and caps them with the header's functions over exact-size heap buffers read from a file, so AddressSanitizer sees any index that
// leaves them.  tests/test_meshfill_host.py builds and runs it.  The plumbing around the header (a counting sort for the incidence,
// a plain walk along next in place of the device's pointer jumping) is plain C++.
//   meshfill_host_main <in.bin> <out.bin> <max_edges, 0 = no limit>
// in:  int32 V, F, has_colors | float32 verts [V,3] | int32 faces [F,3] | float32 colors [V,3] (if has_colors)
// out: int32 boundary edges, loops, filled loops, filled edges, skipped loops, unfillable edges, new vertices, new faces |
//      int32 table [L,2] | int32 loop_offsets [L+1] | int32 loop_vertices [M] | float32 verts' | int32 faces' | float32 colors'
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
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

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: meshfill_host_main <in.bin> <out.bin> <max_edges>\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t* hd = read_exact<int32_t>(in, 3);
    const int64_t V = hd[0], F = hd[1];
    const bool has_colors = hd[2] != 0;
    float* P = read_exact<float>(in, 3 * V);
    int32_t* faces = read_exact<int32_t>(in, 3 * F);
    float* colors = has_colors ? read_exact<float>(in, 3 * V) : nullptr;
    fclose(in);
    const int64_t max_edges = atoll(argv[3]);

    // incidence: corners per vertex, ascending
    int32_t *offsets = alloc_exact<int32_t>(V + 1), *items = alloc_exact<int32_t>(3 * F), *cur = alloc_exact<int32_t>(V);
    for (int64_t c = 0; c < 3 * F; ++c) {
        if (!meshops_index_ok(faces[c], V)) {
            fprintf(stderr, "bad face index\n");
            return 4;
        }
        ++offsets[faces[c] + 1];
    }
    for (int64_t v = 0; v < V; ++v) offsets[v + 1] += offsets[v];
    for (int64_t c = 0; c < 3 * F; ++c) items[offsets[faces[c]] + cur[faces[c]]++] = (int32_t)c;

    // boundary half-edges, ascending; leaving / entering counts; next
    int64_t nb = 0;
    for (int64_t c = 0; c < 3 * F; ++c) nb += meshops_boundary_halfedge(faces, offsets, items, (int32_t)c, V, F);
    int32_t *bhe = alloc_exact<int32_t>(nb), *bnext = alloc_exact<int32_t>(nb);
    int32_t *nout = alloc_exact<int32_t>(V), *nin = alloc_exact<int32_t>(V), *leave = alloc_exact<int32_t>(V);
    for (int64_t c = 0, i = 0; c < 3 * F; ++c)
        if (meshops_boundary_halfedge(faces, offsets, items, (int32_t)c, V, F)) bhe[i++] = (int32_t)c;
    auto head = [&](int32_t c) { return faces[3 * (c / 3) + (c % 3 + 1) % 3]; };
    for (int64_t i = nb - 1; i >= 0; --i) {
        ++nout[faces[bhe[i]]];
        ++nin[head(bhe[i])];
        leave[faces[bhe[i]]] = (int32_t)i;                         // the smallest one is written last
    }
    for (int64_t i = 0; i < nb; ++i) {
        const int32_t h = head(bhe[i]);
        bnext[i] = nout[h] == 1 && nin[h] == 1 ? leave[h] : -1;
    }

    // loops: a walk from every unvisited half-edge in ascending order; the walk that returns to its start is a loop led by the start
    char* seen = alloc_exact<char>(nb);
    int32_t *table = alloc_exact<int32_t>(2 * (nb / 3)), *loop_offsets = alloc_exact<int32_t>(nb / 3 + 1), *loop_vertices = alloc_exact<int32_t>(nb);
    int32_t* path = alloc_exact<int32_t>(nb);
    int64_t L = 0, M = 0;
    for (int64_t s = 0; s < nb; ++s) {
        if (seen[s]) continue;
        int64_t n = 0, i = s;
        while (i >= 0 && !seen[i]) {
            seen[i] = 1;
            path[n++] = (int32_t)i;
            i = bnext[i];
        }
        if (i != s) continue;
        table[2 * L] = bhe[s];
        table[2 * L + 1] = (int32_t)n;
        for (int64_t r = 0; r < n; ++r) loop_vertices[M + r] = faces[bhe[path[r]]];
        M += n;
        loop_offsets[++L] = (int32_t)M;
    }

    // fill
    int32_t counts[8] = {(int32_t)nb, (int32_t)L, 0, 0, 0, (int32_t)(nb - M), 0, 0};
    for (int64_t l = 0; l < L; ++l) {
        const int32_t n = table[2 * l + 1];
        if (max_edges != 0 && n > max_edges) {
            ++counts[4];
            continue;
        }
        ++counts[2];
        counts[3] += n;
        counts[6] += n >= 4;
        counts[7] += n == 3 ? 1 : n;
    }
    const int64_t Vo = V + counts[6], Fo = F + counts[7], slots = M / MESHOPS_FILL_RUN + L + 2;
    float *vo = alloc_exact<float>(3 * Vo), *co = alloc_exact<float>(has_colors ? 3 * Vo : 0);
    int32_t* fo = alloc_exact<int32_t>(3 * Fo);
    double *part = alloc_exact<double>(3 * slots), *cpart = alloc_exact<double>(3 * slots);
    if (V) memcpy(vo, P, 12 * V);
    if (F) memcpy(fo, faces, 12 * F);
    if (V && has_colors) memcpy(co, colors, 12 * V);
    int64_t vnew = 0, fnew = 0;
    for (int64_t l = 0; l < L; ++l) {
        const int32_t n = table[2 * l + 1], off = loop_offsets[l];
        if (max_edges != 0 && n > max_edges) continue;
        const int32_t nfaces = n == 3 ? 1 : n;
        for (int32_t r = 0; r < nfaces; ++r) meshops_fill_face(loop_vertices + off, n, r, (int32_t)(V + vnew), fo + 3 * (F + fnew + r));
        fnew += nfaces;
        if (n < 4) continue;
        const int32_t nruns = (n + MESHOPS_FILL_RUN - 1) / MESHOPS_FILL_RUN;
        const int64_t slot = meshops_fill_slot(off, l, 0);
        for (int32_t k = 0; k < nruns; ++k) {
            const int32_t lo = off + k * MESHOPS_FILL_RUN, hi = (k + 1) * MESHOPS_FILL_RUN < n ? lo + MESHOPS_FILL_RUN : off + n;
            if (meshops_fill_slot(off, l, k) != slot + k || slot + k >= slots) return 5;
            meshops_run_sum(P, loop_vertices, lo, hi, V, part + 3 * (slot + k));
            if (has_colors) meshops_run_sum(colors, loop_vertices, lo, hi, V, cpart + 3 * (slot + k));
        }
        meshops_blocked_mean(part + 3 * slot, nruns, n, vo + 3 * (V + vnew));
        if (has_colors) meshops_blocked_mean(cpart + 3 * slot, nruns, n, co + 3 * (V + vnew));
        ++vnew;
    }

    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    fwrite(counts, sizeof(int32_t), 8, out);
    fwrite(table, sizeof(int32_t), 2 * L, out);
    fwrite(loop_offsets, sizeof(int32_t), L + 1, out);
    fwrite(loop_vertices, sizeof(int32_t), M, out);
    fwrite(vo, sizeof(float), 3 * Vo, out);
    fwrite(fo, sizeof(int32_t), 3 * Fo, out);
    if (has_colors) fwrite(co, sizeof(float), 3 * Vo, out);
    fclose(out);
    free(hd); free(P); free(faces); free(colors); free(offsets); free(items); free(cur); free(bhe); free(bnext); free(nout); free(nin); free(leave);
    free(seen); free(table); free(loop_offsets); free(loop_vertices); free(path); free(vo); free(co); free(fo); free(part); free(cpart);
    return 0;
}
