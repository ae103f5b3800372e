// meshops_kernels.hip - clean-up and measurement of a triangle mesh that is already on the device (what swnerf_mc_emit wrote):
// connected components, selection by component, vertex-face incidence, Taubin smoothing, area-weighted normals, and area / volume /
// extents / edge statistics.  The arithmetic is in meshops_math.h; this file is the graph and reduction plumbing.
//   components  init | union (lock-free union-find, smaller index wins: the label is the component's smallest vertex) | flatten |
//               count (integer atomics) | scan of the root flags | table
//   compact     mark (binary search of the label in the kept list) | two scans | write
//   incidence   count | scan | cursor fill | per-slice sort (ascending corner ids, whatever order the atomics landed in)
//   smooth, normals  one thread per vertex over its sorted slice: a fixed order of fp64 additions
//   measure     union-find again for the component count | vertices (bbox by integer atomics on ordered keys) | corners (edges) |
//               faces (fp64 partial sums per workgroup over contiguous ranges) | one workgroup adds the partials in index order
// Every phase is its own launch; a kernel after the first reader of `faces` returns at once when that one counted a bad index.
// Welding and decimation are in meshsimp_kernels.hip, hole filling in meshfill_kernels.hip; the scan and the CSR construction that
// all three units use are defined here (mo_scan, mo_csr of meshops_common.h).
#include "meshops_common.h"

extern "C" int64_t swnerf_mesh_workspace_bytes(int64_t V, int64_t F) {
    int64_t bytes = 0;
    if (mo_sizes_ok(V, F)) mo_ws(nullptr, V, F, &bytes);
    return bytes;
}

// ---- exclusive scan of an int32 array: tile sums | one workgroup over the tile sums | tiles again ---------------------------------
__global__ __launch_bounds__(MO_THREADS) void mo_tile_sum_kernel(const int32_t* __restrict__ cnt, int64_t n, int64_t ntiles, int32_t* __restrict__ tsum) {
    __shared__ int32_t lds[MO_THREADS / 64];
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t i = tile * MO_THREADS + threadIdx.x;
        int32_t tot;
        block_exclusive_scan<int32_t, MO_THREADS>(i < n ? cnt[i] : 0, lds, &tot);
        if (threadIdx.x == 0) tsum[tile] = tot;
    }
}

__global__ __launch_bounds__(MO_SCAN_THREADS) void mo_scan_tiles_kernel(int64_t ntiles, int32_t* tsum, int32_t* total) {
    __shared__ int32_t lds[MO_SCAN_THREADS / 64];
    const int64_t per = (ntiles + MO_SCAN_THREADS - 1) / MO_SCAN_THREADS;
    const int64_t lo = threadIdx.x * per, hi = lo + per < ntiles ? lo + per : ntiles;
    int32_t s = 0;
    for (int64_t q = lo; q < hi; ++q) s += tsum[q];
    int32_t tot;
    int32_t o = block_exclusive_scan<int32_t, MO_SCAN_THREADS>(s, lds, &tot);
    for (int64_t q = lo; q < hi; ++q) {
        const int32_t a = tsum[q];
        tsum[q] = o;
        o += a;
    }
    if (threadIdx.x == 0 && total) *total = tot;
}

// off may be cnt (each element is read and written by the same thread)
__global__ __launch_bounds__(MO_THREADS) void mo_tile_scan_kernel(const int32_t* cnt, int32_t* off, int64_t n, int64_t ntiles, const int32_t* __restrict__ tsum) {
    __shared__ int32_t lds[MO_THREADS / 64];
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t i = tile * MO_THREADS + threadIdx.x;
        int32_t tot;
        const int32_t ex = block_exclusive_scan<int32_t, MO_THREADS>(i < n ? cnt[i] : 0, lds, &tot);
        if (i < n) off[i] = tsum[tile] + ex;
    }
}

int mo_scan(const int32_t* cnt, int32_t* off, int64_t n, int32_t* tsum, int32_t* total, hipStream_t st) {
    const int64_t ntiles = mo_tiles(n);
    hipLaunchKernelGGL(mo_tile_sum_kernel, dim3(mo_blocks(n)), dim3(MO_THREADS), 0, st, cnt, n, ntiles, tsum);
    hipLaunchKernelGGL(mo_scan_tiles_kernel, dim3(1), dim3(MO_SCAN_THREADS), 0, st, ntiles, tsum, total);
    hipLaunchKernelGGL(mo_tile_scan_kernel, dim3(mo_blocks(n)), dim3(MO_THREADS), 0, st, cnt, off, n, ntiles, (const int32_t*)tsum);
    return sw_check(hipGetLastError(), "mesh scan launches");
}

// ---- components --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MO_THREADS) void mo_init_kernel(int32_t* __restrict__ label, int64_t V) {
    for (int64_t v = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; v < V; v += (int64_t)gridDim.x * MO_THREADS) label[v] = (int32_t)v;
}

// the first reader of `faces`: a face with an index outside 0..V-1 adds its bad indices to *bad and joins nothing
__global__ __launch_bounds__(MO_THREADS) void mo_union_kernel(const int32_t* __restrict__ faces, int64_t V, int64_t F, int32_t* label, int32_t* bad) {
    for (int64_t f = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; f < F; f += (int64_t)gridDim.x * MO_THREADS) {
        const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        const int nbad = !meshops_index_ok(a, V) + !meshops_index_ok(b, V) + !meshops_index_ok(c, V);
        if (nbad) {
            atomicAdd(bad, nbad);
            continue;
        }
        uf_union(label, a, b);
        uf_union(label, b, c);
    }
}

__global__ __launch_bounds__(MO_THREADS) void mo_flatten_kernel(int32_t* label, int64_t V, const int32_t* bad) {
    if (*bad) return;
    for (int64_t v = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; v < V; v += (int64_t)gridDim.x * MO_THREADS) {
        const int root = uf_find(label, (int)v);
        if (root != (int)v) __atomic_store_n(label + v, root, __ATOMIC_RELAXED);
    }
}

// nv[label] += 1 per vertex, nf[label of the first vertex] += 1 per face, isroot[v] = (label[v] == v).  Whole waves loop together
// (mo_count_key shuffles), so the bound is rounded up to the wave.
__global__ __launch_bounds__(MO_THREADS) void mo_count_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ label, int64_t V,
                                                              int64_t F, int32_t* nf, int32_t* nv, int32_t* __restrict__ isroot, const int32_t* bad) {
    if (*bad) return;
    const int64_t n = V > F ? V : F, stride = (int64_t)gridDim.x * MO_THREADS;
    for (int64_t i0 = (int64_t)blockIdx.x * MO_THREADS; i0 < n; i0 += stride) {
        const int64_t i = i0 + threadIdx.x;
        int kv = -1, kf = -1;
        if (i < V) {
            kv = label[i];
            isroot[i] = kv == (int)i;
        }
        if (i < F) kf = label[faces[3 * i]];
        mo_count_key(nv, kv);
        mo_count_key(nf, kf);
    }
}

__global__ __launch_bounds__(MO_THREADS) void mo_table_kernel(const int32_t* __restrict__ label, const int32_t* __restrict__ rank, const int32_t* __restrict__ nf,
                                                              const int32_t* __restrict__ nv, int64_t V, int32_t* __restrict__ table, const int32_t* bad) {
    if (*bad) return;
    for (int64_t v = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; v < V; v += (int64_t)gridDim.x * MO_THREADS)
        if (label[v] == (int32_t)v) {
            const int64_t r = rank[v];
            table[3 * r] = (int32_t)v;
            table[3 * r + 1] = nf[v];
            table[3 * r + 2] = nv[v];
        }
}

// init | union | flatten into `label`; *bad must be zero before
static int mo_label(const int32_t* faces, int64_t V, int64_t F, int32_t* label, int32_t* bad, hipStream_t st) {
    hipLaunchKernelGGL(mo_init_kernel, dim3(mo_blocks(V)), dim3(MO_THREADS), 0, st, label, V);
    if (F > 0) hipLaunchKernelGGL(mo_union_kernel, dim3(mo_blocks(F)), dim3(MO_THREADS), 0, st, faces, V, F, label, bad);
    hipLaunchKernelGGL(mo_flatten_kernel, dim3(mo_blocks(V)), dim3(MO_THREADS), 0, st, label, V, (const int32_t*)bad);
    return sw_check(hipGetLastError(), "mesh label launches");
}

extern "C" int swnerf_mesh_components(const int32_t* faces, int64_t V, int64_t F, void* workspace, int32_t* vlabel, int32_t* table,
                                      int32_t* counts, void* stream) {
    int rc = mo_check("mesh_components", V, F);
    if (rc) return rc;
    if (!counts) return sw_fail(SWNERF_E_ARG, "mesh_components: NULL counts");
    hipStream_t st = (hipStream_t)stream;
    rc = sw_check(hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), st), "mesh_components memset");
    if (rc || V == 0) return rc;
    if (!workspace || !vlabel || !table || (F > 0 && !faces)) return sw_fail(SWNERF_E_ARG, "mesh_components: NULL pointer");
    const MoWs w = mo_ws(workspace, V, F);
    int32_t *nf = w.a0, *nv = w.a1, *isroot = w.a2;
    rc = sw_check(hipMemsetAsync(nf, 0, (char*)w.b0 - (char*)nf, st), "mesh_components memset");       // a0 | a1 | a2
    if (rc) return rc;
    rc = mo_label(faces, V, F, vlabel, counts + 1, st);
    if (rc) return rc;
    hipLaunchKernelGGL(mo_count_kernel, dim3(mo_blocks(V > F ? V : F)), dim3(MO_THREADS), 0, st, faces, (const int32_t*)vlabel, V, F, nf, nv, isroot,
                       (const int32_t*)(counts + 1));
    rc = mo_scan(isroot, isroot, V, w.tsum, counts, st);
    if (rc) return rc;
    hipLaunchKernelGGL(mo_table_kernel, dim3(mo_blocks(V)), dim3(MO_THREADS), 0, st, (const int32_t*)vlabel, (const int32_t*)isroot, (const int32_t*)nf,
                       (const int32_t*)nv, V, table, (const int32_t*)(counts + 1));
    return sw_check(hipGetLastError(), "mesh_components launch");
}

// ---- compaction --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool mo_in_list(const int32_t* __restrict__ kept, int n, int32_t x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (kept[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo < n && kept[lo] == x;
}

__global__ __launch_bounds__(MO_THREADS) void mo_mark_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ label, int64_t V, int64_t F,
                                                             const int32_t* __restrict__ kept, int nkept, int32_t* __restrict__ vflag, int32_t* __restrict__ fflag) {
    const int64_t n = V > F ? V : F;
    for (int64_t i = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * MO_THREADS) {
        if (i < V) vflag[i] = mo_in_list(kept, nkept, label[i]);
        if (i < F) {
            const int32_t a = faces[3 * i], b = faces[3 * i + 1], c = faces[3 * i + 2];
            fflag[i] = meshops_index_ok(a, V) && meshops_index_ok(b, V) && meshops_index_ok(c, V) && mo_in_list(kept, nkept, label[a]);
        }
    }
}

struct MoCompact {
    const float *verts, *normals, *colors;
    const int32_t* faces;
    float *verts_out, *normals_out, *colors_out;
    int32_t* faces_out;
    int64_t V, F, V_out, F_out;
};

// vmap / fpos: the exclusive scans of the flags (mo_kept)
__global__ __launch_bounds__(MO_THREADS) void mo_compact_kernel(MoCompact c, const int32_t* __restrict__ vmap, const int32_t* __restrict__ fpos) {
    const int64_t n = c.V > c.F ? c.V : c.F;
    for (int64_t i = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * MO_THREADS) {
        if (i < c.V && mo_kept(vmap, i, c.V_out)) mo_copy_row(c.verts, c.normals, c.colors, i, c.verts_out, c.normals_out, c.colors_out, vmap[i]);
        if (i < c.F && mo_kept(fpos, i, c.F_out)) {
            const int64_t o = fpos[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) c.faces_out[3 * o + k] = vmap[c.faces[3 * i + k]];   // in range: mo_mark_kernel checked the face
        }
    }
}

extern "C" int swnerf_mesh_compact(const float* verts, const int32_t* faces, const float* normals, const float* colors,
                                   const int32_t* vlabel, int64_t V, int64_t F, const int32_t* kept, int64_t n_kept, void* workspace,
                                   int64_t V_out, int64_t F_out, float* verts_out, int32_t* faces_out, float* normals_out,
                                   float* colors_out, void* stream) {
    int rc = mo_check("mesh_compact", V, F);
    if (rc) return rc;
    if (n_kept < 0 || n_kept > V || V_out < 0 || V_out > V || F_out < 0 || F_out > F)
        return sw_fail(SWNERF_E_ARG, "mesh_compact: n_kept = %lld, V_out = %lld, F_out = %lld do not fit V = %lld, F = %lld", (long long)n_kept,
                       (long long)V_out, (long long)F_out, (long long)V, (long long)F);
    if (V == 0 || n_kept == 0 || V_out == 0) return 0;
    if (!workspace || !verts || !vlabel || !kept || !verts_out || (F > 0 && !faces) || (F_out > 0 && !faces_out) || (normals && !normals_out) ||
        (colors && !colors_out))
        return sw_fail(SWNERF_E_ARG, "mesh_compact: NULL pointer");
    const MoWs w = mo_ws(workspace, V, F);
    int32_t *vflag = w.a0, *fflag = w.b0;
    hipStream_t st = (hipStream_t)stream;
    rc = sw_check(hipMemsetAsync(vflag + V, 0, sizeof(int32_t), st), "mesh_compact memset");
    if (!rc) rc = sw_check(hipMemsetAsync(fflag + F, 0, sizeof(int32_t), st), "mesh_compact memset");
    if (rc) return rc;
    const unsigned blocks = mo_blocks(V > F ? V : F);
    hipLaunchKernelGGL(mo_mark_kernel, dim3(blocks), dim3(MO_THREADS), 0, st, faces, vlabel, V, F, kept, (int)n_kept, vflag, fflag);
    rc = mo_scan(vflag, vflag, V + 1, w.tsum, nullptr, st);
    if (!rc) rc = mo_scan(fflag, fflag, F + 1, w.tsum, nullptr, st);
    if (rc) return rc;
    MoCompact c{verts, normals, colors, faces, verts_out, normals_out, colors_out, faces_out, V, F, V_out, F_out};
    hipLaunchKernelGGL(mo_compact_kernel, dim3(blocks), dim3(MO_THREADS), 0, st, c, (const int32_t*)vflag, (const int32_t*)fflag);
    return sw_check(hipGetLastError(), "mesh_compact launch");
}

// ---- incidence ---------------------------------------------------------------------------------------------------------
// the first reader of `faces` of this call
__global__ __launch_bounds__(MO_THREADS) void mo_valence_kernel(const int32_t* __restrict__ faces, int64_t V, int64_t n_corners, int32_t* cnt, int32_t* bad) {
    for (int64_t c = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; c < n_corners; c += (int64_t)gridDim.x * MO_THREADS) {
        const int32_t v = faces[c];
        if (meshops_index_ok(v, V)) atomicAdd(cnt + v, 1); else atomicAdd(bad, 1);
    }
}

__global__ __launch_bounds__(MO_THREADS) void mo_fill_kernel(const int32_t* __restrict__ faces, int64_t n_corners, const int32_t* __restrict__ offsets,
                                                             int32_t* cursor, int32_t* __restrict__ items, const int32_t* bad) {
    if (*bad) return;
    for (int64_t c = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; c < n_corners; c += (int64_t)gridDim.x * MO_THREADS) {
        const int32_t v = faces[c];
        items[offsets[v] + atomicAdd(cursor + v, 1)] = (int32_t)c;
    }
}

__device__ __forceinline__ void mo_sift_down(int32_t* a, int32_t i, int32_t n) {
    for (;;) {
        int32_t m = 2 * i + 1;
        if (m >= n) return;
        if (m + 1 < n && a[m + 1] > a[m]) ++m;
        if (a[i] >= a[m]) return;
        const int32_t t = a[i]; a[i] = a[m]; a[m] = t;
        i = m;
    }
}

// one thread per slice, in place: no per-thread array, any length
__global__ __launch_bounds__(MO_THREADS) void mo_sort_kernel(const int32_t* __restrict__ offsets, int64_t V, int32_t* items, const int32_t* bad) {
    if (*bad) return;
    for (int64_t v = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; v < V; v += (int64_t)gridDim.x * MO_THREADS) {
        int32_t* a = items + offsets[v];
        const int32_t n = offsets[v + 1] - offsets[v];
        if (n <= MO_SORT_SMALL) {
            for (int32_t i = 1; i < n; ++i) {
                const int32_t x = a[i];
                int32_t j = i - 1;
                for (; j >= 0 && a[j] > x; --j) a[j + 1] = a[j];
                a[j + 1] = x;
            }
        } else {
            for (int32_t i = n / 2 - 1; i >= 0; --i) mo_sift_down(a, i, n);
            for (int32_t m = n - 1; m > 0; --m) {
                const int32_t t = a[0]; a[0] = a[m]; a[m] = t;
                mo_sift_down(a, 0, m);
            }
        }
    }
}

int mo_csr(const int32_t* key, int64_t V, int64_t n, int32_t* cnt, int32_t* offsets, int32_t* items, int32_t* tsum, int32_t* out_of_range, int32_t* bad,
           bool sorted, hipStream_t st) {
    int rc = sw_check(hipMemsetAsync(cnt, 0, (V + 1) * sizeof(int32_t), st), "mesh csr memset");
    if (rc) return rc;
    hipLaunchKernelGGL(mo_valence_kernel, dim3(mo_blocks(n)), dim3(MO_THREADS), 0, st, key, V, n, cnt, out_of_range);
    rc = mo_scan(cnt, offsets, V + 1, tsum, nullptr, st);
    if (!rc) rc = sw_check(hipMemsetAsync(cnt, 0, (V + 1) * sizeof(int32_t), st), "mesh csr memset");
    if (rc) return rc;
    hipLaunchKernelGGL(mo_fill_kernel, dim3(mo_blocks(n)), dim3(MO_THREADS), 0, st, key, n, (const int32_t*)offsets, cnt, items, (const int32_t*)bad);
    if (sorted) hipLaunchKernelGGL(mo_sort_kernel, dim3(mo_blocks(V)), dim3(MO_THREADS), 0, st, (const int32_t*)offsets, V, items, (const int32_t*)bad);
    return sw_check(hipGetLastError(), "mesh csr launches");
}

extern "C" int swnerf_mesh_incidence(const int32_t* faces, int64_t V, int64_t F, void* workspace, int32_t* offsets, int32_t* items,
                                     int32_t* status, void* stream) {
    int rc = mo_check("mesh_incidence", V, F);
    if (rc) return rc;
    if (!status || !offsets) return sw_fail(SWNERF_E_ARG, "mesh_incidence: NULL offsets / status");
    hipStream_t st = (hipStream_t)stream;
    rc = sw_check(hipMemsetAsync(status, 0, sizeof(int32_t), st), "mesh_incidence memset");
    if (!rc) rc = sw_check(hipMemsetAsync(offsets, 0, (V + 1) * sizeof(int32_t), st), "mesh_incidence memset");
    if (rc || V == 0 || F == 0) return rc;
    if (!workspace || !faces || !items) return sw_fail(SWNERF_E_ARG, "mesh_incidence: NULL pointer");
    const MoWs w = mo_ws(workspace, V, F);
    return mo_csr(faces, V, 3 * F, w.a0, offsets, items, w.tsum, status, status, true, st);
}

// ---- smoothing and normals ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MO_THREADS) void mo_smooth_kernel(const float* __restrict__ P, const int32_t* __restrict__ faces, const int32_t* __restrict__ offsets,
                                                               const int32_t* __restrict__ items, int64_t V, int64_t F, float s, float* __restrict__ out) {
    for (int64_t v = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; v < V; v += (int64_t)gridDim.x * MO_THREADS) {
        float o[3];
        meshops_smooth_vertex(P, faces, items, offsets[v], offsets[v + 1], v, V, F, s, o);
        out[3 * v] = o[0]; out[3 * v + 1] = o[1]; out[3 * v + 2] = o[2];
    }
}

__global__ __launch_bounds__(MO_THREADS) void mo_normals_kernel(const float* __restrict__ P, const int32_t* __restrict__ faces, const int32_t* __restrict__ offsets,
                                                                const int32_t* __restrict__ items, int64_t V, int64_t F, float* __restrict__ out) {
    for (int64_t v = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; v < V; v += (int64_t)gridDim.x * MO_THREADS) {
        float o[3];
        meshops_vertex_normal(P, faces, items, offsets[v], offsets[v + 1], V, F, o);
        out[3 * v] = o[0]; out[3 * v + 1] = o[1]; out[3 * v + 2] = o[2];
    }
}

static int mo_check_csr(const char* what, int64_t V, int64_t F, const void* verts, const void* faces, const void* offsets, const void* items, const void* out) {
    int rc = mo_check(what, V, F);
    if (rc) return rc;
    if (V > 0 && (!verts || !offsets || !out)) return sw_fail(SWNERF_E_ARG, "%s: NULL pointer", what);
    if (V > 0 && F > 0 && (!faces || !items)) return sw_fail(SWNERF_E_ARG, "%s: NULL faces / items", what);
    return 0;
}

extern "C" int swnerf_mesh_smooth_step(const float* verts, const int32_t* faces, const int32_t* offsets, const int32_t* items, int64_t V,
                                       int64_t F, float s, float* out, void* stream) {
    int rc = mo_check_csr("mesh_smooth_step", V, F, verts, faces, offsets, items, out);
    if (rc || V == 0) return rc;
    if (out == verts) return sw_fail(SWNERF_E_ARG, "mesh_smooth_step: out must not be verts (every vertex reads its neighbours' old positions)");
    hipLaunchKernelGGL(mo_smooth_kernel, dim3(mo_blocks(V)), dim3(MO_THREADS), 0, (hipStream_t)stream, verts, faces, offsets, items, V, F, s, out);
    return sw_check(hipGetLastError(), "mesh_smooth_step launch");
}

extern "C" int swnerf_mesh_vertex_normals(const float* verts, const int32_t* faces, const int32_t* offsets, const int32_t* items, int64_t V,
                                          int64_t F, float* normals, void* stream) {
    int rc = mo_check_csr("mesh_vertex_normals", V, F, verts, faces, offsets, items, normals);
    if (rc || V == 0) return rc;
    hipLaunchKernelGGL(mo_normals_kernel, dim3(mo_blocks(V)), dim3(MO_THREADS), 0, (hipStream_t)stream, verts, faces, offsets, items, V, F, normals);
    return sw_check(hipGetLastError(), "mesh_vertex_normals launch");
}

// ---- measurement -------------------------------------------------------------------------------------------------------
enum { MO_C_VREF = 0, MO_C_EDGES, MO_C_BOUNDARY, MO_C_NONMANIFOLD, MO_C_COMPONENTS };

__global__ __launch_bounds__(MO_THREADS) void mo_measure_init_kernel(MoWs w) {
    if (threadIdx.x < 3) w.bbox[threadIdx.x] = MO_KEY_POS_INF;
    else if (threadIdx.x < 6) w.bbox[threadIdx.x] = MO_KEY_NEG_INF;
    if (threadIdx.x < 8) w.cnt[threadIdx.x] = 0ull;
    if (threadIdx.x == 0) w.status[0] = 0;
}

// referenced vertices: their count and bounding box; mark[label of a face's first vertex] = 1 (every writer stores the same 1)
__global__ __launch_bounds__(MO_THREADS) void mo_measure_verts_kernel(const float* __restrict__ P, const int32_t* __restrict__ faces, const int32_t* __restrict__ offsets,
                                                                      const int32_t* __restrict__ label, int64_t V, int64_t F, int32_t* mark, MoWs w) {
    if (w.status[0]) return;
    __shared__ uint32_t box[6];
    if (threadIdx.x < 6) box[threadIdx.x] = threadIdx.x < 3 ? MO_KEY_POS_INF : MO_KEY_NEG_INF;
    __syncthreads();
    const int64_t n = V > F ? V : F;
    unsigned long long nref = 0;
    for (int64_t i = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * MO_THREADS) {
        if (i < V && offsets[i + 1] > offsets[i]) {
            ++nref;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const uint32_t key = meshops_float_key(P[3 * i + k]);
                atomicMin(box + k, key);
                atomicMax(box + 3 + k, key);
            }
        }
        if (i < F) mark[label[faces[3 * i]]] = 1;
    }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(w.bbox + threadIdx.x, box[threadIdx.x]);
    else if (threadIdx.x < 6) atomicMax(w.bbox + threadIdx.x, box[threadIdx.x]);
    wave_count(w.cnt + MO_C_VREF, nref);
}

// one thread per corner: its edge's occurrences from the slice of the end point of lower valence; counted at the smallest corner id
__global__ __launch_bounds__(MO_THREADS) void mo_measure_edges_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ offsets,
                                                                      const int32_t* __restrict__ items, const int32_t* __restrict__ mark, int64_t V, int64_t F, MoWs w) {
    if (w.status[0]) return;
    unsigned long long ne = 0, nb = 0, nm = 0, nc = 0;
    const int64_t n = 3 * F > V ? 3 * F : V;
    for (int64_t i = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * MO_THREADS) {
        if (i < V) nc += mark[i] != 0;
        if (i >= 3 * F) continue;
        const int32_t c = (int32_t)i, f = c / 3, k = c - 3 * f;
        const int32_t a = faces[c], b = faces[3 * f + (k + 1) % 3];
        const int32_t la = offsets[a + 1] - offsets[a], lb = offsets[b + 1] - offsets[b];
        const bool from_a = la <= lb;
        const int32_t x = from_a ? a : b, y = from_a ? b : a;
        const MeshopsEdge e = meshops_edge_scan(faces, items, offsets[x], offsets[x + 1], x, y, F);
        if (e.first != c) continue;
        ++ne;
        nb += e.n_xy + e.n_yx == 1;
        nm += e.n_xy + e.n_yx > 2 || e.n_xy >= 2 || e.n_yx >= 2;
    }
    wave_count(w.cnt + MO_C_EDGES, ne);
    wave_count(w.cnt + MO_C_BOUNDARY, nb);
    wave_count(w.cnt + MO_C_NONMANIFOLD, nm);
    wave_count(w.cnt + MO_C_COMPONENTS, nc);
}

// thread t adds the 5 terms in the order given by `term(i, out)` for i = t, t + 256, ..; then the 256 sums are added in a fixed
// tree (lanes by shuffles, then the four waves in order): the result depends on n alone
template <typename Term>
__device__ __forceinline__ void mo_block_sum(int64_t lo, int64_t hi, Term term, double* lds, double* out) {
    double s[MESHOPS_FACE_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = lo + threadIdx.x; i < hi; i += MO_THREADS) {
        double t[MESHOPS_FACE_TERMS];
        term(i, t);
#pragma unroll
        for (int q = 0; q < MESHOPS_FACE_TERMS; ++q) s[q] += t[q];
    }
#pragma unroll
    for (int q = 0; q < MESHOPS_FACE_TERMS; ++q) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s[q] += __shfl_down(s[q], d, 64);
        if ((threadIdx.x & 63) == 0) lds[(threadIdx.x >> 6) * MESHOPS_FACE_TERMS + q] = s[q];
    }
    __syncthreads();
    if (threadIdx.x < MESHOPS_FACE_TERMS) {
        double r = 0.0;
        for (int wv = 0; wv < MO_THREADS / 64; ++wv) r += lds[wv * MESHOPS_FACE_TERMS + threadIdx.x];
        out[threadIdx.x] = r;
    }
}

// workgroup b sums the faces [b per, (b + 1) per): a partition that depends on F alone
__global__ __launch_bounds__(MO_THREADS) void mo_measure_faces_kernel(const float* __restrict__ P, const int32_t* __restrict__ faces, int64_t F, int64_t per, MoWs w) {
    __shared__ double lds[(MO_THREADS / 64) * MESHOPS_FACE_TERMS];
    const bool stop = w.status[0] != 0;
    const int64_t lo = blockIdx.x * per, hi = stop ? lo : (lo + per < F ? lo + per : F);
    mo_block_sum(lo, hi, [&](int64_t f, double* t) {
        meshops_face_terms(P + 3 * (int64_t)faces[3 * f], P + 3 * (int64_t)faces[3 * f + 1], P + 3 * (int64_t)faces[3 * f + 2], t);
    }, lds, w.part + (int64_t)blockIdx.x * MESHOPS_FACE_TERMS);
}

__global__ __launch_bounds__(MO_THREADS) void mo_measure_final_kernel(int64_t F, int nparts, MoWs w, double* __restrict__ values, int64_t* __restrict__ counts) {
    __shared__ double lds[(MO_THREADS / 64) * MESHOPS_FACE_TERMS];
    const bool stop = w.status[0] != 0;
    if (threadIdx.x < 16) values[threadIdx.x] = 0.0;
    __syncthreads();
    mo_block_sum(0, stop ? 0 : nparts, [&](int64_t b, double* t) {
#pragma unroll
        for (int q = 0; q < MESHOPS_FACE_TERMS; ++q) t[q] = w.part[b * MESHOPS_FACE_TERMS + q];
    }, lds, values);
    if (threadIdx.x < 6) values[5 + threadIdx.x] = (double)meshops_key_float(w.bbox[threadIdx.x]);
    if (threadIdx.x == 0) {
        const int64_t vref = (int64_t)w.cnt[MO_C_VREF], e = (int64_t)w.cnt[MO_C_EDGES], nb = (int64_t)w.cnt[MO_C_BOUNDARY], nm = (int64_t)w.cnt[MO_C_NONMANIFOLD];
        counts[0] = vref; counts[1] = e; counts[2] = nb; counts[3] = nm;
        counts[4] = (int64_t)w.cnt[MO_C_COMPONENTS];
        counts[5] = stop ? 0 : vref - e + F;
        counts[6] = !stop && nb == 0 && nm == 0;
        counts[7] = w.status[0];
    }
}

extern "C" int swnerf_mesh_measure(const float* verts, const int32_t* faces, const int32_t* offsets, const int32_t* items, int64_t V,
                                   int64_t F, void* workspace, double* values, int64_t* counts, void* stream) {
    int rc = mo_check_csr("mesh_measure", V, F, verts, faces, offsets, items, values);
    if (rc) return rc;
    if (!values || !counts || !workspace) return sw_fail(SWNERF_E_ARG, "mesh_measure: NULL values / counts / workspace");
    if (V == 0) F = 0;                                             // no vertex: no face can be valid, and none is read
    const MoWs w = mo_ws(workspace, V, F);
    int32_t *label = w.a0, *mark = w.a1;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mo_measure_init_kernel, dim3(1), dim3(MO_THREADS), 0, st, w);
    int nparts = 0;
    if (V > 0) {
        rc = sw_check(hipMemsetAsync(mark, 0, (V + 1) * sizeof(int32_t), st), "mesh_measure memset");
        if (!rc) rc = mo_label(faces, V, F, label, w.status, st);
        if (rc) return rc;
        hipLaunchKernelGGL(mo_measure_verts_kernel, dim3(mo_blocks(V > F ? V : F)), dim3(MO_THREADS), 0, st, verts, faces, offsets, (const int32_t*)label, V, F, mark, w);
        hipLaunchKernelGGL(mo_measure_edges_kernel, dim3(mo_blocks(3 * F > V ? 3 * F : V)), dim3(MO_THREADS), 0, st, faces, offsets, items, (const int32_t*)mark, V, F, w);
        if (F > 0) {
            const int64_t per = (F + MO_PARTS - 1) / MO_PARTS;
            nparts = (int)((F + per - 1) / per);
            hipLaunchKernelGGL(mo_measure_faces_kernel, dim3(nparts), dim3(MO_THREADS), 0, st, verts, faces, F, per, w);
        }
    }
    hipLaunchKernelGGL(mo_measure_final_kernel, dim3(1), dim3(MO_THREADS), 0, st, F, nparts, w, values, counts);
    return sw_check(hipGetLastError(), "mesh_measure launch");
}
