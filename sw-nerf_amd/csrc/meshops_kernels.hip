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
//   cluster, collapse, emit  welding and decimation by vertex clustering on a uniform grid (the second part of this file)
//   boundary, loops, fill    hole filling: boundary half-edges, loops by pointer jumping, fan caps (the last part of this file)
// Every phase is its own launch; a kernel after the first reader of `faces` returns at once when that one counted a bad index.
#include <hip/hip_runtime.h>
#include "../../include/swnerf.h"
#include "host_util.h"
#include "meshops_math.h"

#define MO_THREADS 256
#define MO_MAX_GRID 1024               // grid-stride cap
#define MO_SCAN_THREADS 1024
#define MO_PARTS 256                   // workgroups (= partial sums) of the fp64 face reduction
#define MO_KEY_POS_INF 0xFF800000u     // meshops_float_key of +inf and of -inf: the empty bounding box
#define MO_KEY_NEG_INF 0x007FFFFFu
#define MO_SORT_SMALL 16               // slices up to this length are sorted by insertion, longer ones by heap sort

static inline int64_t mo_round256(int64_t b) { return (b + 255) & ~(int64_t)255; }
static inline int64_t mo_tiles(int64_t n) { return (n + MO_THREADS - 1) / MO_THREADS; }
static inline unsigned mo_blocks(int64_t n) {
    const int64_t t = mo_tiles(n);
    return (unsigned)(t < 1 ? 1 : (t < MO_MAX_GRID ? t : MO_MAX_GRID));
}

static inline bool mo_sizes_ok(int64_t V, int64_t F) { return V >= 0 && V <= INT32_MAX && F >= 0 && F <= INT32_MAX / 3; }   // 3 F < 2^31

// workspace: three int32 [V+1] | one int32 [F+1] | tile sums int32 [tiles(max(V, F) + 1)] | 64 x 8 bytes of status and counters |
// fp64 partials [MO_PARTS, 5]
struct MoWs {
    int32_t *a0, *a1, *a2, *b0, *tsum;
    int32_t* status;                   // [0] bad indices of this call
    uint32_t* bbox;                    // [6] ordered keys: min xyz, max xyz (bytes 64..)
    unsigned long long* cnt;           // [8] integer counters (bytes 128..)
    double* part;
};

static MoWs mo_ws(void* ws, int64_t V, int64_t F) {
    char* p = (char*)ws;
    MoWs w;
    w.a0 = (int32_t*)p;  p += mo_round256(4 * (V + 1));
    w.a1 = (int32_t*)p;  p += mo_round256(4 * (V + 1));
    w.a2 = (int32_t*)p;  p += mo_round256(4 * (V + 1));
    w.b0 = (int32_t*)p;  p += mo_round256(4 * (F + 1));
    w.tsum = (int32_t*)p; p += mo_round256(4 * mo_tiles((V > F ? V : F) + 1));
    w.status = (int32_t*)p;
    w.bbox = (uint32_t*)(p + 64);
    w.cnt = (unsigned long long*)(p + 128);
    p += 512;
    w.part = (double*)p;
    return w;
}

extern "C" int64_t swnerf_mesh_workspace_bytes(int64_t V, int64_t F) {
    if (!mo_sizes_ok(V, F)) return 0;
    return 3 * mo_round256(4 * (V + 1)) + mo_round256(4 * (F + 1)) + mo_round256(4 * mo_tiles((V > F ? V : F) + 1)) + 512 +
           mo_round256(8 * MO_PARTS * MESHOPS_FACE_TERMS);
}

// ---- helpers -----------------------------------------------------------------------------------------------------------
// The union-find of marker_kernels.hip (mk_find / mk_union), restated here so that unit stays as it is.
__device__ __forceinline__ int mo_find(const int* L, int x) {
    int l;
    while ((l = __atomic_load_n(L + x, __ATOMIC_RELAXED)) != x) x = l;
    return x;
}

// link the larger root to the smaller until both ends share one
__device__ __forceinline__ void mo_union(int* L, int a, int b) {
    for (;;) {
        a = mo_find(L, a);
        b = mo_find(L, b);
        if (a == b) return;
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(L + b, a);                       // a < b
        if (old == b) return;
        b = old;
    }
}

// The block scan of mesh_kernels.hip: wave prefix by shuffles, then the wave totals in order.
template <typename T, int NT>
__device__ __forceinline__ T mo_block_exclusive_scan(T x, T* lds, T* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T inc = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(inc, d, 64);
        if (lane >= d) inc += y;
    }
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    T pre = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < NT / 64; ++q) {
        const T s = lds[q];
        pre += (q < w) ? s : (T)0;
        tot += s;
    }
    __syncthreads();                   // lds may be reused by the next call
    *total = tot;
    return pre + inc - x;
}

// Add 1 to cnt[key] for every lane with key >= 0.  The lanes of a wave mostly name one component: those that share the first
// active lane's key issue one atomic between them (integer sums do not depend on the grouping).
__device__ __forceinline__ void mo_count_key(int32_t* cnt, int key) {
    const bool on = key >= 0;
    const unsigned long long act = __ballot(on);
    if (!act) return;
    const int first = __shfl(key, __ffsll((long long)act) - 1, 64);
    const unsigned long long same = __ballot(on && key == first);
    const int lane = threadIdx.x & 63;
    if (on && key == first) {
        if (lane == __ffsll((long long)same) - 1) atomicAdd(cnt + key, __popcll(same));
    } else if (on) {
        atomicAdd(cnt + key, 1);
    }
}

// one atomic per wave for a per-thread count (every lane of the wave must call)
__device__ __forceinline__ void mo_wave_add(unsigned long long* dst, unsigned long long x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d, 64);
    if ((threadIdx.x & 63) == 0 && x) atomicAdd(dst, x);
}

// ---- exclusive scan of an int32 array: tile sums | one workgroup over the tile sums | tiles again ---------------------------------
__global__ __launch_bounds__(MO_THREADS) void mo_tile_sum_kernel(const int32_t* __restrict__ cnt, int64_t n, int64_t ntiles, int32_t* __restrict__ tsum) {
    __shared__ int32_t lds[MO_THREADS / 64];
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t i = tile * MO_THREADS + threadIdx.x;
        int32_t tot;
        mo_block_exclusive_scan<int32_t, MO_THREADS>(i < n ? cnt[i] : 0, lds, &tot);
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
    int32_t o = mo_block_exclusive_scan<int32_t, MO_SCAN_THREADS>(s, lds, &tot);
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
        const int32_t ex = mo_block_exclusive_scan<int32_t, MO_THREADS>(i < n ? cnt[i] : 0, lds, &tot);
        if (i < n) off[i] = tsum[tile] + ex;
    }
}

// off[i] = sum of cnt[0 .. i) for i < n; *total (may be NULL) = the sum of all n.  Three launches.
static int mo_scan(const int32_t* cnt, int32_t* off, int64_t n, int32_t* tsum, int32_t* total, hipStream_t st) {
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
        mo_union(label, a, b);
        mo_union(label, b, c);
    }
}

__global__ __launch_bounds__(MO_THREADS) void mo_flatten_kernel(int32_t* label, int64_t V, const int32_t* bad) {
    if (*bad) return;
    for (int64_t v = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; v < V; v += (int64_t)gridDim.x * MO_THREADS) {
        const int root = mo_find(label, (int)v);
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

static int mo_check(const char* what, int64_t V, int64_t F) {
    if (!mo_sizes_ok(V, F))
        return sw_fail(SWNERF_E_ARG, "%s: V = %lld, F = %lld: need 0 <= V < 2^31 and 0 <= 3 F < 2^31 (corner ids are int32)", what, (long long)V, (long long)F);
    return 0;
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
    rc = sw_check(hipMemsetAsync(workspace, 0, 3 * mo_round256(4 * (V + 1)), st), "mesh_components memset");
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

// vmap / fpos: the exclusive scans of the flags, so element i is kept iff its scan value differs from the next one's
__global__ __launch_bounds__(MO_THREADS) void mo_compact_kernel(MoCompact c, const int32_t* __restrict__ vmap, const int32_t* __restrict__ fpos) {
    const int64_t n = c.V > c.F ? c.V : c.F;
    for (int64_t i = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * MO_THREADS) {
        if (i < c.V && vmap[i + 1] != vmap[i] && vmap[i] < c.V_out) {
            const int64_t o = vmap[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                c.verts_out[3 * o + k] = c.verts[3 * i + k];
                if (c.normals) c.normals_out[3 * o + k] = c.normals[3 * i + k];
                if (c.colors) c.colors_out[3 * o + k] = c.colors[3 * i + k];
            }
        }
        if (i < c.F && fpos[i + 1] != fpos[i] && fpos[i] < c.F_out) {
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
    int32_t* cnt = w.a0;
    rc = sw_check(hipMemsetAsync(cnt, 0, (V + 1) * sizeof(int32_t), st), "mesh_incidence memset");
    if (rc) return rc;
    hipLaunchKernelGGL(mo_valence_kernel, dim3(mo_blocks(3 * F)), dim3(MO_THREADS), 0, st, faces, V, 3 * F, cnt, status);
    rc = mo_scan(cnt, offsets, V + 1, w.tsum, nullptr, st);
    if (!rc) rc = sw_check(hipMemsetAsync(cnt, 0, (V + 1) * sizeof(int32_t), st), "mesh_incidence memset");
    if (rc) return rc;
    hipLaunchKernelGGL(mo_fill_kernel, dim3(mo_blocks(3 * F)), dim3(MO_THREADS), 0, st, faces, 3 * F, (const int32_t*)offsets, cnt, items, (const int32_t*)status);
    hipLaunchKernelGGL(mo_sort_kernel, dim3(mo_blocks(V)), dim3(MO_THREADS), 0, st, (const int32_t*)offsets, V, items, (const int32_t*)status);
    return sw_check(hipGetLastError(), "mesh_incidence launch");
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
    mo_wave_add(w.cnt + MO_C_VREF, nref);
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
    mo_wave_add(w.cnt + MO_C_EDGES, ne);
    mo_wave_add(w.cnt + MO_C_BOUNDARY, nb);
    mo_wave_add(w.cnt + MO_C_NONMANIFOLD, nm);
    mo_wave_add(w.cnt + MO_C_COMPONENTS, nc);
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

// ---- vertex clustering: welding and decimation -------------------------------------------------------------------------------------
//   cluster   origin (integer atomics on ordered keys, unless given) | insert: an open-addressing table of the 64-bit cell keys,
//             a slot claimed by atomicCAS takes the atomicMin of its vertices | label = the slot's minimum; roots are counted
//   collapse  labels of the corners (the first reader of `faces`) | the corner list per label (count | scan | fill; left unsorted) |
//             per face: degenerate, duplicate (a scan of the whole slice of its label with the fewest corners) or kept, kept faces
//             mark their labels | two scans | a guarded copy to the outputs
//   emit      labels of the corners | faces through vmap | WELD: copy rows; MEAN / QUADRIC: member list per label, QUADRIC also the
//             corner list, then one thread per output vertex over its sorted slices (meshops_place_vertex)
// The table decides only which slot a key sits in: every result is a minimum or a count, so nothing depends on the arrival order.
#define MS_MIN_CAPACITY 64

static inline int64_t ms_capacity(int64_t V) {
    int64_t c = MS_MIN_CAPACITY;
    while (c < 2 * V) c <<= 1;
    return c;
}

// workspace: table keys uint64 [cap] | table minima uint32 [cap] | five int32 [V+1] | two int32 [3F+1] | face flags int32 [F+1] |
// tile sums | 512 bytes of status, origin keys and origin.  mesh_cluster uses the layout of (V, 0): the table and the slots.
struct MsWs {
    unsigned long long* tkey;
    uint32_t *tmin, *slot;
    int32_t *cnt, *off, *moff, *mitems, *gl, *items, *fflag, *tsum;
    int32_t* status;                   // [0] bad face indices, [1] invalid vertices, [2] table overflow
    uint32_t* okey;                    // [3] ordered keys of the per-axis minimum (bytes 64..)
    float* origin;                     // [3] the origin in use (bytes 128..)
    int64_t cap;
};

static MsWs ms_ws(void* ws, int64_t V, int64_t F) {
    char* p = (char*)ws;
    MsWs w;
    w.cap = ms_capacity(V);
    w.tkey = (unsigned long long*)p; p += 8 * w.cap;
    w.tmin = (uint32_t*)p;           p += 4 * w.cap;
    w.slot = (uint32_t*)p;  p += mo_round256(4 * (V + 1));
    w.cnt = (int32_t*)p;    p += mo_round256(4 * (V + 1));
    w.off = (int32_t*)p;    p += mo_round256(4 * (V + 1));
    w.moff = (int32_t*)p;   p += mo_round256(4 * (V + 1));
    w.mitems = (int32_t*)p; p += mo_round256(4 * (V + 1));
    w.gl = (int32_t*)p;     p += mo_round256(4 * (3 * F + 1));
    w.items = (int32_t*)p;  p += mo_round256(4 * (3 * F + 1));
    w.fflag = (int32_t*)p;  p += mo_round256(4 * (F + 1));
    w.tsum = (int32_t*)p;   p += mo_round256(4 * mo_tiles((V > F ? V : F) + 1));
    w.status = (int32_t*)p;
    w.okey = (uint32_t*)(p + 64);
    w.origin = (float*)(p + 128);
    return w;
}

extern "C" int64_t swnerf_mesh_simplify_workspace_bytes(int64_t V, int64_t F) {
    if (!mo_sizes_ok(V, F)) return 0;
    return 12 * ms_capacity(V) + 5 * mo_round256(4 * (V + 1)) + 2 * mo_round256(4 * (3 * F + 1)) + mo_round256(4 * (F + 1)) +
           mo_round256(4 * mo_tiles((V > F ? V : F) + 1)) + 512;
}

// one atomic per wave for a per-thread count into an int32 status or count word (every lane of the wave must call)
__device__ __forceinline__ void ms_wave_count(int32_t* dst, unsigned long long x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d, 64);
    if ((threadIdx.x & 63) == 0 && x) atomicAdd(dst, (int32_t)x);
}

__global__ __launch_bounds__(MO_THREADS) void ms_init_kernel(MsWs w, const float* __restrict__ origin) {
    if (threadIdx.x < 16) w.status[threadIdx.x] = 0;
    if (threadIdx.x < 3) {
        w.okey[threadIdx.x] = MO_KEY_POS_INF;
        w.origin[threadIdx.x] = origin ? origin[threadIdx.x] : 0.f;
    }
}

__global__ __launch_bounds__(MO_THREADS) void ms_origin_kernel(const float* __restrict__ P, int64_t V, MsWs w) {
    __shared__ uint32_t box[3];
    if (threadIdx.x < 3) box[threadIdx.x] = MO_KEY_POS_INF;
    __syncthreads();
    uint32_t k0 = MO_KEY_POS_INF, k1 = MO_KEY_POS_INF, k2 = MO_KEY_POS_INF;
    for (int64_t v = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; v < V; v += (int64_t)gridDim.x * MO_THREADS) {
        const uint32_t a = meshops_float_key(P[3 * v]), b = meshops_float_key(P[3 * v + 1]), c = meshops_float_key(P[3 * v + 2]);
        k0 = a < k0 ? a : k0;
        k1 = b < k1 ? b : k1;
        k2 = c < k2 ? c : k2;
    }
    atomicMin(box, k0);
    atomicMin(box + 1, k1);
    atomicMin(box + 2, k2);
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(w.okey + threadIdx.x, box[threadIdx.x]);
}

__global__ __launch_bounds__(MO_THREADS) void ms_origin_final_kernel(MsWs w) {
    if (threadIdx.x < 3) w.origin[threadIdx.x] = meshops_key_float(w.okey[threadIdx.x]);
}

// Claim or find the slot of `key`: at most `cap` probes, never a wait on another thread.  -1: the table is full.
__device__ __forceinline__ int64_t ms_find_slot(unsigned long long* tkey, int64_t cap, unsigned long long key) {
    int64_t s = (int64_t)(meshops_key_hash(key) & (uint64_t)(cap - 1));
    for (int64_t step = 0; step < cap; ++step) {
        unsigned long long cur = __atomic_load_n(tkey + s, __ATOMIC_RELAXED);
        if (cur == MESHOPS_NO_CELL) cur = atomicCAS(tkey + s, (unsigned long long)MESHOPS_NO_CELL, key);
        if (cur == MESHOPS_NO_CELL || cur == key) return s;
        s = (s + 1) & (cap - 1);
    }
    return -1;
}

// One key per lane.  With a coarse cell the lanes of a wave mostly share one cell: those that share the first valid lane's key
// send one probe and one atomicMin between them (its lowest lane holds the smallest vertex index of the group).  Whole waves loop
// together (shuffles), so the bound is rounded up to the block.
__global__ __launch_bounds__(MO_THREADS) void ms_insert_kernel(const float* __restrict__ P, int64_t V, float h, MsWs w) {
    const int lane = threadIdx.x & 63;
    unsigned long long ninvalid = 0, nfull = 0;
    const float o[3] = {w.origin[0], w.origin[1], w.origin[2]};
    for (int64_t v0 = (int64_t)blockIdx.x * MO_THREADS; v0 < V; v0 += (int64_t)gridDim.x * MO_THREADS) {
        const int64_t v = v0 + threadIdx.x;
        unsigned long long key = MESHOPS_NO_CELL;
        if (v < V) {
            const float p[3] = {P[3 * v], P[3 * v + 1], P[3 * v + 2]};
            key = meshops_cell_key(p, o, h, nullptr);
            ninvalid += key == MESHOPS_NO_CELL;
        }
        const bool on = key != MESHOPS_NO_CELL;
        const unsigned long long act = __ballot(on);
        if (!act) continue;
        const int first = __ffsll((long long)act) - 1;
        const unsigned long long fkey = __shfl(key, first, 64);
        const bool grouped = on && key == fkey;
        long long s = 0;
        if (on && (!grouped || lane == first)) {
            s = ms_find_slot(w.tkey, w.cap, key);
            if (s >= 0) atomicMin(w.tmin + s, (uint32_t)v);
            else {
                ++nfull;
                s = 0;
            }
        }
        const long long fs = __shfl(s, first, 64);
        if (grouped) s = fs;
        if (on) w.slot[v] = (uint32_t)s;      // cap <= 2^32 slots
    }
    ms_wave_count(w.status + 1, ninvalid);
    ms_wave_count(w.status + 2, nfull);
}

// vlabel = the minimum of the vertex's slot; nothing is written when a vertex had no cell (or the table overflowed)
__global__ __launch_bounds__(MO_THREADS) void ms_label_kernel(int64_t V, MsWs w, int32_t* __restrict__ vlabel, float* __restrict__ origin_out, int32_t* counts) {
    const bool stop = w.status[1] != 0 || w.status[2] != 0;
    if (blockIdx.x == 0 && threadIdx.x < 2) counts[1 + threadIdx.x] = w.status[1 + threadIdx.x];
    if (stop) return;
    if (blockIdx.x == 0 && threadIdx.x < 3) origin_out[threadIdx.x] = w.origin[threadIdx.x];
    unsigned long long nroot = 0;
    for (int64_t v = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; v < V; v += (int64_t)gridDim.x * MO_THREADS) {
        const int32_t l = (int32_t)w.tmin[w.slot[v]];
        vlabel[v] = l;
        nroot += l == (int32_t)v;
    }
    ms_wave_count(counts, nroot);
}

extern "C" int swnerf_mesh_cluster(const float* verts, int64_t V, const float* origin, float cell, void* workspace, int32_t* vlabel,
                                   float* origin_out, int32_t* counts, void* stream) {
    int rc = mo_check("mesh_cluster", V, 0);
    if (rc) return rc;
    if (!(cell > 0.f) || !(cell - cell == 0.f)) return sw_fail(SWNERF_E_ARG, "mesh_cluster: the cell size must be finite and positive, got %g", (double)cell);
    if (!counts) return sw_fail(SWNERF_E_ARG, "mesh_cluster: NULL counts");
    hipStream_t st = (hipStream_t)stream;
    rc = sw_check(hipMemsetAsync(counts, 0, 3 * sizeof(int32_t), st), "mesh_cluster memset");
    if (rc || V == 0) return rc;
    if (!workspace || !verts || !vlabel || !origin_out) return sw_fail(SWNERF_E_ARG, "mesh_cluster: NULL pointer");
    const MsWs w = ms_ws(workspace, V, 0);
    rc = sw_check(hipMemsetAsync(w.tkey, 0xFF, 12 * w.cap, st), "mesh_cluster memset");      // keys: empty; minima: 2^32 - 1
    if (rc) return rc;
    hipLaunchKernelGGL(ms_init_kernel, dim3(1), dim3(MO_THREADS), 0, st, w, origin);
    if (!origin) {
        hipLaunchKernelGGL(ms_origin_kernel, dim3(mo_blocks(V)), dim3(MO_THREADS), 0, st, verts, V, w);
        hipLaunchKernelGGL(ms_origin_final_kernel, dim3(1), dim3(64), 0, st, w);
    }
    hipLaunchKernelGGL(ms_insert_kernel, dim3(mo_blocks(V)), dim3(MO_THREADS), 0, st, verts, V, cell, w);
    hipLaunchKernelGGL(ms_label_kernel, dim3(mo_blocks(V)), dim3(MO_THREADS), 0, st, V, w, vlabel, origin_out, counts);
    return sw_check(hipGetLastError(), "mesh_cluster launch");
}

// the first reader of `faces` (and of `vlabel`): gl[c] = vlabel[faces[c]]; an index or a label outside 0..V-1 is counted, not followed
__global__ __launch_bounds__(MO_THREADS) void ms_corner_label_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ vlabel, int64_t V,
                                                                     int64_t n_corners, int32_t* __restrict__ gl, int32_t* bad) {
    unsigned long long nbad = 0;
    for (int64_t c = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; c < n_corners; c += (int64_t)gridDim.x * MO_THREADS) {
        const int32_t a = faces[c];
        const int32_t l = meshops_index_ok(a, V) ? vlabel[a] : -1;
        const bool ok = meshops_index_ok(l, V);
        gl[c] = ok ? l : -1;
        nbad += !ok;
    }
    ms_wave_count(bad, nbad);
}

// CSR of the values key[0 .. n) per value: offsets [V+1], items ascending when `sorted` (else in the order the atomics landed, for
// a reader that does not care).  The incidence construction again: a value outside 0..V-1 is counted into *out_of_range, and the
// fill and the sort return at once when *bad is set.
static int ms_csr(const int32_t* key, int64_t V, int64_t n, int32_t* cnt, int32_t* offsets, int32_t* items, int32_t* tsum, int32_t* out_of_range,
                  int32_t* bad, bool sorted, hipStream_t st) {
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

// fflag[f] = 1 for a surviving face, whose three labels get vflag = 1 (every writer stores the same 1)
__global__ __launch_bounds__(MO_THREADS) void ms_collapse_kernel(int64_t V, int64_t F, MsWs w, int32_t* __restrict__ vflag, int32_t* counts) {
    if (w.status[0]) return;
    unsigned long long ndeg = 0, ndup = 0;
    for (int64_t f = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; f < F; f += (int64_t)gridDim.x * MO_THREADS) {
        int32_t r[3];
        if (!meshops_collapsed_face(w.gl + 3 * f, r)) {
            ++ndeg;
            continue;
        }
        int32_t best = r[0], len = w.off[r[0] + 1] - w.off[r[0]];
        for (int k = 1; k < 3; ++k) {
            const int32_t n = w.off[r[k] + 1] - w.off[r[k]];
            if (n < len) {
                len = n;
                best = r[k];
            }
        }
        if (meshops_face_is_duplicate(w.gl, w.items, w.off[best], w.off[best + 1], (int32_t)f, r, F)) {
            ++ndup;
            continue;
        }
        w.fflag[f] = 1;
        vflag[r[0]] = 1;
        vflag[r[1]] = 1;
        vflag[r[2]] = 1;
    }
    ms_wave_count(counts + 2, ndeg);
    ms_wave_count(counts + 3, ndup);
}

__global__ __launch_bounds__(MO_THREADS) void ms_collapse_out_kernel(int64_t V, int64_t F, MsWs w, const int32_t* __restrict__ vscan, int32_t* __restrict__ vmap,
                                                                     int32_t* __restrict__ fpos, int32_t* counts) {
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[4] = w.status[0];
    if (w.status[0]) return;
    const int64_t n = V > F ? V : F;
    for (int64_t i = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; i <= n; i += (int64_t)gridDim.x * MO_THREADS) {
        if (i <= V) vmap[i] = vscan[i];
        if (i <= F) fpos[i] = w.fflag[i];
    }
}

extern "C" int swnerf_mesh_collapse(const int32_t* faces, const int32_t* vlabel, int64_t V, int64_t F, void* workspace, int32_t* vmap,
                                    int32_t* fpos, int32_t* counts, void* stream) {
    int rc = mo_check("mesh_collapse", V, F);
    if (rc) return rc;
    if (!counts) return sw_fail(SWNERF_E_ARG, "mesh_collapse: NULL counts");
    hipStream_t st = (hipStream_t)stream;
    rc = sw_check(hipMemsetAsync(counts, 0, 5 * sizeof(int32_t), st), "mesh_collapse memset");
    if (rc) return rc;
    if (V == 0) F = 0;                                             // no vertex: no face can be valid, and none is read
    if (!workspace || !vmap || !fpos || (V > 0 && !vlabel) || (F > 0 && !faces)) return sw_fail(SWNERF_E_ARG, "mesh_collapse: NULL pointer");
    const MsWs w = ms_ws(workspace, V, F);
    int32_t* vflag = w.moff;
    rc = sw_check(hipMemsetAsync(w.status, 0, 64, st), "mesh_collapse memset");
    if (!rc) rc = sw_check(hipMemsetAsync(vflag, 0, (V + 1) * sizeof(int32_t), st), "mesh_collapse memset");
    if (!rc) rc = sw_check(hipMemsetAsync(w.fflag, 0, (F + 1) * sizeof(int32_t), st), "mesh_collapse memset");
    if (rc) return rc;
    if (F > 0) {
        hipLaunchKernelGGL(ms_corner_label_kernel, dim3(mo_blocks(3 * F)), dim3(MO_THREADS), 0, st, faces, vlabel, V, 3 * F, w.gl, w.status);
        // a -1 in gl is in status[0] already; the duplicate test reads whole slices in any order, so they are not sorted
        rc = ms_csr(w.gl, V, 3 * F, w.cnt, w.off, w.items, w.tsum, w.status + 4, w.status, false, st);
        if (rc) return rc;
        hipLaunchKernelGGL(ms_collapse_kernel, dim3(mo_blocks(F)), dim3(MO_THREADS), 0, st, V, F, w, vflag, counts);
    }
    rc = mo_scan(vflag, vflag, V + 1, w.tsum, counts, st);
    if (!rc) rc = mo_scan(w.fflag, w.fflag, F + 1, w.tsum, counts + 1, st);
    if (rc) return rc;
    hipLaunchKernelGGL(ms_collapse_out_kernel, dim3(mo_blocks((V > F ? V : F) + 1)), dim3(MO_THREADS), 0, st, V, F, w, (const int32_t*)vflag, vmap, fpos, counts);
    return sw_check(hipGetLastError(), "mesh_collapse launch");
}

struct MsEmit {
    const float *verts, *normals, *colors, *origin;
    const int32_t *faces, *vmap, *fpos;
    float *verts_out, *normals_out, *colors_out;
    int32_t* faces_out;
    int64_t V, F, V_out, F_out;
    int placement;
    float cell;
    double eps;
};

// surviving faces through vmap; with WELD also the rows of the labels in use
__global__ __launch_bounds__(MO_THREADS) void ms_emit_kernel(MsEmit e, MsWs w) {
    if (w.status[0]) return;
    const int64_t n = e.V > e.F ? e.V : e.F;
    for (int64_t i = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * MO_THREADS) {
        if (i < e.F && e.fpos[i + 1] != e.fpos[i] && meshops_index_ok(e.fpos[i], e.F_out)) {
            const int64_t o = e.fpos[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) e.faces_out[3 * o + k] = e.vmap[w.gl[3 * i + k]];     // a label in 0..V-1: the status word is clear
        }
        if (e.placement == MESHOPS_PLACE_WELD && i < e.V && e.vmap[i + 1] != e.vmap[i] && meshops_index_ok(e.vmap[i], e.V_out)) {
            const int64_t o = e.vmap[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                e.verts_out[3 * o + k] = e.verts[3 * i + k];
                if (e.normals) e.normals_out[3 * o + k] = e.normals[3 * i + k];
                if (e.colors) e.colors_out[3 * o + k] = e.colors[3 * i + k];
            }
        }
    }
}

// MEAN / QUADRIC: one thread per label in use, over its sorted member slice (and corner slice)
__global__ __launch_bounds__(MO_THREADS) void ms_place_kernel(MsEmit e, MsWs w) {
    if (w.status[0]) return;
    const float o[3] = {e.origin[0], e.origin[1], e.origin[2]};
    const bool quadric = e.placement == MESHOPS_PLACE_QUADRIC && e.F > 0;
    for (int64_t l = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; l < e.V; l += (int64_t)gridDim.x * MO_THREADS) {
        if (e.vmap[l + 1] == e.vmap[l] || !meshops_index_ok(e.vmap[l], e.V_out) || w.moff[l + 1] == w.moff[l]) continue;
        float pos[3], col[3];
        meshops_place_vertex(e.placement, e.verts, e.colors, e.faces, w.mitems, w.moff[l], w.moff[l + 1], w.items, quadric ? w.off[l] : 0,
                             quadric ? w.off[l + 1] : 0, l, e.V, e.F, o, e.cell, e.eps, pos, col);
        const int64_t q = e.vmap[l];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            e.verts_out[3 * q + k] = pos[k];
            if (e.colors) e.colors_out[3 * q + k] = col[k];
        }
    }
}

__global__ void ms_status_kernel(MsWs w, int32_t* __restrict__ status) {
    if (threadIdx.x == 0) status[0] = w.status[0];
}

static_assert(SWNERF_MESH_WELD == MESHOPS_PLACE_WELD && SWNERF_MESH_MEAN == MESHOPS_PLACE_MEAN && SWNERF_MESH_QUADRIC == MESHOPS_PLACE_QUADRIC,
              "swnerf.h and meshops_math.h name the placements alike");

extern "C" int swnerf_mesh_collapse_emit(const float* verts, const int32_t* faces, const float* normals, const float* colors,
                                         const int32_t* vlabel, const int32_t* vmap, const int32_t* fpos, const float* origin, float cell,
                                         int64_t V, int64_t F, int placement, double eps, void* workspace, int64_t V_out, int64_t F_out,
                                         float* verts_out, int32_t* faces_out, float* normals_out, float* colors_out, int32_t* status,
                                         void* stream) {
    int rc = mo_check("mesh_collapse_emit", V, F);
    if (rc) return rc;
    if (placement != MESHOPS_PLACE_WELD && placement != MESHOPS_PLACE_MEAN && placement != MESHOPS_PLACE_QUADRIC)
        return sw_fail(SWNERF_E_ARG, "mesh_collapse_emit: placement %d is none of SWNERF_MESH_WELD, _MEAN, _QUADRIC", placement);
    if (!(cell > 0.f) || !(cell - cell == 0.f) || !(eps >= 0.0) || !(eps - eps == 0.0))
        return sw_fail(SWNERF_E_ARG, "mesh_collapse_emit: cell = %g must be finite and positive, eps = %g finite and >= 0", (double)cell, eps);
    if (V_out < 0 || V_out > V || F_out < 0 || F_out > F)
        return sw_fail(SWNERF_E_ARG, "mesh_collapse_emit: V_out = %lld, F_out = %lld do not fit V = %lld, F = %lld", (long long)V_out, (long long)F_out,
                       (long long)V, (long long)F);
    if (!status) return sw_fail(SWNERF_E_ARG, "mesh_collapse_emit: NULL status");
    hipStream_t st = (hipStream_t)stream;
    rc = sw_check(hipMemsetAsync(status, 0, sizeof(int32_t), st), "mesh_collapse_emit memset");
    if (rc || V == 0 || V_out == 0) return rc;
    if (!workspace || !verts || !vlabel || !vmap || !fpos || !origin || !verts_out || (F > 0 && !faces) || (F_out > 0 && !faces_out) ||
        (colors && !colors_out) || (placement == MESHOPS_PLACE_WELD && normals && !normals_out))
        return sw_fail(SWNERF_E_ARG, "mesh_collapse_emit: NULL pointer");
    const MsWs w = ms_ws(workspace, V, F);
    rc = sw_check(hipMemsetAsync(w.status, 0, 64, st), "mesh_collapse_emit memset");
    if (rc) return rc;
    if (F > 0) hipLaunchKernelGGL(ms_corner_label_kernel, dim3(mo_blocks(3 * F)), dim3(MO_THREADS), 0, st, faces, vlabel, V, 3 * F, w.gl, w.status);
    MsEmit e{verts, normals, colors, origin, faces, vmap, fpos, verts_out, normals_out, colors_out, faces_out, V, F, V_out, F_out, placement, cell, eps};
    if (placement != MESHOPS_PLACE_WELD) {
        rc = ms_csr(vlabel, V, V, w.cnt, w.moff, w.mitems, w.tsum, w.status, w.status, true, st);
        if (!rc && placement == MESHOPS_PLACE_QUADRIC && F > 0) rc = ms_csr(w.gl, V, 3 * F, w.cnt, w.off, w.items, w.tsum, w.status + 4, w.status, true, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(ms_emit_kernel, dim3(mo_blocks(V > F ? V : F)), dim3(MO_THREADS), 0, st, e, w);
    if (placement != MESHOPS_PLACE_WELD) hipLaunchKernelGGL(ms_place_kernel, dim3(mo_blocks(V)), dim3(MO_THREADS), 0, st, e, w);
    hipLaunchKernelGGL(ms_status_kernel, dim3(1), dim3(64), 0, st, w, status);
    return sw_check(hipGetLastError(), "mesh_collapse_emit launch");
}

// ---- hole filling: boundary half-edges, loops by pointer jumping, fan caps ---------------------------------------------------------
//   boundary  the corner list per vertex (count, the first reader of `faces` | scan | fill; left unsorted: an edge's occurrences are
//             counted, whatever their order) | classify every corner (meshops_boundary_halfedge) | scan: the boundary half-edges
//             in ascending order | per-vertex leaving / entering counts and the smallest leaving one | next
//   loops     pointer jumping between two buffers, one launch per round, ceil(log2 nb) rounds: (jump target, smallest id seen); a
//             chain ends in "none", a cycle ends with its leader everywhere | cut every cycle in front of its leader | the same
//             rounds again with (jump target, distance to the end): rank = distance of the leader - own distance (Wyllie) | four
//             scans at the leaders' positions: loop index, vertex offset, new vertices, new faces | write
//   emit      copy the inputs | one thread per listed vertex: its new face, and at every 64th rank the run's fp64 sum | one thread
//             per loop: the run sums in order, the mean
// next is injective where defined (a simple head has one entering and one leaving half-edge), so the half-edges fall into pure
// cycles and chains; should a caller hand in other links, every write below is still guarded by its bound.
#define MF_NONE (-1)

struct MfBoundaryWs { int32_t *flag, *nout, *nin, *leave, *cnt, *off, *items, *tsum; };
struct MfLoopsWs { int2 *a, *b; int32_t *leader, *s2, *s3, *tsum; };

static inline int64_t mf_tsum_bytes(int64_t V, int64_t F) { return mo_round256(4 * mo_tiles((3 * F > V ? 3 * F : V) + 2)); }
static inline int64_t mf_boundary_bytes(int64_t V, int64_t F) { return 2 * mo_round256(4 * (3 * F + 2)) + 5 * mo_round256(4 * (V + 1)) + mf_tsum_bytes(V, F); }
static inline int64_t mf_loops_bytes(int64_t V, int64_t F) { return 2 * mo_round256(8 * (3 * F + 1)) + 3 * mo_round256(4 * (3 * F + 2)) + mf_tsum_bytes(V, F); }
static inline int64_t mf_slots(int64_t M, int64_t L) { return M / MESHOPS_FILL_RUN + L + 2; }
static inline int64_t mf_emit_bytes(int64_t F) { return mo_round256(8 * 6 * mf_slots(3 * F, F)); }

static MfBoundaryWs mf_boundary_ws(void* ws, int64_t V, int64_t F) {
    char* p = (char*)ws;
    MfBoundaryWs w;
    w.flag = (int32_t*)p;  p += mo_round256(4 * (3 * F + 2));
    w.nout = (int32_t*)p;  p += mo_round256(4 * (V + 1));
    w.nin = (int32_t*)p;   p += mo_round256(4 * (V + 1));
    w.leave = (int32_t*)p; p += mo_round256(4 * (V + 1));
    w.cnt = (int32_t*)p;   p += mo_round256(4 * (V + 1));
    w.off = (int32_t*)p;   p += mo_round256(4 * (V + 1));
    w.items = (int32_t*)p; p += mo_round256(4 * (3 * F + 2));
    w.tsum = (int32_t*)p;
    return w;
}

static MfLoopsWs mf_loops_ws(void* ws, int64_t F) {
    char* p = (char*)ws;
    MfLoopsWs w;
    w.a = (int2*)p;         p += mo_round256(8 * (3 * F + 1));
    w.b = (int2*)p;         p += mo_round256(8 * (3 * F + 1));
    w.leader = (int32_t*)p; p += mo_round256(4 * (3 * F + 2));
    w.s2 = (int32_t*)p;     p += mo_round256(4 * (3 * F + 2));
    w.s3 = (int32_t*)p;     p += mo_round256(4 * (3 * F + 2));
    w.tsum = (int32_t*)p;
    return w;
}

extern "C" int64_t swnerf_mesh_fill_workspace_bytes(int64_t V, int64_t F) {
    if (!mo_sizes_ok(V, F)) return 0;
    const int64_t a = mf_boundary_bytes(V, F), b = mf_loops_bytes(V, F), c = mf_emit_bytes(F);
    return (a > b ? (a > c ? a : c) : (b > c ? b : c)) + 512;
}

// flag[c] = 1 for a boundary half-edge (the corner lists were built from these faces: every index is in range when *bad is clear)
__global__ __launch_bounds__(MO_THREADS) void mf_classify_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ offsets,
                                                                 const int32_t* __restrict__ items, int64_t V, int64_t F, int32_t* __restrict__ flag, const int32_t* bad) {
    if (*bad) return;
    for (int64_t c = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; c < 3 * F; c += (int64_t)gridDim.x * MO_THREADS)
        flag[c] = meshops_boundary_halfedge(faces, offsets, items, (int32_t)c, V, F);
}

// pos = the exclusive scan of the flags: half-edge c is the pos[c]-th boundary half-edge iff pos[c + 1] != pos[c]
__global__ __launch_bounds__(MO_THREADS) void mf_compact_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ pos, int64_t V, int64_t F,
                                                                int32_t* __restrict__ bhe, MfBoundaryWs w, const int32_t* bad) {
    if (*bad) return;
    for (int64_t c = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; c < 3 * F; c += (int64_t)gridDim.x * MO_THREADS) {
        const int32_t i = pos[c];
        if (pos[c + 1] == i || !meshops_index_ok(i, 3 * F)) continue;
        const int64_t f = c / 3;
        const int32_t a = faces[c], b = faces[3 * f + (c - 3 * f + 1) % 3];      // both in range: the half-edge was flagged
        bhe[i] = (int32_t)c;
        atomicAdd(w.nout + a, 1);
        atomicAdd(w.nin + b, 1);
        atomicMin(w.leave + a, i);
    }
}

__global__ __launch_bounds__(MO_THREADS) void mf_next_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ bhe, int64_t F, MfBoundaryWs w,
                                                             int32_t* __restrict__ bnext, int32_t* counts) {
    if (counts[1]) {
        if (blockIdx.x == 0 && threadIdx.x == 0) counts[0] = 0;
        return;
    }
    const int64_t nb = w.flag[3 * F];
    for (int64_t i = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; i < nb && i < 3 * F; i += (int64_t)gridDim.x * MO_THREADS) {
        const int64_t c = bhe[i], f = c / 3;
        const int32_t h = faces[3 * f + (c - 3 * f + 1) % 3];
        bnext[i] = (w.nout[h] == 1 && w.nin[h] == 1) ? w.leave[h] : MF_NONE;
    }
}

extern "C" int swnerf_mesh_boundary(const int32_t* faces, int64_t V, int64_t F, void* workspace, int32_t* bhe, int32_t* bnext, int32_t* counts,
                                    void* stream) {
    int rc = mo_check("mesh_boundary", V, F);
    if (rc) return rc;
    if (!counts) return sw_fail(SWNERF_E_ARG, "mesh_boundary: NULL counts");
    hipStream_t st = (hipStream_t)stream;
    rc = sw_check(hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), st), "mesh_boundary memset");
    if (rc || V == 0 || F == 0) return rc;
    if (!faces || !workspace || !bhe || !bnext) return sw_fail(SWNERF_E_ARG, "mesh_boundary: NULL pointer");
    const MfBoundaryWs w = mf_boundary_ws(workspace, V, F);
    rc = sw_check(hipMemsetAsync(w.flag, 0, 4 * (3 * F + 2), st), "mesh_boundary memset");
    if (!rc) rc = sw_check(hipMemsetAsync(w.nout, 0, 2 * mo_round256(4 * (V + 1)), st), "mesh_boundary memset");       // nout and nin
    if (!rc) rc = sw_check(hipMemsetAsync(w.leave, 0x7F, 4 * (V + 1), st), "mesh_boundary memset");
    if (!rc) rc = ms_csr(faces, V, 3 * F, w.cnt, w.off, w.items, w.tsum, counts + 1, counts + 1, false, st);
    if (rc) return rc;
    hipLaunchKernelGGL(mf_classify_kernel, dim3(mo_blocks(3 * F)), dim3(MO_THREADS), 0, st, faces, (const int32_t*)w.off, (const int32_t*)w.items, V, F, w.flag,
                       (const int32_t*)(counts + 1));
    rc = mo_scan(w.flag, w.flag, 3 * F + 1, w.tsum, counts, st);
    if (rc) return rc;
    hipLaunchKernelGGL(mf_compact_kernel, dim3(mo_blocks(3 * F)), dim3(MO_THREADS), 0, st, faces, (const int32_t*)w.flag, V, F, bhe, w, (const int32_t*)(counts + 1));
    hipLaunchKernelGGL(mf_next_kernel, dim3(mo_blocks(3 * F)), dim3(MO_THREADS), 0, st, faces, (const int32_t*)bhe, F, w, bnext, counts);
    return sw_check(hipGetLastError(), "mesh_boundary launch");
}

// (jump target, smallest id seen): the element itself
__global__ __launch_bounds__(MO_THREADS) void mf_jump_init_kernel(const int32_t* __restrict__ bnext, int64_t nb, int2* __restrict__ x) {
    for (int64_t i = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; i < nb; i += (int64_t)gridDim.x * MO_THREADS) {
        const int32_t j = bnext[i];
        x[i] = make_int2(meshops_index_ok(j, nb) ? j : MF_NONE, (int32_t)i);
    }
}

// One round of pointer jumping, x -> y: MIN keeps the smaller second word (the leader search), else the words are added (the
// distance to the end).  A target of "none" stays: the element has reached the end of its chain.
template <bool MIN>
__global__ __launch_bounds__(MO_THREADS) void mf_jump_kernel(const int2* __restrict__ x, int64_t nb, int2* __restrict__ y) {
    for (int64_t i = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; i < nb; i += (int64_t)gridDim.x * MO_THREADS) {
        int2 e = x[i];
        if (e.x >= 0) {
            const int2 t = x[e.x];                                 // in 0..nb-1: the init kernels wrote nothing else
            e.y = MIN ? (t.y < e.y ? t.y : e.y) : e.y + t.y;
            e.x = t.x;
        }
        y[i] = e;
    }
}

// x = the leader search's result.  leader[i] = the cycle's smallest element, or none on a chain; y = the cycle cut in front of its
// leader as (next, 1), (none, 0) for the last element and for a chain.
__global__ __launch_bounds__(MO_THREADS) void mf_cut_kernel(const int2* __restrict__ x, const int32_t* __restrict__ bnext, int64_t nb, int32_t* __restrict__ leader,
                                                            int2* __restrict__ y) {
    for (int64_t i = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; i < nb; i += (int64_t)gridDim.x * MO_THREADS) {
        const int2 e = x[i];
        const int32_t j = bnext[i];
        const bool cyc = e.x >= 0 && meshops_index_ok(e.y, nb) && meshops_index_ok(j, nb);
        leader[i] = cyc ? e.y : MF_NONE;
        y[i] = cyc && j != e.y ? make_int2(j, 1) : make_int2(MF_NONE, 0);
    }
}

struct MfMark { int32_t *s0, *s1, *s2, *s3; };

// at a leader: 1, the loop's length, "gets a new vertex", its new faces; 0 elsewhere and at the end (the scans' totals)
__global__ __launch_bounds__(MO_THREADS) void mf_mark_kernel(const int2* __restrict__ x, const int32_t* __restrict__ leader, int64_t nb, int32_t max_edges, MfMark m,
                                                             int32_t* counts) {
    unsigned long long nloops = 0, nedges = 0;
    for (int64_t i = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; i <= nb; i += (int64_t)gridDim.x * MO_THREADS) {
        const bool lead = i < nb && leader[i] == (int32_t)i;
        const int32_t n = lead ? x[i].y + 1 : 0;
        const bool fill = lead && n >= 3 && (max_edges <= 0 || n <= max_edges);
        m.s0[i] = lead;
        m.s1[i] = n;
        m.s2[i] = fill && n >= 4;
        m.s3[i] = fill ? (n == 3 ? 1 : n) : 0;
        nloops += fill;
        nedges += fill ? n : 0;
    }
    ms_wave_count(counts + 2, nloops);
    ms_wave_count(counts + 3, nedges);
}

struct MfLoopsOut { int32_t *table, *loop_offsets, *loop_vertices, *loop_vnew, *loop_fnew; };

// s0..s3 are scanned: at a leader they hold the loop's index, its offset in the vertex list and its new vertex / face offsets
__global__ __launch_bounds__(MO_THREADS) void mf_loops_write_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ bhe, const int2* __restrict__ x,
                                                                    const int32_t* __restrict__ leader, int64_t F, int64_t nb, MfMark m, MfLoopsOut o) {
    const int64_t cap = nb / 3;                                    // loops: each has at least 3 half-edges
    if (blockIdx.x == 0 && threadIdx.x == 0 && meshops_index_ok(m.s0[nb], cap + 1)) {
        const int64_t L = m.s0[nb];
        o.loop_offsets[L] = m.s1[nb];
        o.loop_vnew[L] = m.s2[nb];
        o.loop_fnew[L] = m.s3[nb];
    }
    for (int64_t i = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; i < nb; i += (int64_t)gridDim.x * MO_THREADS) {
        const int32_t l = leader[i];
        if (l < 0) continue;
        const int32_t dl = x[l].y, r = dl - x[i].y, off = m.s1[l], li = m.s0[l], c = bhe[i];
        if (meshops_index_ok(r, (int64_t)dl + 1) && meshops_index_ok(off, nb) && meshops_index_ok((int64_t)off + r, nb) && meshops_index_ok(c, 3 * F))
            o.loop_vertices[off + r] = faces[c];
        if (l == (int32_t)i && meshops_index_ok(li, cap)) {
            o.table[2 * (int64_t)li] = c;
            o.table[2 * (int64_t)li + 1] = dl + 1;
            o.loop_offsets[li] = off;
            o.loop_vnew[li] = m.s2[l];
            o.loop_fnew[li] = m.s3[l];
        }
    }
}

extern "C" int swnerf_mesh_boundary_loops(const int32_t* faces, const int32_t* bhe, const int32_t* bnext, int64_t V, int64_t F, int64_t nb,
                                          int64_t max_edges, void* workspace, int32_t* table, int32_t* loop_offsets, int32_t* loop_vertices,
                                          int32_t* loop_vnew, int32_t* loop_fnew, int32_t* counts, void* stream) {
    int rc = mo_check("mesh_boundary_loops", V, F);
    if (rc) return rc;
    if (nb < 0 || nb > 3 * F) return sw_fail(SWNERF_E_ARG, "mesh_boundary_loops: nb = %lld is not in 0..3 F = %lld", (long long)nb, (long long)(3 * F));
    if (max_edges != 0 && (max_edges < 3 || max_edges > INT32_MAX))
        return sw_fail(SWNERF_E_ARG, "mesh_boundary_loops: max_edges = %lld must be 0 (no limit) or in 3..2^31-1", (long long)max_edges);
    if (!counts || !loop_offsets || !loop_vnew || !loop_fnew) return sw_fail(SWNERF_E_ARG, "mesh_boundary_loops: NULL counts / loop_offsets / loop_vnew / loop_fnew");
    hipStream_t st = (hipStream_t)stream;
    rc = sw_check(hipMemsetAsync(counts, 0, 8 * sizeof(int32_t), st), "mesh_boundary_loops memset");
    if (!rc) rc = sw_check(hipMemsetAsync(loop_offsets, 0, sizeof(int32_t), st), "mesh_boundary_loops memset");
    if (!rc) rc = sw_check(hipMemsetAsync(loop_vnew, 0, sizeof(int32_t), st), "mesh_boundary_loops memset");
    if (!rc) rc = sw_check(hipMemsetAsync(loop_fnew, 0, sizeof(int32_t), st), "mesh_boundary_loops memset");
    if (rc || nb == 0) return rc;
    if (!faces || !bhe || !bnext || !workspace || !table || !loop_vertices) return sw_fail(SWNERF_E_ARG, "mesh_boundary_loops: NULL pointer");
    const MfLoopsWs w = mf_loops_ws(workspace, F);
    int rounds = 0;
    while (((int64_t)1 << rounds) < nb) ++rounds;
    const dim3 grid(mo_blocks(nb)), block(MO_THREADS);
    int2 *x = w.a, *y = w.b;
    hipLaunchKernelGGL(mf_jump_init_kernel, grid, block, 0, st, bnext, nb, x);
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(mf_jump_kernel<true>, grid, block, 0, st, (const int2*)x, nb, y);
        int2* t = x; x = y; y = t;
    }
    hipLaunchKernelGGL(mf_cut_kernel, grid, block, 0, st, (const int2*)x, bnext, nb, w.leader, y);
    { int2* t = x; x = y; y = t; }
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(mf_jump_kernel<false>, grid, block, 0, st, (const int2*)x, nb, y);
        int2* t = x; x = y; y = t;
    }
    // x holds (none, distance to the end); the other buffer is free for two of the four scan arrays
    MfMark m{(int32_t*)y, (int32_t*)y + (nb + 1), w.s2, w.s3};
    hipLaunchKernelGGL(mf_mark_kernel, dim3(mo_blocks(nb + 1)), block, 0, st, (const int2*)x, (const int32_t*)w.leader, nb, (int32_t)max_edges, m, counts);
    rc = mo_scan(m.s0, m.s0, nb + 1, w.tsum, counts, st);
    if (!rc) rc = mo_scan(m.s1, m.s1, nb + 1, w.tsum, counts + 1, st);
    if (!rc) rc = mo_scan(m.s2, m.s2, nb + 1, w.tsum, counts + 4, st);
    if (!rc) rc = mo_scan(m.s3, m.s3, nb + 1, w.tsum, counts + 5, st);
    if (rc) return rc;
    MfLoopsOut o{table, loop_offsets, loop_vertices, loop_vnew, loop_fnew};
    hipLaunchKernelGGL(mf_loops_write_kernel, grid, block, 0, st, faces, bhe, (const int2*)x, (const int32_t*)w.leader, F, nb, m, o);
    return sw_check(hipGetLastError(), "mesh_boundary_loops launch");
}

struct MfEmit {
    const float *verts, *colors;
    const int32_t *loop_offsets, *loop_vertices, *loop_vnew, *loop_fnew;
    float *verts_out, *colors_out;
    int32_t* faces_out;
    double *part, *cpart;
    int64_t V, F, L, M, V_out, F_out, slots;
};

// the loop li whose slice of the vertex list holds position p (offsets ascending, offsets[L] = M > p)
__device__ __forceinline__ int64_t mf_loop_of(const int32_t* __restrict__ offsets, int64_t L, int64_t p) {
    int64_t lo = 0, hi = L;                                        // the answer is in [lo, hi)
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)offsets[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

struct MfLoop { int32_t off, n, vnew, fnew; bool fill, fan; };

// loop li as the lists give it; n = 0 when its slice is not a loop of the list (then nothing is done for it)
__device__ __forceinline__ MfLoop mf_loop(const MfEmit& e, int64_t li) {
    MfLoop l;
    l.off = e.loop_offsets[li];
    const int64_t n = (int64_t)e.loop_offsets[li + 1] - l.off;
    l.n = l.off >= 0 && n >= 3 && l.off + n <= e.M ? (int32_t)n : 0;
    l.vnew = e.loop_vnew[li];
    l.fnew = e.loop_fnew[li];
    l.fill = l.n > 0 && e.loop_fnew[li + 1] != l.fnew;
    l.fan = l.fill && e.loop_vnew[li + 1] != l.vnew;
    return l;
}

__global__ __launch_bounds__(MO_THREADS) void mf_emit_faces_kernel(MfEmit e, int32_t* bad) {
    unsigned long long nbad = 0;
    for (int64_t p = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; p < e.M; p += (int64_t)gridDim.x * MO_THREADS) {
        nbad += !meshops_index_ok(e.loop_vertices[p], e.V);
        const int64_t li = mf_loop_of(e.loop_offsets, e.L, p);
        const MfLoop l = mf_loop(e, li);
        const int64_t r = p - l.off;
        if (!l.fill || !meshops_index_ok((int32_t)r, l.n)) continue;
        if (l.fan || r == 0) {
            const int64_t o = e.F + l.fnew + r;
            int32_t t[3];
            meshops_fill_face(e.loop_vertices + l.off, l.n, (int32_t)r, (int32_t)(e.V + l.vnew), t);
            if (meshops_index_ok(l.fnew, e.F_out) && o < e.F_out) {
                e.faces_out[3 * o] = t[0]; e.faces_out[3 * o + 1] = t[1]; e.faces_out[3 * o + 2] = t[2];
            }
        }
        if (l.fan && r % MESHOPS_FILL_RUN == 0) {
            const int64_t slot = meshops_fill_slot(l.off, li, r / MESHOPS_FILL_RUN);
            if (slot >= e.slots) continue;
            const int32_t hi = (int32_t)(r + MESHOPS_FILL_RUN < l.n ? p + MESHOPS_FILL_RUN : (int64_t)l.off + l.n);
            meshops_run_sum(e.verts, e.loop_vertices, (int32_t)p, hi, e.V, e.part + 3 * slot);
            if (e.colors) meshops_run_sum(e.colors, e.loop_vertices, (int32_t)p, hi, e.V, e.cpart + 3 * slot);
        }
    }
    ms_wave_count(bad, nbad);
}

__global__ __launch_bounds__(MO_THREADS) void mf_emit_verts_kernel(MfEmit e) {
    for (int64_t li = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; li < e.L; li += (int64_t)gridDim.x * MO_THREADS) {
        const MfLoop l = mf_loop(e, li);
        const int64_t o = e.V + l.vnew, slot = meshops_fill_slot(l.off, li, 0);
        const int32_t nruns = (l.n + MESHOPS_FILL_RUN - 1) / MESHOPS_FILL_RUN;
        if (!l.fan || l.vnew < 0 || o >= e.V_out || slot + nruns > e.slots) continue;
        meshops_blocked_mean(e.part + 3 * slot, nruns, l.n, e.verts_out + 3 * o);
        if (e.colors) meshops_blocked_mean(e.cpart + 3 * slot, nruns, l.n, e.colors_out + 3 * o);
    }
}

extern "C" int swnerf_mesh_fill_emit(const float* verts, const int32_t* faces, const float* colors, int64_t V, int64_t F, const int32_t* loop_offsets,
                                     const int32_t* loop_vertices, const int32_t* loop_vnew, const int32_t* loop_fnew, int64_t L, int64_t M,
                                     void* workspace, int64_t V_out, int64_t F_out, float* verts_out, int32_t* faces_out, float* colors_out,
                                     int32_t* status, void* stream) {
    int rc = mo_check("mesh_fill_emit", V, F);
    if (!rc) rc = mo_check("mesh_fill_emit (output)", V_out, F_out);
    if (rc) return rc;
    if (M < 0 || M > 3 * F || L < 0 || 3 * L > M || V_out < V || V_out > V + L || F_out < F || F_out > F + M)
        return sw_fail(SWNERF_E_ARG, "mesh_fill_emit: L = %lld loops of M = %lld vertices, V_out = %lld, F_out = %lld do not fit V = %lld, F = %lld", (long long)L,
                       (long long)M, (long long)V_out, (long long)F_out, (long long)V, (long long)F);
    if (!status) return sw_fail(SWNERF_E_ARG, "mesh_fill_emit: NULL status");
    if ((V_out > 0 && !verts_out) || (F_out > 0 && !faces_out) || (V > 0 && !verts) || (F > 0 && !faces) || (colors && !colors_out))
        return sw_fail(SWNERF_E_ARG, "mesh_fill_emit: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    rc = sw_check(hipMemsetAsync(status, 0, sizeof(int32_t), st), "mesh_fill_emit memset");
    if (!rc && V > 0) rc = sw_check(hipMemcpyAsync(verts_out, verts, 12 * V, hipMemcpyDeviceToDevice, st), "mesh_fill_emit copy");
    if (!rc && F > 0) rc = sw_check(hipMemcpyAsync(faces_out, faces, 12 * F, hipMemcpyDeviceToDevice, st), "mesh_fill_emit copy");
    if (!rc && V > 0 && colors) rc = sw_check(hipMemcpyAsync(colors_out, colors, 12 * V, hipMemcpyDeviceToDevice, st), "mesh_fill_emit copy");
    if (rc || L == 0) return rc;
    if (!workspace || !loop_offsets || !loop_vertices || !loop_vnew || !loop_fnew) return sw_fail(SWNERF_E_ARG, "mesh_fill_emit: NULL pointer");
    const int64_t slots = mf_slots(M, L);                          // <= mf_slots(3 F, F): the workspace holds them
    MfEmit e{verts, colors, loop_offsets, loop_vertices, loop_vnew, loop_fnew, verts_out, colors_out, faces_out, (double*)workspace, (double*)workspace + 3 * slots,
             V, F, L, M, V_out, F_out, slots};
    hipLaunchKernelGGL(mf_emit_faces_kernel, dim3(mo_blocks(M)), dim3(MO_THREADS), 0, st, e, status);
    hipLaunchKernelGGL(mf_emit_verts_kernel, dim3(mo_blocks(L)), dim3(MO_THREADS), 0, st, e);
    return sw_check(hipGetLastError(), "mesh_fill_emit launch");
}
