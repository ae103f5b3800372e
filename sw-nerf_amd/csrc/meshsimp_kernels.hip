// meshsimp_kernels.hip - welding and decimation of a triangle mesh that is already on the device, by vertex clustering on a uniform
// grid.  The arithmetic is in meshops_math.h, the workspace layout in meshops_layout.h; the scan and the CSR construction are those
// of meshops_kernels.hip (mo_scan, mo_csr of meshops_common.h).
//   cluster   origin (integer atomics on ordered keys, unless given) | insert: an open-addressing table of the 64-bit cell keys,
//             a slot claimed by atomicCAS takes the atomicMin of its vertices | label = the slot's minimum; roots are counted
//   collapse  labels of the corners (the first reader of `faces`) | the corner list per label (count | scan | fill; left unsorted) |
//             per face: degenerate, duplicate (a scan of the whole slice of its label with the fewest corners) or kept, kept faces
//             mark their labels | two scans | a guarded copy to the outputs
//   emit      labels of the corners | faces through vmap | WELD: copy rows; MEAN / QUADRIC: member list per label, QUADRIC also the
//             corner list, then one thread per output vertex over its sorted slices (meshops_place_vertex)
// The table decides only which slot a key sits in: every result is a minimum or a count, so nothing depends on the arrival order.
#include "meshops_common.h"

extern "C" int64_t swnerf_mesh_simplify_workspace_bytes(int64_t V, int64_t F) {
    int64_t bytes = 0;
    if (mo_sizes_ok(V, F)) ms_ws(nullptr, V, F, &bytes);
    return bytes;
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
    wave_count(w.status + 1, ninvalid);
    wave_count(w.status + 2, nfull);
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
    wave_count(counts, nroot);
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
    rc = sw_check(hipMemsetAsync(w.tkey, 0xFF, (char*)w.slot - (char*)w.tkey, st), "mesh_cluster memset");      // tkey | tmin.  keys: empty; minima: 2^32 - 1
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
    wave_count(bad, nbad);
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
    wave_count(counts + 2, ndeg);
    wave_count(counts + 3, ndup);
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
        rc = mo_csr(w.gl, V, 3 * F, w.cnt, w.off, w.items, w.tsum, w.status + 4, w.status, false, st);
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
        if (i < e.F && mo_kept(e.fpos, i, e.F_out)) {
            const int64_t o = e.fpos[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) e.faces_out[3 * o + k] = e.vmap[w.gl[3 * i + k]];     // a label in 0..V-1: the status word is clear
        }
        if (e.placement == MESHOPS_PLACE_WELD && i < e.V && mo_kept(e.vmap, i, e.V_out))
            mo_copy_row(e.verts, e.normals, e.colors, i, e.verts_out, e.normals_out, e.colors_out, e.vmap[i]);
    }
}

// MEAN / QUADRIC: one thread per label in use, over its sorted member slice (and corner slice)
__global__ __launch_bounds__(MO_THREADS) void ms_place_kernel(MsEmit e, MsWs w) {
    if (w.status[0]) return;
    const float o[3] = {e.origin[0], e.origin[1], e.origin[2]};
    const bool quadric = e.placement == MESHOPS_PLACE_QUADRIC && e.F > 0;
    for (int64_t l = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; l < e.V; l += (int64_t)gridDim.x * MO_THREADS) {
        if (!mo_kept(e.vmap, l, e.V_out) || w.moff[l + 1] == w.moff[l]) continue;
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
        rc = mo_csr(vlabel, V, V, w.cnt, w.moff, w.mitems, w.tsum, w.status, w.status, true, st);
        if (!rc && placement == MESHOPS_PLACE_QUADRIC && F > 0) rc = mo_csr(w.gl, V, 3 * F, w.cnt, w.off, w.items, w.tsum, w.status + 4, w.status, true, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(ms_emit_kernel, dim3(mo_blocks(V > F ? V : F)), dim3(MO_THREADS), 0, st, e, w);
    if (placement != MESHOPS_PLACE_WELD) hipLaunchKernelGGL(ms_place_kernel, dim3(mo_blocks(V)), dim3(MO_THREADS), 0, st, e, w);
    hipLaunchKernelGGL(ms_status_kernel, dim3(1), dim3(64), 0, st, w, status);
    return sw_check(hipGetLastError(), "mesh_collapse_emit launch");
}
