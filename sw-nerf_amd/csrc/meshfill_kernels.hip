// meshfill_kernels.hip - hole filling of a triangle mesh that is already on the device: boundary half-edges, loops by pointer jumping,
// fan caps.  The arithmetic is in meshops_math.h, the workspace layouts of the three phases in meshops_layout.h; the scan and the CSR
// construction are those of meshops_kernels.hip (mo_scan, mo_csr of meshops_common.h).
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
#include "meshops_common.h"

#define MF_NONE (-1)

// the largest of the three phases' layouts, which follow one another in the same workspace, and 512 bytes
extern "C" int64_t swnerf_mesh_fill_workspace_bytes(int64_t V, int64_t F) {
    if (!mo_sizes_ok(V, F)) return 0;
    int64_t a, b;
    mf_boundary_ws(nullptr, V, F, &a);
    mf_loops_ws(nullptr, V, F, &b);
    const int64_t c = mf_emit_bytes(F);
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
        if (!mo_kept(pos, c, 3 * F)) continue;
        const int32_t i = pos[c];
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
    if (!rc) rc = sw_check(hipMemsetAsync(w.nout, 0, (char*)w.leave - (char*)w.nout, st), "mesh_boundary memset");     // nout | nin
    if (!rc) rc = sw_check(hipMemsetAsync(w.leave, 0x7F, 4 * (V + 1), st), "mesh_boundary memset");
    if (!rc) rc = mo_csr(faces, V, 3 * F, w.cnt, w.off, w.items, w.tsum, counts + 1, counts + 1, false, st);
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
    wave_count(counts + 2, nloops);
    wave_count(counts + 3, nedges);
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
    const MfLoopsWs w = mf_loops_ws(workspace, V, F);
    int rounds = 0;
    while (((int64_t)1 << rounds) < nb) ++rounds;
    const dim3 grid(mo_blocks(nb)), block(MO_THREADS);
    int2 *x = (int2*)w.a, *y = (int2*)w.b;
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
    wave_count(bad, nbad);
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
