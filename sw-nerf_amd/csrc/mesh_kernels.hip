// mesh_kernels.hip - marching cubes on a device-resident scalar field: the second half of nerf/extract_mesh.py
// (generate_mesh, :92-131, which calls skimage.measure.marching_cubes).  Three deterministic passes, no atomics:
//   classify  one work item per 4 consecutive points of a grid row: the crossing mask of each point's 3 owned edges
//             (+x, +y, +z) and the case of the cell whose min corner it is, stored as a uint16 code; per 256-item tile the
//             (vertex, triangle) totals
//   scan      one workgroup turns the tile totals into exclusive int64 tile offsets and the grand totals; the in-tile part
//             of the scan is redone from the codes by the emit kernels (reduce, scan the reductions, rescan the tiles)
//   emit      vertices in (owner point, axis x < y < z) order, then triangles in (cell, table) order; a cell finds the vertex
//             of its edge (owner q, axis a) at voff[q] + popcount(mask(q) & ((1 << a) - 1))
// Field layout: nx * ny * nz points in C order (i slowest), consecutive points `ld` floats apart.
#include <hip/hip_runtime.h>
#include "../../include/swnerf.h"
#include "host_util.h"
#include "par_prims.h"                 // block_exclusive_scan
#define SW_MC_TABLE_QUAL static __constant__ const
#include "mc_tables.h"

#define MC_BLOCK 256                   // work items per tile (= threads per workgroup of the tile kernels)
#define MC_PTS 4                       // points per work item (along z)
#define MC_SCAN_THREADS 1024
#define MC_MAX_GRID 2048               // grid-stride cap (Guideline 11)

struct McGrid {
    const float* f; int64_t ld;
    int64_t nx, ny, nz, syz;           // syz = ny * nz (points per x plane)
    int64_t kg, ngroups, ntiles;       // work items per row = ceil(nz / 4); items; tiles of MC_BLOCK items
    float level;
    int vec;                           // ld == 1, nz % 4 == 0 and 16-byte aligned field: float4 row loads
};

static inline int64_t mc_round256(int64_t b) { return (b + 255) & ~(int64_t)255; }

static McGrid mc_grid(int64_t nx, int64_t ny, int64_t nz) {
    McGrid g{};
    g.nx = nx; g.ny = ny; g.nz = nz; g.syz = ny * nz;
    g.kg = (nz + MC_PTS - 1) / MC_PTS;
    g.ngroups = nx * ny * g.kg;
    g.ntiles = (g.ngroups + MC_BLOCK - 1) / MC_BLOCK;
    return g;
}

// workspace: code uint16 [N] | voff int32 [N] | tile vertex sums int64 [T] | tile triangle sums int64 [T] (scanned in place)
struct McWs { uint16_t* code; int32_t* voff; int64_t* tv; int64_t* tt; };

static McWs mc_ws(void* ws, const McGrid& g) {
    const int64_t N = g.nx * g.syz;
    char* p = (char*)ws;
    McWs w;
    w.code = (uint16_t*)p;                 p += mc_round256(2 * N);
    w.voff = (int32_t*)p;                  p += mc_round256(4 * N);
    w.tv = (int64_t*)p;                    p += mc_round256(8 * g.ntiles);
    w.tt = (int64_t*)p;
    return w;
}

// 5 values of one grid row from k0 on (k0 + t < nz; the others are never read): float4 + 1 when vectorised
__device__ __forceinline__ void mc_load_row(const McGrid& g, int64_t row, int64_t k0, float v[MC_PTS + 1]) {
    const int64_t p = row * g.nz + k0;
    if (g.vec) {
        const float4 q = *reinterpret_cast<const float4*>(g.f + p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        v[4] = (k0 + 4 < g.nz) ? g.f[p + 4] : 0.f;
    } else {
#pragma unroll
        for (int t = 0; t <= MC_PTS; ++t) v[t] = (k0 + t < g.nz) ? g.f[(p + t) * g.ld] : 0.f;
    }
}

__device__ __forceinline__ void mc_item(const McGrid& g, int64_t item, int64_t* row, int64_t* i, int64_t* j, int64_t* k0, int* np) {
    *row = item / g.kg;
    *k0 = (item - *row * g.kg) * MC_PTS;
    *i = *row / g.ny;
    *j = *row - *i * g.ny;
    const int64_t left = g.nz - *k0;
    *np = left < MC_PTS ? (int)left : MC_PTS;
}

__global__ void __launch_bounds__(MC_BLOCK) mc_classify_kernel(McGrid g, McWs w) {
    __shared__ int64_t lds[MC_BLOCK / 64];
    for (int64_t tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
        const int64_t item = tile * MC_BLOCK + threadIdx.x;
        int nv = 0, nt = 0;
        if (item < g.ngroups) {
            int64_t row, i, j, k0;
            int np;
            mc_item(g, item, &row, &i, &j, &k0, &np);
            const bool hx = i + 1 < g.nx, hy = j + 1 < g.ny;
            float v[2][2][MC_PTS + 1] = {};                       // [di][dj][t]; rows past the grid stay 0 (never read)
            mc_load_row(g, row, k0, v[0][0]);
            if (hy) mc_load_row(g, row + 1, k0, v[0][1]);
            if (hx) mc_load_row(g, row + g.ny, k0, v[1][0]);
            if (hx && hy) mc_load_row(g, row + g.ny + 1, k0, v[1][1]);
            unsigned in[2][2] = {{0u, 0u}, {0u, 0u}};            // bit t: value at k0 + t is inside
#pragma unroll
            for (int di = 0; di < 2; ++di)
#pragma unroll
                for (int dj = 0; dj < 2; ++dj)
#pragma unroll
                    for (int t = 0; t <= MC_PTS; ++t)
                        in[di][dj] |= (v[di][dj][t] > g.level ? 1u : 0u) << t;
            uint16_t code[MC_PTS];
#pragma unroll
            for (int t = 0; t < MC_PTS; ++t) {
                const bool hz = k0 + t + 1 < g.nz;
                const unsigned b00 = in[0][0] >> t & 1u;
                unsigned m = 0, c = 0;
                if (hx && (b00 != (in[1][0] >> t & 1u))) m |= 1u;
                if (hy && (b00 != (in[0][1] >> t & 1u))) m |= 2u;
                if (hz && (b00 != (in[0][0] >> (t + 1) & 1u))) m |= 4u;
                if (hx && hy && hz) {
#pragma unroll
                    for (int cn = 0; cn < 8; ++cn)
                        c |= (in[cn & 1][cn >> 1 & 1] >> (t + (cn >> 2)) & 1u) << cn;
                }
                code[t] = (uint16_t)(c | m << 8);
                if (t < np) {
                    nv += __builtin_popcount(m);
                    nt += sw_mc_ntri[c];
                }
            }
            const int64_t p = row * g.nz + k0;
            if (np == MC_PTS && (p & 3) == 0) {
                ushort4 q; q.x = code[0]; q.y = code[1]; q.z = code[2]; q.w = code[3];
                *reinterpret_cast<ushort4*>(w.code + p) = q;
            } else {
                for (int t = 0; t < np; ++t) w.code[p + t] = code[t];
            }
        }
        int64_t sv, st;
        block_exclusive_scan<int64_t, MC_BLOCK>((int64_t)nv, lds, &sv);
        block_exclusive_scan<int64_t, MC_BLOCK>((int64_t)nt, lds, &st);
        if (threadIdx.x == 0) { w.tv[tile] = sv; w.tt[tile] = st; }
    }
}

// one workgroup: tile sums -> exclusive tile offsets (in place), grand totals -> totals[2]
__global__ void __launch_bounds__(MC_SCAN_THREADS) mc_scan_kernel(int64_t ntiles, int64_t* tv, int64_t* tt, int64_t* totals) {
    __shared__ int64_t lds[MC_SCAN_THREADS / 64];
    const int64_t per = (ntiles + MC_SCAN_THREADS - 1) / MC_SCAN_THREADS;
    const int64_t lo = threadIdx.x * per, hi = lo + per < ntiles ? lo + per : ntiles;
    int64_t sv = 0, st = 0;
    for (int64_t q = lo; q < hi; ++q) { sv += tv[q]; st += tt[q]; }
    int64_t totv, tott;
    int64_t ov = block_exclusive_scan<int64_t, MC_SCAN_THREADS>(sv, lds, &totv);
    int64_t ot = block_exclusive_scan<int64_t, MC_SCAN_THREADS>(st, lds, &tott);
    for (int64_t q = lo; q < hi; ++q) {
        const int64_t a = tv[q], b = tt[q];
        tv[q] = ov; tt[q] = ot;
        ov += a; ot += b;
    }
    if (threadIdx.x == 0) { totals[0] = totv; totals[1] = tott; }
}

struct McOut {
    float s[3], o[3];
    const float* col; int64_t cld;
    float* verts; int32_t* faces; float* normals; float* vcol;
};

__device__ __forceinline__ float mc_at(const McGrid& g, int64_t p) { return g.f[p * g.ld]; }

// np.gradient along axis b at point p (index pb of n): central differences inside, one-sided at the faces, / spacing
__device__ __forceinline__ float mc_grad(const McGrid& g, int64_t p, int64_t pb, int64_t n, int64_t step, float s) {
    if (pb == 0) return (mc_at(g, p + step) - mc_at(g, p)) / s;
    if (pb == n - 1) return (mc_at(g, p) - mc_at(g, p - step)) / s;
    return (mc_at(g, p + step) - mc_at(g, p - step)) / (2.f * s);
}

__global__ void __launch_bounds__(MC_BLOCK) mc_emit_verts_kernel(McGrid g, McWs w, McOut o) {
    __shared__ int32_t lds[MC_BLOCK / 64];
    const int64_t step[3] = {g.syz, g.nz, 1}, dim[3] = {g.nx, g.ny, g.nz};
    for (int64_t tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
        const int64_t item = tile * MC_BLOCK + threadIdx.x;
        int64_t row = 0, i = 0, j = 0, k0 = 0, p0 = 0;
        int np = 0, nv = 0;
        unsigned masks = 0;                                        // 3 bits per point
        if (item < g.ngroups) {
            mc_item(g, item, &row, &i, &j, &k0, &np);
            p0 = row * g.nz + k0;
            for (int t = 0; t < np; ++t) {
                const unsigned m = w.code[p0 + t] >> 8;
                masks |= m << (3 * t);
                nv += __builtin_popcount(m);
            }
        }
        int32_t tot;
        const int32_t ex = block_exclusive_scan<int32_t, MC_BLOCK>(nv, lds, &tot);
        int64_t vi = w.tv[tile] + ex;                              // < INT32_MAX: checked on the host before launch
        for (int t = 0; t < np; ++t) {
            const int64_t p = p0 + t;
            w.voff[p] = (int32_t)vi;
            const int64_t c[3] = {i, j, k0 + t};
            const unsigned m = masks >> (3 * t) & 7u;
            for (int a = 0; a < 3; ++a) {
                if (!(m >> a & 1u)) continue;
                const int64_t q = p + step[a];
                const float f0 = mc_at(g, p), f1 = mc_at(g, q);
                float tt = (g.level - f0) / (f1 - f0);
                if (!isfinite(tt)) tt = 0.5f;
                tt = fminf(fmaxf(tt, 0.f), 1.f);
                float nrm[3];
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    const int64_t cq = c[b] + (b == a ? 1 : 0);
                    const float g0 = mc_grad(g, p, c[b], dim[b], step[b], o.s[b]);
                    const float g1 = mc_grad(g, q, cq, dim[b], step[b], o.s[b]);
                    nrm[b] = -((1.f - tt) * g0 + tt * g1);
                    const float x = (b == a) ? ((float)c[b] + tt) * o.s[b] : (float)c[b] * o.s[b];
                    o.verts[3 * vi + b] = x + o.o[b];
                }
                const float len = sqrtf((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]);
                float r[3] = {nrm[0] / len, nrm[1] / len, nrm[2] / len};
                if (!(len > 0.f) || !isfinite(r[0]) || !isfinite(r[1]) || !isfinite(r[2])) r[0] = r[1] = r[2] = 0.f;
#pragma unroll
                for (int b = 0; b < 3; ++b) o.normals[3 * vi + b] = r[b];
                if (o.col) {
                    const float* src = o.col + (tt > 0.5f ? q : p) * o.cld;
#pragma unroll
                    for (int b = 0; b < 3; ++b) o.vcol[3 * vi + b] = src[b];
                }
                ++vi;
            }
        }
    }
}

__global__ void __launch_bounds__(MC_BLOCK) mc_emit_tris_kernel(McGrid g, McWs w, McOut o) {
    __shared__ int32_t lds[MC_BLOCK / 64];
    for (int64_t tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
        const int64_t item = tile * MC_BLOCK + threadIdx.x;
        int64_t row, i, j, k0, p0 = 0;
        int np = 0, nt = 0;
        if (item < g.ngroups) {
            mc_item(g, item, &row, &i, &j, &k0, &np);
            p0 = row * g.nz + k0;
            for (int t = 0; t < np; ++t) nt += sw_mc_ntri[w.code[p0 + t] & 0xff];
        }
        int32_t tot;
        const int32_t ex = block_exclusive_scan<int32_t, MC_BLOCK>(nt, lds, &tot);
        int64_t ti = w.tt[tile] + ex;
        for (int t = 0; t < np; ++t) {
            const int64_t p = p0 + t;
            const unsigned cs = w.code[p] & 0xffu;
            const int n = sw_mc_ntri[cs];
            for (int e3 = 0; e3 < 3 * n; ++e3) {
                const int e = sw_mc_tri[cs][e3], a = e >> 2;
                // base corner offset: (e & 1) along the lower other axis, (e >> 1 & 1) along the higher one
                const int64_t u = e & 1, v = e >> 1 & 1;
                const int64_t q = p + (a == 0 ? u * g.nz + v : (a == 1 ? u * g.syz + v : u * g.syz + v * g.nz));
                const unsigned m = w.code[q] >> 8;
                o.faces[3 * ti + e3] = w.voff[q] + __builtin_popcount(m & ((1u << a) - 1u));
            }
            ti += n;
        }
    }
}

static int mc_check_dims(const char* what, int64_t nx, int64_t ny, int64_t nz, int64_t ld) {
    if (nx < 2 || ny < 2 || nz < 2)
        return sw_fail(SWNERF_E_ARG, "%s: every grid dimension must be >= 2, got (%lld, %lld, %lld)", what, (long long)nx, (long long)ny, (long long)nz);
    if (ld < 1) return sw_fail(SWNERF_E_ARG, "%s: point stride ld must be >= 1, got %lld", what, (long long)ld);
    return 0;
}

static unsigned mc_blocks(int64_t ntiles) { return (unsigned)(ntiles < MC_MAX_GRID ? ntiles : MC_MAX_GRID); }

extern "C" size_t swnerf_mc_workspace_bytes(int64_t nx, int64_t ny, int64_t nz) {
    if (nx < 2 || ny < 2 || nz < 2) return 0;
    const McGrid g = mc_grid(nx, ny, nz);
    const int64_t N = nx * ny * nz;
    return (size_t)(mc_round256(2 * N) + mc_round256(4 * N) + 2 * mc_round256(8 * g.ntiles));
}

extern "C" int swnerf_mc_count(const float* field, int64_t nx, int64_t ny, int64_t nz, int64_t ld, float level,
                               void* workspace, int64_t* totals, void* stream) {
    int rc = mc_check_dims("mc_count", nx, ny, nz, ld);
    if (rc) return rc;
    if (!field || !workspace || !totals) return sw_fail(SWNERF_E_ARG, "mc_count: NULL pointer");
    McGrid g = mc_grid(nx, ny, nz);
    g.f = field; g.ld = ld; g.level = level;
    g.vec = (ld == 1 && nz % 4 == 0 && ((uintptr_t)field & 15) == 0) ? 1 : 0;
    const McWs w = mc_ws(workspace, g);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mc_classify_kernel, dim3(mc_blocks(g.ntiles)), dim3(MC_BLOCK), 0, st, g, w);
    rc = sw_check(hipGetLastError(), "mc_classify launch");
    if (rc) return rc;
    hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(MC_SCAN_THREADS), 0, st, g.ntiles, w.tv, w.tt, totals);
    return sw_check(hipGetLastError(), "mc_scan launch");
}

extern "C" int swnerf_mc_emit(const float* field, const float* colors, int64_t nx, int64_t ny, int64_t nz, int64_t ld,
                              int64_t colors_ld, float level, const float* spacing, const float* origin, void* workspace,
                              int64_t n_verts, int64_t n_tris, float* verts, int32_t* faces, float* normals,
                              float* vertex_colors, void* stream) {
    int rc = mc_check_dims("mc_emit", nx, ny, nz, ld);
    if (rc) return rc;
    if (n_verts < 0 || n_tris < 0 || n_verts > INT32_MAX || n_tris > INT32_MAX)
        return sw_fail(SWNERF_E_ARG, "mc_emit: %lld vertices / %lld triangles: int32 indices hold at most %d",
                       (long long)n_verts, (long long)n_tris, INT32_MAX);
    if (!field || !workspace || !spacing || !origin) return sw_fail(SWNERF_E_ARG, "mc_emit: NULL pointer");
    if (n_verts > 0 && (!verts || !normals)) return sw_fail(SWNERF_E_ARG, "mc_emit: NULL verts / normals");
    if (n_tris > 0 && !faces) return sw_fail(SWNERF_E_ARG, "mc_emit: NULL faces");
    if (colors && (colors_ld < 3 || (n_verts > 0 && !vertex_colors)))
        return sw_fail(SWNERF_E_ARG, "mc_emit: colours need colors_ld >= 3 (got %lld) and a vertex_colors output", (long long)colors_ld);
    if (n_verts == 0 && n_tris == 0) return 0;                     // an empty surface writes nothing
    McGrid g = mc_grid(nx, ny, nz);
    g.f = field; g.ld = ld; g.level = level; g.vec = 0;
    const McWs w = mc_ws(workspace, g);
    McOut o;
    for (int b = 0; b < 3; ++b) { o.s[b] = spacing[b]; o.o[b] = origin[b]; }
    o.col = colors; o.cld = colors_ld; o.verts = verts; o.faces = faces; o.normals = normals; o.vcol = vertex_colors;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(mc_blocks(g.ntiles)), block(MC_BLOCK);
    hipLaunchKernelGGL(mc_emit_verts_kernel, grid, block, 0, st, g, w, o);
    rc = sw_check(hipGetLastError(), "mc_emit_verts launch");
    if (rc) return rc;
    hipLaunchKernelGGL(mc_emit_tris_kernel, grid, block, 0, st, g, w, o);
    return sw_check(hipGetLastError(), "mc_emit_tris launch");
}
