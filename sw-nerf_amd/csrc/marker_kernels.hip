// marker_kernels.hip - square fiducial markers (ArUco-like, 4 x 4 payload in a one-cell black border) found in uint8 frames that
// are already on the device (nerf/transform_mesh.py: cv2.aruco's detectMarkers; DESIGN.md 6k "Markers").  The arithmetic lives in
// marker_math.h; tests/marker_ref.py restates it in numpy.  For each threshold radius:
//   grey        14-bit fixed-point luma, one thread per pixel
//   threshold   exact int32 box sums: a row pass through an LDS segment (uint16 row sums), then a column pass with a running sum
//               over bands of 32 rows; dark iff g cnt < s - C cnt
//   labels      8-connected union-find: 32 x 32 tiles merged in LDS, then unions across tile borders in global memory, then path
//               compression.  Every union links the larger root to the smaller, so the final label is the smallest linear index
//               of the component whatever the schedule, and a component may span any number of tiles.
//   components  area by atomicAdd on the root; the roots of at least min_area pixels are compacted in ascending label order with
//               a three-launch scan (at most H W / MARKER_MIN_AREA of them exist, which sizes the tables); then four passes over
//               the pixels with integer atomics only (64-bit sums, min/max, atomicMax on (value, index) keys): centroid and
//               bounding box, P1, P2, P3 / P4.  Integer sums and maxima do not depend on the order of arrival - nor on their
//               grouping: a wave whose pixels all name one component combines them first and issues one atomic (MkWave).
//   refinement  one wave per candidate, read from the compacted table whose length is in device memory: 96 edge points, four
//               total-least-squares lines (each summed by one lane in index order), corners, homography, 36 cells, payload
//   merge       per frame, radius by radius: a survivor is dropped when a survivor of a smaller radius has its centre within
//               4 px; the rest are numbered by a scan in (radius, label) order and the first K stored; count is the true number
// No allocation, no host synchronisation: the launch geometry depends on n, H, W only.  Frame-local pixel indices are int32
// (H, W <= 16384), every element offset is 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/swnerf.h"
#include "host_util.h"
#include "marker_math.h"
#include "par_prims.h"

#define MK_THREADS 256
#define MK_TILE 32                      // label tile side; 256 threads own 4 rows each
#define MK_BAND 32                      // rows per thread of the column pass
#define MK_CHUNK 1024                   // pixels per block of the root scan
#define MK_MAX_BLOCKS 65535
#define MK_CAND_INTS 11                 // label, area, flags, 4 corners: the rows swnerf_marker_candidates returns

struct MkCand {
    unsigned long long sumx, sumy, k1, k2, k3, k4;
    int label, area, xmin, ymin, xmax, ymax, cx2, cy2, p1x, p1y, p2x, p2y, flags;
    int corners[8];
    int pad;
};

struct MkFound {
    float quad[8];
    int payload;                        // -1: dropped
};

struct MkPlan {                         // the workspace, carved once on the host
    uint8_t* grey;
    uint8_t* mask;
    uint16_t* hsum;
    int32_t* labels;
    int32_t* slot;                      // per root: area, then the root's slot in the table (or -1); 0 elsewhere
    int32_t* blocksum;
    int32_t* ncand;                     // [MARKER_MAX_RADII][n]
    MkCand* cand;                       // [n][cap]
    MkFound* found;                     // [MARKER_MAX_RADII][n][cap]
    int64_t cap, nblk, bytes;
};

static inline int64_t mk_align(int64_t b) { return (b + 255) & ~(int64_t)255; }

static MkPlan mk_plan(void* ws, int64_t n, int64_t H, int64_t W) {
    MkPlan P;
    const int64_t px = n * H * W;
    P.cap = H * W / MARKER_MIN_AREA + 1;
    P.nblk = (H * W + MK_CHUNK - 1) / MK_CHUNK;
    char* base = static_cast<char*>(ws);
    int64_t off = 0;
    auto take = [&](int64_t bytes) { char* p = base + off; off += mk_align(bytes); return p; };
    P.grey = reinterpret_cast<uint8_t*>(take(px));
    P.mask = reinterpret_cast<uint8_t*>(take(px));
    P.hsum = reinterpret_cast<uint16_t*>(take(px * 2));
    P.labels = reinterpret_cast<int32_t*>(take(px * 4));
    P.slot = reinterpret_cast<int32_t*>(take(px * 4));
    P.blocksum = reinterpret_cast<int32_t*>(take(n * P.nblk * 4));
    P.ncand = reinterpret_cast<int32_t*>(take(MARKER_MAX_RADII * n * 4));
    P.cand = reinterpret_cast<MkCand*>(take(n * P.cap * (int64_t)sizeof(MkCand)));
    P.found = reinterpret_cast<MkFound*>(take(MARKER_MAX_RADII * n * P.cap * (int64_t)sizeof(MkFound)));
    P.bytes = off;
    return P;
}

// exclusive scan of one int per thread over the 256 threads of a workgroup; *total = the sum.  Every thread must call it.
__device__ __forceinline__ int mk_block_scan(int v, int* lds, int* total) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int d = 1; d < MK_THREADS; d <<= 1) {
        const int add = t >= d ? lds[t - d] : 0;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    const int incl = lds[t];
    *total = lds[MK_THREADS - 1];
    __syncthreads();
    return incl - v;
}

// ---- grey --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MK_THREADS) void mk_grey_kernel(const uint8_t* __restrict__ frames, int64_t total, int c,
                                                              uint8_t* __restrict__ grey) {
    for (int64_t p = (int64_t)blockIdx.x * MK_THREADS + threadIdx.x; p < total; p += (int64_t)gridDim.x * MK_THREADS) {
        const uint8_t* s = frames + p * c;
        grey[p] = c == 1 ? s[0] : (uint8_t)marker_luma(s[0], s[1], s[2]);
    }
}

// ---- threshold ---------------------------------------------------------------------------------------------------------
// row sums over [x - r, x + r] clipped to the row.  grid (ceil(W / 256), rows)
__global__ __launch_bounds__(MK_THREADS) void mk_hsum_kernel(const uint8_t* __restrict__ grey, int64_t rows, int W, int r,
                                                              uint16_t* __restrict__ hsum) {
    __shared__ uint8_t seg[MK_THREADS + 2 * MARKER_MAX_RADIUS];
    const int x0 = blockIdx.x * MK_THREADS;
    for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
        const uint8_t* G = grey + row * W;
        for (int t = threadIdx.x; t < MK_THREADS + 2 * r; t += MK_THREADS) {
            const int x = x0 - r + t;
            seg[t] = (x >= 0 && x < W) ? G[x] : 0;
        }
        __syncthreads();
        const int x = x0 + threadIdx.x;
        if (x < W) {
            int s = 0;
            for (int k = 0; k <= 2 * r; ++k) s += seg[threadIdx.x + k];
            hsum[row * W + x] = (uint16_t)s;
        }
        __syncthreads();
    }
}

// column pass + the test.  grid (ceil(W / 256), ceil(H / MK_BAND), n)
__global__ __launch_bounds__(MK_THREADS) void mk_threshold_kernel(const uint8_t* __restrict__ grey, const uint16_t* __restrict__ hsum,
                                                                   int H, int W, int r, int C, uint8_t* __restrict__ mask) {
    const int x = blockIdx.x * MK_THREADS + threadIdx.x;
    if (x >= W) return;
    const int64_t f = (int64_t)blockIdx.z * H * W;
    const int y0 = blockIdx.y * MK_BAND;
    const int cx = marker_window(x, r, W);
    int s = 0;
    for (int y = max(y0 - r, 0); y <= min(y0 + r, H - 1); ++y) s += hsum[f + (int64_t)y * W + x];
    for (int y = y0; y < min(y0 + MK_BAND, H); ++y) {
        const int64_t e = f + (int64_t)y * W + x;
        mask[e] = marker_dark(grey[e], s, cx * marker_window(y, r, H), C) ? 1 : 0;
        if (y + r + 1 < H) s += hsum[e + (int64_t)(r + 1) * W];
        if (y - r >= 0) s -= hsum[e - (int64_t)r * W];
    }
}

// ---- labels (uf_find / uf_union of par_prims.h) ------------------------------------------------------------------------
// grid (ceil(W / 32), ceil(H / 32), n), 256 threads as 32 x 8
__global__ __launch_bounds__(MK_THREADS) void mk_label_tile_kernel(const uint8_t* __restrict__ mask, int H, int W, int32_t* __restrict__ labels) {
    __shared__ int L[MK_TILE * MK_TILE];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int gx = blockIdx.x * MK_TILE + tx, gy0 = blockIdx.y * MK_TILE;
    const int64_t f = (int64_t)blockIdx.z * H * W;
    bool dark[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = ty + 8 * k, gy = gy0 + r;
        dark[k] = gx < W && gy < H && mask[f + (int64_t)gy * W + gx] != 0;
        L[r * MK_TILE + tx] = dark[k] ? r * MK_TILE + tx : -1;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = ty + 8 * k, me = r * MK_TILE + tx;
        if (!dark[k]) continue;
        if (tx > 0 && L[me - 1] >= 0) uf_union(L, me, me - 1);
        if (r > 0) {
            if (tx > 0 && L[me - MK_TILE - 1] >= 0) uf_union(L, me, me - MK_TILE - 1);
            if (L[me - MK_TILE] >= 0) uf_union(L, me, me - MK_TILE);
            if (tx < MK_TILE - 1 && L[me - MK_TILE + 1] >= 0) uf_union(L, me, me - MK_TILE + 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = ty + 8 * k, gy = gy0 + r;
        if (gx >= W || gy >= H) continue;
        int out = -1;
        if (dark[k]) {
            const int root = uf_find(L, r * MK_TILE + tx);
            out = (gy0 + (root >> 5)) * W + blockIdx.x * MK_TILE + (root & 31);
        }
        labels[f + (int64_t)gy * W + gx] = out;
    }
}

// unions across tile borders: a dark pixel in a tile's first row or column, or in its last column (for the neighbour up and to the
// right), joins the dark neighbours W, NW, N, NE that lie in another tile.  One thread per pixel; grid (blocks, n)
__global__ __launch_bounds__(MK_THREADS) void mk_label_border_kernel(int H, int W, int32_t* labels) {
    int* L = labels + (int64_t)blockIdx.y * H * W;
    const int HW = H * W;
    for (int p = blockIdx.x * MK_THREADS + threadIdx.x; p < HW; p += gridDim.x * MK_THREADS) {
        const int y = p / W, x = p - y * W;
        const bool col0 = (x & (MK_TILE - 1)) == 0, row0 = (y & (MK_TILE - 1)) == 0, col31 = (x & (MK_TILE - 1)) == MK_TILE - 1;
        if (!(col0 || row0 || col31) || L[p] < 0) continue;
        if (col0 && x > 0 && L[p - 1] >= 0) uf_union(L, p, p - 1);
        if (y > 0) {
            if ((col0 || row0) && x > 0 && L[p - W - 1] >= 0) uf_union(L, p, p - W - 1);
            if (row0 && L[p - W] >= 0) uf_union(L, p, p - W);
            if ((col31 || row0) && x + 1 < W && L[p - W + 1] >= 0) uf_union(L, p, p - W + 1);
        }
    }
}

__global__ __launch_bounds__(MK_THREADS) void mk_label_flatten_kernel(int H, int W, int32_t* labels) {
    int* L = labels + (int64_t)blockIdx.y * H * W;
    const int HW = H * W;
    for (int p = blockIdx.x * MK_THREADS + threadIdx.x; p < HW; p += gridDim.x * MK_THREADS)
        if (L[p] >= 0) {
            const int root = uf_find(L, p);
            if (root != p) __atomic_store_n(L + p, root, __ATOMIC_RELAXED);
        }
}

// ---- components --------------------------------------------------------------------------------------------------------
// Atomics on one address serialise, and the pixels of a wave are 64 neighbours of one row: mostly one component.  When every lane
// that has something to add names the same target, the wave combines its values with shuffles and one lane issues the atomics;
// integer sums and maxima are the same whichever way they are grouped.
struct MkWave {
    int leader;                         // the first lane with a target
    bool uniform;                       // all lanes with a target share it
};

__device__ __forceinline__ MkWave mk_wave_targets(int target) {           // target < 0: nothing to add; called by whole waves
    MkWave w;
    const unsigned long long have = __ballot(target >= 0);
    w.leader = have ? __ffsll((long long)have) - 1 : 0;
    const int t0 = __shfl(target, w.leader);
    w.uniform = have != 0 && __ballot(target >= 0 && target != t0) == 0;
    return w;
}

__device__ __forceinline__ int mk_wave_sum(int v) {
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ int mk_wave_min(int v) {
    for (int d = 32; d; d >>= 1) v = min(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ int mk_wave_max(int v) {
    for (int d = 32; d; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ unsigned long long mk_wave_max64(unsigned long long v) {
    for (int d = 32; d; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(MK_THREADS) void mk_area_kernel(const int32_t* __restrict__ labels, int HW, int32_t* slot) {
    const int64_t f = (int64_t)blockIdx.y * HW;
    const int lane = threadIdx.x & 63;
    for (int p = blockIdx.x * MK_THREADS + threadIdx.x; p - lane < HW; p += gridDim.x * MK_THREADS) {   // uniform over a wave
        const int l = p < HW ? labels[f + p] : -1;
        const MkWave w = mk_wave_targets(l);
        if (w.uniform) {
            const int cnt = __popcll(__ballot(l >= 0));
            if (lane == w.leader) atomicAdd(slot + f + l, cnt);
        } else if (l >= 0) {
            atomicAdd(slot + f + l, 1);
        }
    }
}

__device__ __forceinline__ bool mk_is_kept_root(const int32_t* labels, const int32_t* slot, int64_t f, int p, int HW, int min_area) {
    return p < HW && labels[f + p] == p && slot[f + p] >= min_area;
}

// grid (nblk, n): kept roots per chunk of 1024 pixels (4 consecutive pixels per thread)
__global__ __launch_bounds__(MK_THREADS) void mk_root_count_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ slot,
                                                                    int HW, int min_area, int nblk, int32_t* __restrict__ blocksum) {
    __shared__ int lds[MK_THREADS];
    const int64_t f = (int64_t)blockIdx.y * HW;
    const int p0 = blockIdx.x * MK_CHUNK + threadIdx.x * 4;
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) c += mk_is_kept_root(labels, slot, f, p0 + k, HW, min_area) ? 1 : 0;
    int total;
    mk_block_scan(c, lds, &total);
    if (threadIdx.x == 0) blocksum[(int64_t)blockIdx.y * nblk + blockIdx.x] = total;
}

// grid n: exclusive scan of a frame's chunk counts in place; ncand = the total
__global__ __launch_bounds__(MK_THREADS) void mk_root_offsets_kernel(int nblk, int32_t* blocksum, int cap, int32_t* __restrict__ ncand) {
    __shared__ int lds[MK_THREADS];
    int32_t* B = blocksum + (int64_t)blockIdx.x * nblk;
    int base = 0;
    for (int b0 = 0; b0 < nblk; b0 += MK_THREADS) {
        const int b = b0 + threadIdx.x;
        const int v = b < nblk ? B[b] : 0;
        int total;
        const int ex = mk_block_scan(v, lds, &total);
        if (b < nblk) B[b] = base + ex;
        base += total;
    }
    if (threadIdx.x == 0) ncand[blockIdx.x] = base < cap ? base : cap;   // base <= H W / min_area < cap: the clamp never binds
}

// grid (nblk, n): number the kept roots, start their table rows, turn slot[] from areas into slots
__global__ __launch_bounds__(MK_THREADS) void mk_root_assign_kernel(const int32_t* __restrict__ labels, int32_t* slot, int HW, int W,
                                                                     int min_area, int nblk, const int32_t* __restrict__ blocksum,
                                                                     int cap, MkCand* __restrict__ cand) {
    __shared__ int lds[MK_THREADS];
    const int64_t f = (int64_t)blockIdx.y * HW;
    const int p0 = blockIdx.x * MK_CHUNK + threadIdx.x * 4;
    bool keep[4];
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        keep[k] = mk_is_kept_root(labels, slot, f, p0 + k, HW, min_area);
        c += keep[k] ? 1 : 0;
    }
    int total;
    int at = blocksum[(int64_t)blockIdx.y * nblk + blockIdx.x] + mk_block_scan(c, lds, &total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = p0 + k;
        if (p >= HW || labels[f + p] != p) continue;                       // only roots hold an area
        int s = -1;
        if (keep[k] && at < cap) {
            s = at;
            MkCand* c0 = cand + (int64_t)blockIdx.y * cap + s;
            c0->sumx = c0->sumy = c0->k1 = c0->k2 = c0->k3 = c0->k4 = 0ull;
            c0->label = p;
            c0->area = slot[f + p];
            c0->xmin = c0->ymin = MARKER_MAX_SIDE;
            c0->xmax = c0->ymax = -1;
            c0->flags = 0;
        }
        if (keep[k]) ++at;
        slot[f + p] = s;
    }
}

// the four pixel passes.  PASS 1: sums and bounding box, 2: P1, 3: P2, 4: P3 and P4.  grid (blocks, n)
template <int PASS>
__global__ __launch_bounds__(MK_THREADS) void mk_reduce_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ slot,
                                                               int HW, int W, int cap, MkCand* cand) {
    const int64_t f = (int64_t)blockIdx.y * HW;
    MkCand* Cf = cand + (int64_t)blockIdx.y * cap;
    const int lane = threadIdx.x & 63;
    for (int p = blockIdx.x * MK_THREADS + threadIdx.x; p - lane < HW; p += gridDim.x * MK_THREADS) {   // uniform over a wave
        const int l = p < HW ? labels[f + p] : -1;
        const int s = l >= 0 ? slot[f + l] : -1;
        const MkWave w = mk_wave_targets(s);
        if (!w.uniform && s < 0) continue;                                  // in a uniform wave every lane takes part in the shuffles
        const bool on = s >= 0;
        const bool lead = w.uniform && lane == w.leader;
        MkCand* c = Cf + (on ? s : 0);
        const int y = on ? p / W : 0, x = on ? p - y * W : 0;
        if (PASS == 1) {
            if (w.uniform) {
                const int sx = mk_wave_sum(x), sy = mk_wave_sum(y);         // at most 64 * 16383
                const int x0 = mk_wave_min(on ? x : MARKER_MAX_SIDE), y0 = mk_wave_min(on ? y : MARKER_MAX_SIDE);
                const int x1 = mk_wave_max(on ? x : -1), y1 = mk_wave_max(on ? y : -1);
                if (lead) {
                    atomicAdd(&c->sumx, (unsigned long long)sx);
                    atomicAdd(&c->sumy, (unsigned long long)sy);
                    atomicMin(&c->xmin, x0);
                    atomicMin(&c->ymin, y0);
                    atomicMax(&c->xmax, x1);
                    atomicMax(&c->ymax, y1);
                }
            } else {
                atomicAdd(&c->sumx, (unsigned long long)x);
                atomicAdd(&c->sumy, (unsigned long long)y);
                atomicMin(&c->xmin, x);
                atomicMin(&c->ymin, y);
                atomicMax(&c->xmax, x);
                atomicMax(&c->ymax, y);
            }
        } else if (PASS == 2 || PASS == 3) {
            unsigned long long key = 0ull;                                  // below every real key
            if (on) {
                const int dx = PASS == 2 ? 2 * x - c->cx2 : x - c->p1x, dy = PASS == 2 ? 2 * y - c->cy2 : y - c->p1y;
                key = marker_key((uint32_t)(dx * dx + dy * dy), (uint32_t)p);
            }
            unsigned long long* dst = PASS == 2 ? &c->k1 : &c->k2;
            if (w.uniform) {
                key = mk_wave_max64(key);
                if (lead) atomicMax(dst, key);
            } else {
                atomicMax(dst, key);
            }
        } else {
            unsigned long long kp = 0ull, kn = 0ull;
            if (on) {
                const int cr = (c->p2x - c->p1x) * (y - c->p1y) - (c->p2y - c->p1y) * (x - c->p1x);
                if (cr > 0) kp = marker_key((uint32_t)cr, (uint32_t)p);
                if (cr < 0) kn = marker_key((uint32_t)(-cr), (uint32_t)p);
            }
            if (w.uniform) {
                kp = mk_wave_max64(kp);
                kn = mk_wave_max64(kn);
                if (lead && kp) atomicMax(&c->k3, kp);
                if (lead && kn) atomicMax(&c->k4, kn);
            } else {
                if (kp) atomicMax(&c->k3, kp);
                if (kn) atomicMax(&c->k4, kn);
            }
        }
    }
}

// per-candidate step after pass PASS.  grid (blocks, n)
template <int PASS>
__global__ __launch_bounds__(MK_THREADS) void mk_finish_kernel(const int32_t* __restrict__ ncand, int H, int W, int min_area, int cap,
                                                               MkCand* cand) {
    const int m = ncand[blockIdx.y];
    for (int s = blockIdx.x * MK_THREADS + threadIdx.x; s < m; s += gridDim.x * MK_THREADS) {
        MkCand* c = cand + (int64_t)blockIdx.y * cap + s;
        if (PASS == 1) {
            c->cx2 = marker_centre2((int64_t)c->sumx, c->area);
            c->cy2 = marker_centre2((int64_t)c->sumy, c->area);
            if (c->xmin == 0 || c->ymin == 0 || c->xmax == W - 1 || c->ymax == H - 1) c->flags |= MARKER_FLAG_BORDER;
        } else if (PASS == 2) {
            const int p = (int)marker_key_index(c->k1);                    // area >= 16: some pixel is off the centroid, k1 != 0
            c->p1y = p / W;
            c->p1x = p - c->p1y * W;
        } else if (PASS == 3) {
            const int p = (int)marker_key_index(c->k2);
            c->p2y = p / W;
            c->p2x = p - c->p2y * W;
        } else {
            const int cp = (int)marker_key_value(c->k3), cn = (int)marker_key_value(c->k4);
            int x3 = 0, y3 = 0, x4 = 0, y4 = 0;
            if (cp > 0) {
                const int p = (int)marker_key_index(c->k3);
                y3 = p / W;
                x3 = p - y3 * W;
            }
            if (cn > 0) {
                const int p = (int)marker_key_index(c->k4);
                y4 = p / W;
                x4 = p - y4 * W;
            }
            if (cp == 0 || cn == 0) c->flags |= MARKER_FLAG_ONE_SIDED;
            if (cp + cn < 2 * min_area) c->flags |= MARKER_FLAG_SMALL_QUAD;
            // clockwise with y down: P1, the point on the negative side, P2, the point on the positive side
            c->corners[0] = c->p1x; c->corners[1] = c->p1y;
            c->corners[2] = x4;     c->corners[3] = y4;
            c->corners[4] = c->p2x; c->corners[5] = c->p2y;
            c->corners[6] = x3;     c->corners[7] = y3;
        }
    }
}

// rows of swnerf_marker_candidates.  grid (blocks, n)
__global__ __launch_bounds__(MK_THREADS) void mk_export_kernel(const int32_t* __restrict__ ncand, int cap, const MkCand* __restrict__ cand,
                                                               int out_cap, int32_t* __restrict__ rows, int32_t* __restrict__ count) {
    const int m = ncand[blockIdx.y];
    if (blockIdx.x == 0 && threadIdx.x == 0) count[blockIdx.y] = m;
    for (int s = blockIdx.x * MK_THREADS + threadIdx.x; s < m && s < out_cap; s += gridDim.x * MK_THREADS) {
        const MkCand* c = cand + (int64_t)blockIdx.y * cap + s;
        int32_t* o = rows + ((int64_t)blockIdx.y * out_cap + s) * MK_CAND_INTS;
        o[0] = c->label;
        o[1] = c->area;
        o[2] = c->flags;
        for (int k = 0; k < 8; ++k) o[3 + k] = c->corners[k];
    }
}

// ---- refinement and decoding: one wave (one 64-thread workgroup) per candidate.  grid (blocks, n) -------------------------
__global__ __launch_bounds__(64) void mk_refine_kernel(const uint8_t* __restrict__ grey, int H, int W, const int32_t* __restrict__ ncand,
                                                       int cap, const MkCand* __restrict__ cand, MkFound* __restrict__ found) {
    __shared__ float px[4 * MARKER_SIDE_POINTS], py[4 * MARKER_SIDE_POINTS];
    __shared__ int valid[4 * MARKER_SIDE_POINTS];
    __shared__ float lines[4][4], q[8], cell[36];
    __shared__ int ok[8];
    const uint8_t* G = grey + (int64_t)blockIdx.y * H * W;
    const int lane = threadIdx.x;
    const int m = ncand[blockIdx.y];                                        // the table's length, read from device memory
    for (int s = blockIdx.x; s < m; s += gridDim.x) {                       // uniform over the wave
        const MkCand* c = cand + (int64_t)blockIdx.y * cap + s;
        MkFound* out = found + (int64_t)blockIdx.y * cap + s;
        if (c->flags != 0) {
            if (lane == 0) out->payload = -1;
            continue;
        }
        float cx[4], cy[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cx[k] = (float)c->corners[2 * k] + 0.5f;
            cy[k] = (float)c->corners[2 * k + 1] + 0.5f;
        }
        for (int pt = lane; pt < 4 * MARKER_SIDE_POINTS; pt += 64) {
            float x = 0.f, y = 0.f;
            const int v = marker_side_point<float>(G, H, W, cx, cy, pt, &x, &y) ? 1 : 0;
            px[pt] = x;
            py[pt] = y;
            valid[pt] = v;
        }
        __syncthreads();
        if (lane < 4) {
            const int cnt = marker_fit_line<float>(px + lane * MARKER_SIDE_POINTS, py + lane * MARKER_SIDE_POINTS,
                                                   valid + lane * MARKER_SIDE_POINTS, MARKER_SIDE_POINTS, lines[lane]);
            ok[lane] = cnt >= MARKER_MIN_LINE_POINTS;
        }
        __syncthreads();
        if (lane < 4) {
            float x = 0.f, y = 0.f;
            ok[4 + lane] = (ok[(lane + 3) & 3] && ok[lane]) ? (marker_intersect<float>(lines[(lane + 3) & 3], lines[lane], &x, &y) ? 1 : 0) : 0;
            q[2 * lane] = x;
            q[2 * lane + 1] = y;
        }
        __syncthreads();
        bool good = true;
#pragma unroll
        for (int k = 0; k < 8; ++k) good = good && ok[k] != 0;
        float h[8];
        marker_square_to_quad<float>(q, h);
#pragma unroll
        for (int k = 0; k < 8; ++k) good = good && isfinite(h[k]);
        if (lane < 36) {
            float x, y;
            marker_cell_point<float>(h, lane, &x, &y);
            cell[lane] = good ? marker_bilinear<float>(G, H, W, x, y) : 0.f;
        }
        __syncthreads();
        if (lane == 0) {
            for (int k = 0; k < 8; ++k) out->quad[k] = q[k];
            out->payload = good ? marker_decode<float>(cell) : -1;
        }
        __syncthreads();                                                    // the LDS arrays are reused by the next candidate
    }
}

// ---- merge across radii and store.  grid n, 256 threads ------------------------------------------------------------------
__global__ __launch_bounds__(MK_THREADS) void mk_merge_kernel(int64_t n, int nradii, const int32_t* __restrict__ ncand, int cap,
                                                              const MkFound* __restrict__ found, int K, float* __restrict__ quads,
                                                              int32_t* __restrict__ payload, int32_t* __restrict__ count) {
    __shared__ int lds[MK_THREADS];
    const int64_t f = blockIdx.x;
    int base = 0;
    for (int ri = 0; ri < nradii; ++ri) {
        const MkFound* F = found + ((int64_t)ri * n + f) * cap;
        const int m = ncand[(int64_t)ri * n + f];
        for (int s0 = 0; s0 < m; s0 += MK_THREADS) {                        // uniform: every thread reaches the scan
            const int s = s0 + threadIdx.x;
            bool keep = s < m && F[s].payload >= 0;
            if (keep) {
                float mx = 0.f, my = 0.f;
                for (int k = 0; k < 4; ++k) {
                    mx += F[s].quad[2 * k];
                    my += F[s].quad[2 * k + 1];
                }
                mx *= 0.25f;
                my *= 0.25f;
                for (int rj = 0; rj < ri && keep; ++rj) {
                    const MkFound* E = found + ((int64_t)rj * n + f) * cap;
                    const int me = ncand[(int64_t)rj * n + f];
                    for (int e = 0; e < me; ++e) {
                        if (E[e].payload < 0) continue;
                        float ex = 0.f, ey = 0.f;
                        for (int k = 0; k < 4; ++k) {
                            ex += E[e].quad[2 * k];
                            ey += E[e].quad[2 * k + 1];
                        }
                        ex = ex * 0.25f - mx;
                        ey = ey * 0.25f - my;
                        if (!(ex * ex + ey * ey > (float)(MARKER_MERGE_DIST * MARKER_MERGE_DIST))) {
                            keep = false;
                            break;
                        }
                    }
                }
            }
            int total;
            const int at = base + mk_block_scan(keep ? 1 : 0, lds, &total);
            if (keep && at < K) {                                           // the only stores into the K-sized outputs
                for (int k = 0; k < 8; ++k) quads[(f * K + at) * 8 + k] = F[s].quad[k];
                payload[f * K + at] = F[s].payload;
            }
            base += total;
        }
    }
    if (threadIdx.x == 0) count[f] = base;
}

// ---- host --------------------------------------------------------------------------------------------------------------
static int mk_check_size(const char* who, int64_t n, int64_t H, int64_t W) {
    if (n < 0) return sw_fail(SWNERF_E_ARG, "%s: negative frame count %lld", who, (long long)n);
    if (H < 1 || W < 1 || H > MARKER_MAX_SIDE || W > MARKER_MAX_SIDE)
        return sw_fail(SWNERF_E_ARG, "%s: frame size %lld x %lld outside 1..%d", who, (long long)H, (long long)W, MARKER_MAX_SIDE);
    if (n > MK_MAX_BLOCKS) return sw_fail(SWNERF_E_ARG, "%s: %lld frames in one call; at most %d", who, (long long)n, MK_MAX_BLOCKS);
    return 0;
}

static unsigned mk_blocks(int64_t items, int per_block) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b > MK_MAX_BLOCKS ? MK_MAX_BLOCKS : b));
}

static int mk_check_ws(const char* who, const void* ws) {
    if (!ws) return sw_fail(SWNERF_E_ARG, "%s: NULL workspace", who);
    if ((uintptr_t)ws & 255) return sw_fail(SWNERF_E_ARG, "%s: the workspace must be 256-byte aligned", who);
    return 0;
}

static void mk_run_grey(const uint8_t* frames, int64_t n, int64_t H, int64_t W, int c, uint8_t* grey, hipStream_t st) {
    hipLaunchKernelGGL(mk_grey_kernel, dim3(mk_blocks(n * H * W, MK_THREADS)), dim3(MK_THREADS), 0, st, frames, n * H * W, c, grey);
}

static void mk_run_threshold(const MkPlan& P, const uint8_t* grey, int64_t n, int H, int W, int r, int C, uint8_t* mask, hipStream_t st) {
    hipLaunchKernelGGL(mk_hsum_kernel, dim3((W + MK_THREADS - 1) / MK_THREADS, mk_blocks(n * H, 1)), dim3(MK_THREADS), 0, st, grey,
                       n * H, W, r, P.hsum);
    hipLaunchKernelGGL(mk_threshold_kernel, dim3((W + MK_THREADS - 1) / MK_THREADS, (H + MK_BAND - 1) / MK_BAND, (unsigned)n),
                       dim3(MK_THREADS), 0, st, grey, P.hsum, H, W, r, C, mask);
}

static void mk_run_label(const uint8_t* mask, int64_t n, int H, int W, int32_t* labels, hipStream_t st) {
    const dim3 px(mk_blocks((int64_t)H * W, MK_THREADS), (unsigned)n);
    hipLaunchKernelGGL(mk_label_tile_kernel, dim3((W + MK_TILE - 1) / MK_TILE, (H + MK_TILE - 1) / MK_TILE, (unsigned)n), dim3(MK_THREADS),
                       0, st, mask, H, W, labels);
    hipLaunchKernelGGL(mk_label_border_kernel, px, dim3(MK_THREADS), 0, st, H, W, labels);
    hipLaunchKernelGGL(mk_label_flatten_kernel, px, dim3(MK_THREADS), 0, st, H, W, labels);
}

// labels -> the candidate table of this plan; ncand = P.ncand + ri * n
static int mk_run_components(const MkPlan& P, const int32_t* labels, int64_t n, int H, int W, int min_area, int32_t* ncand, hipStream_t st) {
    const int HW = H * W, cap = (int)P.cap, nblk = (int)P.nblk;
    const dim3 px(mk_blocks(HW, MK_THREADS), (unsigned)n), chunks((unsigned)nblk, (unsigned)n), per_cand(mk_blocks(cap, MK_THREADS), (unsigned)n);
    int rc = sw_check(hipMemsetAsync(P.slot, 0, (size_t)n * HW * 4, st), "marker: clearing the area table");
    if (rc) return rc;
    hipLaunchKernelGGL(mk_area_kernel, px, dim3(MK_THREADS), 0, st, labels, HW, P.slot);
    hipLaunchKernelGGL(mk_root_count_kernel, chunks, dim3(MK_THREADS), 0, st, labels, P.slot, HW, min_area, nblk, P.blocksum);
    hipLaunchKernelGGL(mk_root_offsets_kernel, dim3((unsigned)n), dim3(MK_THREADS), 0, st, nblk, P.blocksum, cap, ncand);
    hipLaunchKernelGGL(mk_root_assign_kernel, chunks, dim3(MK_THREADS), 0, st, labels, P.slot, HW, W, min_area, nblk, P.blocksum, cap, P.cand);
    hipLaunchKernelGGL(mk_reduce_kernel<1>, px, dim3(MK_THREADS), 0, st, labels, P.slot, HW, W, cap, P.cand);
    hipLaunchKernelGGL(mk_finish_kernel<1>, per_cand, dim3(MK_THREADS), 0, st, ncand, H, W, min_area, cap, P.cand);
    hipLaunchKernelGGL(mk_reduce_kernel<2>, px, dim3(MK_THREADS), 0, st, labels, P.slot, HW, W, cap, P.cand);
    hipLaunchKernelGGL(mk_finish_kernel<2>, per_cand, dim3(MK_THREADS), 0, st, ncand, H, W, min_area, cap, P.cand);
    hipLaunchKernelGGL(mk_reduce_kernel<3>, px, dim3(MK_THREADS), 0, st, labels, P.slot, HW, W, cap, P.cand);
    hipLaunchKernelGGL(mk_finish_kernel<3>, per_cand, dim3(MK_THREADS), 0, st, ncand, H, W, min_area, cap, P.cand);
    hipLaunchKernelGGL(mk_reduce_kernel<4>, px, dim3(MK_THREADS), 0, st, labels, P.slot, HW, W, cap, P.cand);
    hipLaunchKernelGGL(mk_finish_kernel<4>, per_cand, dim3(MK_THREADS), 0, st, ncand, H, W, min_area, cap, P.cand);
    return sw_check(hipGetLastError(), "marker component launches");
}

static int mk_check_params(const char* who, int r, int C, int min_area) {
    if (r < 1 || r > MARKER_MAX_RADIUS) return sw_fail(SWNERF_E_ARG, "%s: window radius %d outside 1..%d", who, r, MARKER_MAX_RADIUS);
    if (C < -255 || C > 255) return sw_fail(SWNERF_E_ARG, "%s: threshold offset %d outside -255..255", who, C);
    if (min_area < MARKER_MIN_AREA) return sw_fail(SWNERF_E_ARG, "%s: min_area %d below %d (it sizes the workspace)", who, min_area, MARKER_MIN_AREA);
    return 0;
}

extern "C" int64_t swnerf_marker_workspace_bytes(int64_t n, int64_t H, int64_t W) {
    if (n < 1 || H < 1 || W < 1 || H > MARKER_MAX_SIDE || W > MARKER_MAX_SIDE || n > MK_MAX_BLOCKS) return 0;
    return mk_plan(nullptr, n, H, W).bytes;
}

extern "C" int swnerf_marker_mask(const uint8_t* frames, int64_t n, int64_t H, int64_t W, int c, int radius, int C, void* workspace,
                                  uint8_t* grey, uint8_t* mask, void* stream) {
    int rc = mk_check_size("marker_mask", n, H, W);
    if (rc) return rc;
    if (c != 1 && c != 3 && c != 4) return sw_fail(SWNERF_E_ARG, "marker_mask: %d channels; 1, 3 and 4 are built", c);
    if ((rc = mk_check_params("marker_mask", radius, C, MARKER_MIN_AREA))) return rc;
    if (n == 0) return 0;
    if (!frames || !grey || !mask) return sw_fail(SWNERF_E_ARG, "marker_mask: NULL pointer");
    if ((rc = mk_check_ws("marker_mask", workspace))) return rc;
    const MkPlan P = mk_plan(workspace, n, H, W);
    hipStream_t st = (hipStream_t)stream;
    mk_run_grey(frames, n, H, W, c, grey, st);
    mk_run_threshold(P, grey, n, (int)H, (int)W, radius, C, mask, st);
    return sw_check(hipGetLastError(), "marker_mask launch");
}

extern "C" int swnerf_marker_label(const uint8_t* mask, int64_t n, int64_t H, int64_t W, int32_t* labels, void* stream) {
    int rc = mk_check_size("marker_label", n, H, W);
    if (rc) return rc;
    if (n == 0) return 0;
    if (!mask || !labels) return sw_fail(SWNERF_E_ARG, "marker_label: NULL pointer");
    if ((uintptr_t)labels & 3) return sw_fail(SWNERF_E_ARG, "marker_label: labels must be 4-byte aligned");
    mk_run_label(mask, n, (int)H, (int)W, labels, (hipStream_t)stream);
    return sw_check(hipGetLastError(), "marker_label launch");
}

extern "C" int swnerf_marker_candidates(const int32_t* labels, int64_t n, int64_t H, int64_t W, int min_area, void* workspace,
                                        int64_t capacity, int32_t* rows, int32_t* count, void* stream) {
    int rc = mk_check_size("marker_candidates", n, H, W);
    if (rc) return rc;
    if ((rc = mk_check_params("marker_candidates", 1, 0, min_area))) return rc;
    if (capacity < 0 || capacity > INT32_MAX) return sw_fail(SWNERF_E_ARG, "marker_candidates: capacity %lld", (long long)capacity);
    if (n == 0) return 0;
    if (!labels || !count || (capacity && !rows)) return sw_fail(SWNERF_E_ARG, "marker_candidates: NULL pointer");
    if (((uintptr_t)labels | (uintptr_t)rows | (uintptr_t)count) & 3) return sw_fail(SWNERF_E_ARG, "marker_candidates: operands must be 4-byte aligned");
    if ((rc = mk_check_ws("marker_candidates", workspace))) return rc;
    const MkPlan P = mk_plan(workspace, n, H, W);
    hipStream_t st = (hipStream_t)stream;
    if ((rc = mk_run_components(P, labels, n, (int)H, (int)W, min_area, P.ncand, st))) return rc;
    hipLaunchKernelGGL(mk_export_kernel, dim3(mk_blocks(P.cap, MK_THREADS), (unsigned)n), dim3(MK_THREADS), 0, st, P.ncand, (int)P.cap,
                       P.cand, (int)capacity, rows, count);
    return sw_check(hipGetLastError(), "marker_candidates launch");
}

extern "C" int swnerf_marker_detect(const uint8_t* frames, int64_t n, int64_t H, int64_t W, int c, const int* radii, int nradii, int C,
                                    int min_area, int K, void* workspace, float* quads, int32_t* payload, int32_t* count, void* stream) {
    int rc = mk_check_size("marker_detect", n, H, W);
    if (rc) return rc;
    if (c != 1 && c != 3 && c != 4) return sw_fail(SWNERF_E_ARG, "marker_detect: %d channels; 1, 3 and 4 are built", c);
    if (!radii || nradii < 1 || nradii > MARKER_MAX_RADII) return sw_fail(SWNERF_E_ARG, "marker_detect: 1..%d radii", MARKER_MAX_RADII);
    for (int i = 0; i < nradii; ++i) {
        if ((rc = mk_check_params("marker_detect", radii[i], C, min_area))) return rc;
        if (i && radii[i] <= radii[i - 1]) return sw_fail(SWNERF_E_ARG, "marker_detect: the radii must ascend");
    }
    if (K < 0) return sw_fail(SWNERF_E_ARG, "marker_detect: negative capacity %d", K);
    if (n == 0) return 0;
    if (!frames || !count || (K && (!quads || !payload))) return sw_fail(SWNERF_E_ARG, "marker_detect: NULL pointer");
    if (((uintptr_t)quads | (uintptr_t)payload | (uintptr_t)count) & 3) return sw_fail(SWNERF_E_ARG, "marker_detect: outputs must be 4-byte aligned");
    if ((rc = mk_check_ws("marker_detect", workspace))) return rc;
    const MkPlan P = mk_plan(workspace, n, H, W);
    hipStream_t st = (hipStream_t)stream;
    mk_run_grey(frames, n, H, W, c, P.grey, st);
    for (int ri = 0; ri < nradii; ++ri) {
        int32_t* ncand = P.ncand + (int64_t)ri * n;
        mk_run_threshold(P, P.grey, n, (int)H, (int)W, radii[ri], C, P.mask, st);
        mk_run_label(P.mask, n, (int)H, (int)W, P.labels, st);
        if ((rc = mk_run_components(P, P.labels, n, (int)H, (int)W, min_area, ncand, st))) return rc;
        hipLaunchKernelGGL(mk_refine_kernel, dim3(mk_blocks(P.cap, 1) > 1024 ? 1024 : mk_blocks(P.cap, 1), (unsigned)n), dim3(64), 0, st,
                           P.grey, (int)H, (int)W, ncand, (int)P.cap, P.cand, P.found + (int64_t)ri * n * P.cap);
    }
    hipLaunchKernelGGL(mk_merge_kernel, dim3((unsigned)n), dim3(MK_THREADS), 0, st, n, nradii, P.ncand, (int)P.cap, P.found, K, quads,
                       payload, count);
    return sw_check(hipGetLastError(), "marker_detect launch");
}
