// par_prims.h - the small parallel primitives that more than one unit needs (marching cubes, markers, the three mesh units), each
// written once: device-inline only, no state.  Wave size 64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// deterministic block-wide exclusive scan over NT threads (wave prefix by shuffles, then the wave totals in order); lds holds
// NT / 64 elements, *total = the sum.  Every thread must call it.
template <typename T, int NT>
__device__ __forceinline__ T block_exclusive_scan(T x, T* lds, T* total) {
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

// Lock-free union-find over L[x] = parent of x (a root is its own parent), in LDS or in global memory.
__device__ __forceinline__ int uf_find(const int* L, int x) {
    int l;
    while ((l = __atomic_load_n(L + x, __ATOMIC_RELAXED)) != x) x = l;
    return x;
}

// link the larger root to the smaller until both ends share one: the final root is the set's smallest index, whatever the schedule
__device__ __forceinline__ void uf_union(int* L, int a, int b) {
    for (;;) {
        a = uf_find(L, a);
        b = uf_find(L, b);
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

// one atomic per wave for a per-thread count, into a 64-bit counter or an int32 status / count word (every lane of the wave must
// call)
template <typename T>
__device__ __forceinline__ void wave_count(T* dst, unsigned long long x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d, 64);
    if ((threadIdx.x & 63) == 0 && x) atomicAdd(dst, (T)x);
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
