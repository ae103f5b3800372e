// meshops_common.h - what the three mesh units share on the host and in their kernels: the launch geometry, the size check, the
// "kept" test of a scanned flag array, the copy of a vertex row, and the two multi-launch helpers (scan, CSR) whose kernels live in
// meshops_kernels.hip alone.  The workspace layouts are in meshops_layout.h, the device primitives in par_prims.h.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/swnerf.h"
#include "host_util.h"
#include "meshops_math.h"
#include "meshops_layout.h"
#include "par_prims.h"

#define MO_MAX_GRID 1024               // grid-stride cap
#define MO_SCAN_THREADS 1024
#define MO_KEY_POS_INF 0xFF800000u     // meshops_float_key of +inf and of -inf: the empty bounding box
#define MO_KEY_NEG_INF 0x007FFFFFu
#define MO_SORT_SMALL 16               // slices up to this length are sorted by insertion, longer ones by heap sort

static inline unsigned mo_blocks(int64_t n) {
    const int64_t t = mo_tiles(n);
    return (unsigned)(t < 1 ? 1 : (t < MO_MAX_GRID ? t : MO_MAX_GRID));
}

static inline int mo_check(const char* what, int64_t V, int64_t F) {
    if (!mo_sizes_ok(V, F))
        return sw_fail(SWNERF_E_ARG, "%s: V = %lld, F = %lld: need 0 <= V < 2^31 and 0 <= 3 F < 2^31 (corner ids are int32)", what, (long long)V, (long long)F);
    return 0;
}

// scan = the exclusive scan of a flag array with one more element at its end: element i is kept iff its scan value differs from the
// next one's, and then scan[i] is its place in the output - used only when it is inside an output of n_out elements
__device__ __forceinline__ bool mo_kept(const int32_t* scan, int64_t i, int64_t n_out) {
    return scan[i + 1] != scan[i] && meshops_index_ok(scan[i], n_out);
}

// row i of a vertex table to row o of the output: the position, and the normal and the colour where the input has them
__device__ __forceinline__ void mo_copy_row(const float* verts, const float* normals, const float* colors, int64_t i, float* verts_out, float* normals_out,
                                            float* colors_out, int64_t o) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        verts_out[3 * o + k] = verts[3 * i + k];
        if (normals) normals_out[3 * o + k] = normals[3 * i + k];
        if (colors) colors_out[3 * o + k] = colors[3 * i + k];
    }
}

// The library is linked without relocatable device code: a kernel is launched only from the unit that defines it, so the other
// units reach the scan and the CSR kernels through these two host functions (hidden: the library exports the swnerf_* names).

// off[i] = sum of cnt[0 .. i) for i < n (off may be cnt); *total (may be NULL) = the sum of all n.  Three launches.
__attribute__((visibility("hidden"))) int mo_scan(const int32_t* cnt, int32_t* off, int64_t n, int32_t* tsum, int32_t* total, hipStream_t st);

// CSR of the values key[0 .. n) per value: offsets [V+1], items ascending when `sorted` (else in the order the atomics landed, for
// a reader that does not care).  memset | valence | scan | memset | fill | sort: a value outside 0..V-1 is counted into
// *out_of_range, and the fill and the sort return at once when *bad is set.  cnt: int32 [V+1] of scratch.
__attribute__((visibility("hidden"))) int mo_csr(const int32_t* key, int64_t V, int64_t n, int32_t* cnt, int32_t* offsets, int32_t* items, int32_t* tsum,
                                                 int32_t* out_of_range, int32_t* bad, bool sorted, hipStream_t st);
