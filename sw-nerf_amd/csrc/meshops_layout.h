// meshops_layout.h - the workspace layouts of the three mesh units (meshops_kernels.hip, meshsimp_kernels.hip, meshfill_kernels.hip),
// each written once as a function of (V, F): a bump arena carves the arrays in order, and the same carving from a null base gives
// the byte total that the swnerf_mesh_*workspace_bytes functions report.  Plain C++: g++ compiles this header without HIP
// (tests/meshlayout_host_main.cpp carves every layout from a heap block of exactly the reported size under AddressSanitizer).
#pragma once
#include <stdint.h>
#include "meshops_math.h"

#define MO_THREADS 256
#define MO_PARTS 256                   // workgroups (= partial sums) of the fp64 face reduction
#define MS_MIN_CAPACITY 64

static inline int64_t mo_round256(int64_t b) { return (b + 255) & ~(int64_t)255; }
static inline int64_t mo_tiles(int64_t n) { return (n + MO_THREADS - 1) / MO_THREADS; }
static inline bool mo_sizes_ok(int64_t V, int64_t F) { return V >= 0 && V <= INT32_MAX && F >= 0 && F <= INT32_MAX / 3; }   // 3 F < 2^31

// Every array starts on a multiple of 256 bytes.  Addresses are integers until an array is handed out, so a null base is as good as
// any other: `off` is then the size of the layout.
struct MoArena {
    uintptr_t base;
    int64_t off;
    template <typename T>
    T* take(int64_t count) {
        T* p = (T*)(base + (uintptr_t)off);
        off += mo_round256((int64_t)sizeof(T) * count);
        return p;
    }
};

template <typename T>
static inline T* mo_at(void* p, int64_t bytes) { return (T*)((uintptr_t)p + (uintptr_t)bytes); }

// clean-up and measurement: three int32 [V+1] | one int32 [F+1] | tile sums int32 [tiles(max(V, F) + 1)] | 64 x 8 bytes of status
// and counters | fp64 partials [MO_PARTS, 5]
struct MoWs {
    int32_t *a0, *a1, *a2, *b0, *tsum;
    int32_t* status;                   // [0] bad indices of this call
    uint32_t* bbox;                    // [6] ordered keys: min xyz, max xyz (bytes 64..)
    unsigned long long* cnt;           // [8] integer counters (bytes 128..)
    double* part;
};

static inline MoWs mo_ws(void* ws, int64_t V, int64_t F, int64_t* bytes = nullptr) {
    MoArena a{(uintptr_t)ws, 0};
    MoWs w;
    w.a0 = a.take<int32_t>(V + 1);     // a0 | a1 | a2: one span (mesh_components clears it at once)
    w.a1 = a.take<int32_t>(V + 1);
    w.a2 = a.take<int32_t>(V + 1);
    w.b0 = a.take<int32_t>(F + 1);
    w.tsum = a.take<int32_t>(mo_tiles((V > F ? V : F) + 1));
    char* s = a.take<char>(512);
    w.status = (int32_t*)s;
    w.bbox = mo_at<uint32_t>(s, 64);
    w.cnt = mo_at<unsigned long long>(s, 128);
    w.part = a.take<double>(MO_PARTS * MESHOPS_FACE_TERMS);
    if (bytes) *bytes = a.off;
    return w;
}

// welding and decimation: table keys uint64 [cap] | table minima uint32 [cap] | five int32 [V+1] | two int32 [3F+1] | face flags
// int32 [F+1] | tile sums | 512 bytes of status, origin keys and origin.  mesh_cluster uses the layout of (V, 0): the table and the
// slots.
struct MsWs {
    unsigned long long* tkey;
    uint32_t *tmin, *slot;
    int32_t *cnt, *off, *moff, *mitems, *gl, *items, *fflag, *tsum;
    int32_t* status;                   // [0] bad face indices, [1] invalid vertices, [2] table overflow
    uint32_t* okey;                    // [3] ordered keys of the per-axis minimum (bytes 64..)
    float* origin;                     // [3] the origin in use (bytes 128..)
    int64_t cap;
};

static inline int64_t ms_capacity(int64_t V) {
    int64_t c = MS_MIN_CAPACITY;
    while (c < 2 * V) c <<= 1;
    return c;
}

static inline MsWs ms_ws(void* ws, int64_t V, int64_t F, int64_t* bytes = nullptr) {
    MoArena a{(uintptr_t)ws, 0};
    MsWs w;
    // cap is a power of two >= 64: 8 cap and 4 cap are multiples of 256, so tkey | tmin is one span of 12 cap bytes with no padding
    // (mesh_cluster fills it at once)
    w.cap = ms_capacity(V);
    w.tkey = a.take<unsigned long long>(w.cap);
    w.tmin = a.take<uint32_t>(w.cap);
    w.slot = a.take<uint32_t>(V + 1);
    w.cnt = a.take<int32_t>(V + 1);
    w.off = a.take<int32_t>(V + 1);
    w.moff = a.take<int32_t>(V + 1);
    w.mitems = a.take<int32_t>(V + 1);
    w.gl = a.take<int32_t>(3 * F + 1);
    w.items = a.take<int32_t>(3 * F + 1);
    w.fflag = a.take<int32_t>(F + 1);
    w.tsum = a.take<int32_t>(mo_tiles((V > F ? V : F) + 1));
    char* s = a.take<char>(512);
    w.status = (int32_t*)s;
    w.okey = mo_at<uint32_t>(s, 64);
    w.origin = mo_at<float>(s, 128);
    if (bytes) *bytes = a.off;
    return w;
}

// hole filling, the boundary phase: flags int32 [3F+2] | five int32 [V+1] | corner items int32 [3F+2] | tile sums
struct MfBoundaryWs { int32_t *flag, *nout, *nin, *leave, *cnt, *off, *items, *tsum; };

static inline int64_t mf_tsum_len(int64_t V, int64_t F) { return mo_tiles((3 * F > V ? 3 * F : V) + 2); }

static inline MfBoundaryWs mf_boundary_ws(void* ws, int64_t V, int64_t F, int64_t* bytes = nullptr) {
    MoArena a{(uintptr_t)ws, 0};
    MfBoundaryWs w;
    w.flag = a.take<int32_t>(3 * F + 2);
    w.nout = a.take<int32_t>(V + 1);   // nout | nin: one span (mesh_boundary clears it at once)
    w.nin = a.take<int32_t>(V + 1);
    w.leave = a.take<int32_t>(V + 1);
    w.cnt = a.take<int32_t>(V + 1);
    w.off = a.take<int32_t>(V + 1);
    w.items = a.take<int32_t>(3 * F + 2);
    w.tsum = a.take<int32_t>(mf_tsum_len(V, F));
    if (bytes) *bytes = a.off;
    return w;
}

// hole filling, the loop phase: two buffers of (int32, int32) pairs [3F+1] (typed as 8-byte elements here, int2 on the device) |
// three int32 [3F+2] | tile sums
struct MfLoopsWs { int64_t *a, *b; int32_t *leader, *s2, *s3, *tsum; };

static inline MfLoopsWs mf_loops_ws(void* ws, int64_t V, int64_t F, int64_t* bytes = nullptr) {
    MoArena a{(uintptr_t)ws, 0};
    MfLoopsWs w;
    w.a = a.take<int64_t>(3 * F + 1);
    w.b = a.take<int64_t>(3 * F + 1);
    w.leader = a.take<int32_t>(3 * F + 2);
    w.s2 = a.take<int32_t>(3 * F + 2);
    w.s3 = a.take<int32_t>(3 * F + 2);
    w.tsum = a.take<int32_t>(mf_tsum_len(V, F));
    if (bytes) *bytes = a.off;
    return w;
}

// hole filling, the emit phase: fp64 run sums [2, slots, 3] of positions and colours
static inline int64_t mf_slots(int64_t M, int64_t L) { return M / MESHOPS_FILL_RUN + L + 2; }
static inline int64_t mf_emit_bytes(int64_t F) { return mo_round256(8 * 6 * mf_slots(3 * F, F)); }
