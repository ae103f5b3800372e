// meshlayout_host_main.cpp - the workspace layouts of csrc/meshops_layout.h on the host: every layout is carved from a heap block of
// exactly the size that the same carving reports from a null base, so AddressSanitizer sees a size that is too small.  Checked for
// each: every array starts on a multiple of 256 bytes (the table minima: right behind the keys), the arrays follow one another in
// the written order without overlap, the last one ends inside the block, the spans that the library clears with one memset are
// what lies between the two pointers it uses, and the first and the last element of every array can be written.
// tests/test_meshlayout_host.py builds and runs it.
//   meshlayout_host_main        prints one line per layout: name V F bytes
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "meshops_layout.h"

struct Arr {
    const char* name;
    void* p;
    int64_t count, elem;               // elements in use, bytes per element
    bool aligned;                      // starts on a multiple of 256 bytes
};

static int failures = 0;

#define EXPECT(cond, ...)                                   \
    do {                                                    \
        if (!(cond)) {                                      \
            fprintf(stderr, "%s V = %lld F = %lld: ", layout, (long long)V, (long long)F); \
            fprintf(stderr, __VA_ARGS__);                   \
            fprintf(stderr, "\n");                          \
            ++failures;                                     \
        }                                                   \
    } while (0)

static void check(const char* layout, int64_t V, int64_t F, char* base, int64_t total, int64_t carved, const Arr* a, int n) {
    EXPECT(carved == total, "carving from the block gives %lld bytes, from a null base %lld", (long long)carved, (long long)total);
    EXPECT(total % 256 == 0, "total %lld is no multiple of 256", (long long)total);
    char* end = base;
    for (int i = 0; i < n; ++i) {
        char* p = (char*)a[i].p;
        const int64_t bytes = a[i].count * a[i].elem;
        EXPECT(p >= end, "%s starts %lld bytes before the end of %s", a[i].name, (long long)(end - p), i ? a[i - 1].name : "the base");
        EXPECT(!a[i].aligned || (p - base) % 256 == 0, "%s starts at offset %lld", a[i].name, (long long)(p - base));
        EXPECT(((uintptr_t)p) % a[i].elem == 0, "%s is not aligned to its element", a[i].name);
        EXPECT(p + bytes <= base + total, "%s ends %lld bytes past the block", a[i].name, (long long)(p + bytes - (base + total)));
        if (p >= base && p + bytes <= base + total && bytes > 0) {
            memset(p, 0xA5, a[i].elem);                            // first and last element
            memset(p + bytes - a[i].elem, 0x5A, a[i].elem);
        }
        end = p + bytes;
    }
    printf("%s %lld %lld %lld\n", layout, (long long)V, (long long)F, (long long)total);
}

// the span [from, to) that one memset clears holds exactly the arrays a[lo .. hi)
static void check_span(const char* layout, int64_t V, int64_t F, const Arr* a, int lo, int hi, void* from, void* to) {
    EXPECT(from == a[lo].p && to == a[hi].p, "the span does not run from %s to %s", a[lo].name, a[hi].name);
    const int64_t span = (char*)to - (char*)from;
    EXPECT(span >= 0, "negative span");
    if (span >= 0) memset(from, 0, (size_t)span);                  // what the library does; past the block: AddressSanitizer
}

static void mesh(int64_t V, int64_t F) {
    const char* layout = "mesh";
    int64_t total = 0, carved = 0;
    mo_ws(nullptr, V, F, &total);
    char* base = (char*)malloc((size_t)total);
    const MoWs w = mo_ws(base, V, F, &carved);
    const Arr a[] = {{"a0", w.a0, V + 1, 4, true}, {"a1", w.a1, V + 1, 4, true}, {"a2", w.a2, V + 1, 4, true}, {"b0", w.b0, F + 1, 4, true},
                     {"tsum", w.tsum, mo_tiles((V > F ? V : F) + 1), 4, true}, {"status", w.status, 1, 4, true}, {"bbox", w.bbox, 6, 4, false},
                     {"cnt", w.cnt, 8, 8, false}, {"part", w.part, MO_PARTS * MESHOPS_FACE_TERMS, 8, true}};
    check(layout, V, F, base, total, carved, a, 9);
    check_span(layout, V, F, a, 0, 3, w.a0, w.b0);                 // mesh_components
    EXPECT((char*)w.part - (char*)w.status == 512, "the status block is not 512 bytes");
    free(base);
}

static void simplify(int64_t V, int64_t F) {
    const char* layout = "simplify";
    int64_t total = 0, carved = 0;
    ms_ws(nullptr, V, F, &total);
    char* base = (char*)malloc((size_t)total);
    const MsWs w = ms_ws(base, V, F, &carved);
    EXPECT(w.cap >= MS_MIN_CAPACITY && w.cap >= 2 * V && (w.cap & (w.cap - 1)) == 0, "cap = %lld", (long long)w.cap);
    const Arr a[] = {{"tkey", w.tkey, w.cap, 8, true}, {"tmin", w.tmin, w.cap, 4, false}, {"slot", w.slot, V + 1, 4, true}, {"cnt", w.cnt, V + 1, 4, true},
                     {"off", w.off, V + 1, 4, true}, {"moff", w.moff, V + 1, 4, true}, {"mitems", w.mitems, V + 1, 4, true}, {"gl", w.gl, 3 * F + 1, 4, true},
                     {"items", w.items, 3 * F + 1, 4, true}, {"fflag", w.fflag, F + 1, 4, true}, {"tsum", w.tsum, mo_tiles((V > F ? V : F) + 1), 4, true},
                     {"status", w.status, 16, 4, true}, {"okey", w.okey, 3, 4, false}, {"origin", w.origin, 3, 4, false}};
    check(layout, V, F, base, total, carved, a, 14);
    EXPECT((char*)w.tmin == (char*)w.tkey + 8 * w.cap, "the minima do not start at 8 cap");
    EXPECT((char*)w.slot == (char*)w.tmin + 4 * w.cap, "the slots do not start at 12 cap");
    check_span(layout, V, F, a, 0, 2, w.tkey, w.slot);             // mesh_cluster
    EXPECT(base + total - (char*)w.status == 512, "the status block is not 512 bytes");
    free(base);
}

static void fill_boundary(int64_t V, int64_t F) {
    const char* layout = "fill_boundary";
    int64_t total = 0, carved = 0;
    mf_boundary_ws(nullptr, V, F, &total);
    char* base = (char*)malloc((size_t)total);
    const MfBoundaryWs w = mf_boundary_ws(base, V, F, &carved);
    const Arr a[] = {{"flag", w.flag, 3 * F + 2, 4, true}, {"nout", w.nout, V + 1, 4, true}, {"nin", w.nin, V + 1, 4, true}, {"leave", w.leave, V + 1, 4, true},
                     {"cnt", w.cnt, V + 1, 4, true}, {"off", w.off, V + 1, 4, true}, {"items", w.items, 3 * F + 2, 4, true},
                     {"tsum", w.tsum, mf_tsum_len(V, F), 4, true}};
    check(layout, V, F, base, total, carved, a, 8);
    check_span(layout, V, F, a, 1, 3, w.nout, w.leave);            // mesh_boundary
    free(base);
}

static void fill_loops(int64_t V, int64_t F) {
    const char* layout = "fill_loops";
    int64_t total = 0, carved = 0;
    mf_loops_ws(nullptr, V, F, &total);
    char* base = (char*)malloc((size_t)total);
    const MfLoopsWs w = mf_loops_ws(base, V, F, &carved);
    const Arr a[] = {{"a", w.a, 3 * F + 1, 8, true}, {"b", w.b, 3 * F + 1, 8, true}, {"leader", w.leader, 3 * F + 2, 4, true}, {"s2", w.s2, 3 * F + 2, 4, true},
                     {"s3", w.s3, 3 * F + 2, 4, true}, {"tsum", w.tsum, mf_tsum_len(V, F), 4, true}};
    check(layout, V, F, base, total, carved, a, 6);
    free(base);
}

int main() {
    static const int64_t sizes[][2] = {{1, 1}, {3, 1}, {257, 85}, {360, 716}};
    for (const auto& s : sizes) {
        mesh(s[0], s[1]);
        simplify(s[0], s[1]);
        fill_boundary(s[0], s[1]);
        fill_loops(s[0], s[1]);
    }
    simplify(360, 0);                                              // mesh_cluster: the table and the slots
    if (failures) fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}
