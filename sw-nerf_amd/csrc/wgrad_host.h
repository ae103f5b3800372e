// wgrad_host.h - host arithmetic shared by every weight-gradient launch of wgrad_kernels.hip and wgrad_x3_kernels.hip.  No device code and no HIP header:
// plain C / C++, so that a host compiler alone can test it (tests/test_cabi_and_host.py).
#pragma once
#include <stdbool.h>
#include <stdint.h>
#include "../../include/swnerf.h"

// M rows over about `target_wgs` workgroups, each a whole number of `slab`-row slabs (only a slice's LAST slab may be partial):
// rows_per_wg % slab == 0, (nwg - 1) * rows_per_wg < M <= nwg * rows_per_wg, nwg <= max(target_wgs, 1).
typedef struct RowSplit { int64_t rows_per_wg; int64_t nwg; } RowSplit;
static inline RowSplit split_rows(int64_t M, int64_t target_wgs, int slab) {
    RowSplit s;
    if (target_wgs < 1) target_wgs = 1;
    s.rows_per_wg = ((M + target_wgs - 1) / target_wgs + slab - 1) / slab * slab;
    s.nwg = (M + s.rows_per_wg - 1) / s.rows_per_wg;
    return s;
}

// A kernel that adds row offsets to its slice's base as the unsigned 32-bit byte offset of a global load: the slice's rows of the
// widest operand must stay below 4 GiB.  gemm_tn_kernel needs exactly this; narrow5_kernel and narrow_plan_kernel advance 64-bit
// bases per slab and form 32-bit offsets within one 16-row slab only, so for them the bound is conservative by construction.
static inline bool fits_u32_offsets(int64_t rows_per_wg, int64_t max_ld) { return rows_per_wg * max_ld < ((int64_t)1 << 30); }

// An operand that 16-byte LDS-DMA can stage: every row starts on a 16-byte boundary.
static inline bool dma_aligned(const void* p, int ld) { return (uintptr_t)p % 16 == 0 && ld % 4 == 0; }

// A "fused item" (swnerf_gemm_item: one 256 x 256 GEMM with its optional riders), checked the same way by every entry point that
// takes one: the name of the operand group that is wrong, or NULL.
static inline const char* fused_item_bad(const swnerf_gemm_item* q) {
    if (!q->A || !q->B || !q->C || q->lda < 256 || q->ldb < 256 || q->ldc < 256) return "main operands";
    if (q->B2 && (!q->C2 || q->Ni2 < 1 || q->Ni2 > 64 || q->ldb2 < q->Ni2 || q->ldc2 < q->Ni2)) return "B2 rider";
    if (q->A2 && (!q->C3 || q->No2 < 1 || q->No2 > 32 || q->lda2 < q->No2 || q->ldc3 < 256)) return "A2 rider";
    return 0;
}
// the double-buffered LDS-DMA kernels (fp32 and bf16x3) take the item's main GEMM; otherwise it is separate swnerf_gemm_tn calls
static inline bool fused_item_takes_dma(const swnerf_gemm_item* q, int64_t M) { return dma_aligned(q->A, q->lda) && dma_aligned(q->B, q->ldb) && M >= 4096; }
