// fit2d_cols.h - the column scatter of the 2-D fitting encoder (fit2d_kernels.hip), in a header of its own so that the host can
// print and check the map (tests/fit2d_cols_host_main.cpp).
#pragma once
#ifndef __HIPCC__
#define __host__
#define __device__
#endif

// Lane half h = 0 holds the x coordinate's terms, h = 1 the y coordinate's: both halves run one instruction stream.
// B-operand slot a = 0..47 (k-tile a >> 4, register a & 15) of half h carries encoding column sw_fit2d_col(a, h, L).
#define SW_F2_MAX_L 23                     // 2 * 23 + 1 slots per half fit three 16-register k-tiles
static inline __host__ __device__ int sw_fit2d_col(int a, int h, int L) {
    if (a < 2 * SW_F2_MAX_L) { const int i = a >> 1, s = a & 1; return i < L ? 2 + 4 * i + 2 * s + h : -1; }
    if (a == 2 * SW_F2_MAX_L) return h;
    return -1;
}
