// fit2d_cols_host_main.cpp - a stand-alone program around csrc/fit2d_cols.h: the slot map of the 2-D fitting encoder, printed for
// every band count the fused pass accepts.  One line per (L, lane half): "L h c0 c1 .. c47", c = sw_fit2d_col(slot, h, L).
#include <stdio.h>
#include "fit2d_cols.h"

int main() {
    for (int L = 0; L <= SW_F2_MAX_L; ++L)
        for (int h = 0; h < 2; ++h) {
            printf("%d %d", L, h);
            for (int a = 0; a < 48; ++a) printf(" %d", sw_fit2d_col(a, h, L));
            printf("\n");
        }
    return 0;
}
