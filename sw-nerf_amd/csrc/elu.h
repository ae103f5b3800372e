// elu.h - ELU (alpha = 1) on the device: x > 0 ? x : expm1(x), shared by the fused T-NeRF pass (tnerf_kernels.hip) and the
// generic GEMM epilogue (generic_kernels.hip), so that both paths produce the same bits.
//
// torch's CPU ELU evaluates expm1 (nearly correctly rounded); exp(x) - 1 loses everything near 0.  Here:
//   -0.5 <= x <= 0: the degree-8 Taylor polynomial of expm1 (truncation < 6e-9), Horner with explicit FMAs;
//   x < -0.5:       v_exp_f32(x log2 e) - 1.  exp(x) < 0.61, so the subtraction is exact down to x = -ln 2 (Sterbenz) and
//                   rounds by at most 3e-8 below; the rounding of x log2 e costs < 3e-8 absolute at any x.
// Max abs error against expm1 over [-20, 0]: <= 1.2e-7 (tests/test_gpu_tnerf.py pins it).  Branch free: ~14 VALU ops.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float sw_expm1_neg(float x) {      // x <= 0
    float p = fmaf(x, 2.48015873e-5f, 1.98412698e-4f);        // 1/8!, 1/7!
    p = fmaf(p, x, 1.38888889e-3f);                           // 1/6!
    p = fmaf(p, x, 8.33333333e-3f);                           // 1/5!
    p = fmaf(p, x, 4.16666667e-2f);                           // 1/4!
    p = fmaf(p, x, 1.66666667e-1f);                           // 1/3!
    p = fmaf(p, x, 0.5f);
    p = fmaf(p, x * x, x);                                    // x + x^2 (1/2 + x/6 + ...)
    const float e = __builtin_amdgcn_exp2f(x * 1.44269504088896341f) - 1.f;
    return x >= -0.5f ? p : e;
}

__device__ __forceinline__ float sw_elu(float x) {
    const float m = sw_expm1_neg(fminf(x, 0.f));
    return (x > 0.f || x != x) ? x : m;                     // NaN stays NaN, like torch
}
