// bf16x3_split.h - the operand split of the "bf16x3" arithmetic, shared by the inference MLP (mlp_core_x3.h) and the
// weight-gradient GEMM (wgrad_x3_kernels.hip): v = hi + lo with hi = bf16(v), lo = bf16(v - hi), both round to nearest even
// (16 significant bits together); a product a.b is then a_hi.b_hi + a_hi.b_lo + a_lo.b_hi with fp32 accumulation.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned x3_cvt_pk(float a, float b) {       // [bf16(a) | bf16(b) << 16], round to nearest even
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// two fp32 values -> their packed hi halves and packed lo halves (a in the low 16 bits, as the MFMA's element order wants)
__device__ __forceinline__ void x3_split_pair(float a, float b, unsigned& hi, unsigned& lo) {
    hi = x3_cvt_pk(a, b);
    lo = x3_cvt_pk(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u));
}
