// optim_kernels.hip - one Adam / AdamW step over a LIST of tensors for gfx950 (MI355X): every parameter of every net of a runner
// in as few launches as the kernel-argument block allows.  DESIGN.md 6j.
//
// The multi-tensor-apply scheme: the kernel's ONE argument is a descriptor passed by value - per tensor p, g, m, v, the element
// count and the tensor's own scalars, and a block -> (tensor, chunk) map.  Nothing is uploaded per step: autograd allocates the
// gradients anew every iteration, so a device-side pointer table would need a host -> device copy per step and a lifetime the
// kernel arguments do not have.  A list longer than the descriptor holds is cut into consecutive launches by adam_plan_next,
// the one planner (swnerf_adam_plan runs the same function without a device, for the tests).
//
// Arithmetic: fp32, the lines of torch's single-tensor Adam (torch/optim/adam.py _single_tensor_adam), each operation rounded
// (the unit is built with -ffp-contract=off; sqrtf and the divisions are correctly rounded):
//   g' = g * grad_scale                                (grad_scale = 1 multiplies by exactly 1.0)
//   decoupled (AdamW):  p = p * (1 - lr wd)            else, wd != 0 (L2):  g' = g' + wd p
//   m = m + (g' - m)(1 - b1)          v = b2 v + (1 - b2) g' g'
//   denom = sqrt(v) / sqrt(1 - b2^t) + eps             p = p + (-(lr / (1 - b1^t)) m) / denom
// 1 - lr wd, lr / (1 - b1^t) and sqrt(1 - b2^t) are formed on the host in double from the tensor's OWN step count t (torch
// advances `step` only for parameters that had a gradient) and rounded to float once, as torch's Python scalars are.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/swnerf.h"
#include "host_util.h"

#define SW_ADAM_THREADS 256
#define SW_ADAM_CHUNK_MULT_MAX 16            // a launch that one tensor fills alone may give a block up to 16 x SWNERF_ADAM_CHUNK elements

struct AdamTensor {
    float* p; const float* g; float* m; float* v;
    int64_t n, base;                             // elements | the element at which this launch's chunk 0 of the tensor begins
    float decay_mul, wd, neg_step, bc2_sqrt;     // 1 - lr wd (decoupled) | wd (L2, else 0) | -(lr / (1 - b1^t)) | sqrt(1 - b2^t)
    int vec, pad_;                               // all four pointers 16-byte aligned: 4 floats per thread and access
};

struct AdamLaunch {
    AdamTensor t[SWNERF_ADAM_MAX_TENSORS];
    uint16_t block_chunk[SWNERF_ADAM_MAX_BLOCKS];
    uint8_t block_tensor[SWNERF_ADAM_MAX_BLOCKS];
    int64_t chunk;                               // elements per block of this launch: a multiple of SWNERF_ADAM_CHUNK
    float omb1, b2, omb2, eps, grad_scale;       // 1 - b1 | b2 | 1 - b2
    int decoupled;
};
static_assert(sizeof(AdamLaunch) <= 4096 - 256, "the descriptor and the 256 bytes of implicit kernel arguments must fit the 4 KB argument block");
static_assert(SWNERF_ADAM_MAX_TENSORS <= 256 && SWNERF_ADAM_MAX_BLOCKS <= 65536, "block_tensor is a byte, block_chunk two");
static_assert(SWNERF_ADAM_CHUNK % (4 * SW_ADAM_THREADS) == 0, "a chunk is whole rounds of the vector path, and keeps 16-byte alignment");

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamTensor& T, const AdamLaunch& A) {
    g = g * A.grad_scale;
    if (A.decoupled) p = p * T.decay_mul;
    else if (T.wd != 0.f) g = g + T.wd * p;
    m = m + (g - m) * A.omb1;
    v = A.b2 * v + (A.omb2 * g) * g;
    const float denom = sqrtf(v) / T.bc2_sqrt + A.eps;
    p = p + (T.neg_step * m) / denom;
}

__global__ void __launch_bounds__(SW_ADAM_THREADS) adam_step_kernel(const AdamLaunch A) {
    const AdamTensor& T = A.t[A.block_tensor[blockIdx.x]];
    const int64_t lo = T.base + (int64_t)A.block_chunk[blockIdx.x] * A.chunk;
    const int64_t hi = (T.n - lo < A.chunk) ? T.n : lo + A.chunk;               // the tensor's last chunk is masked
    if (T.vec) {
        for (int64_t e = lo + 4 * (int64_t)threadIdx.x; e < hi; e += 4 * SW_ADAM_THREADS) {
            if (e + 4 <= hi) {
                float4 p = *reinterpret_cast<const float4*>(T.p + e), m = *reinterpret_cast<const float4*>(T.m + e);
                float4 v = *reinterpret_cast<const float4*>(T.v + e);
                const float4 g = *reinterpret_cast<const float4*>(T.g + e);
                adam_one(p.x, g.x, m.x, v.x, T, A); adam_one(p.y, g.y, m.y, v.y, T, A);
                adam_one(p.z, g.z, m.z, v.z, T, A); adam_one(p.w, g.w, m.w, v.w, T, A);
                *reinterpret_cast<float4*>(T.p + e) = p; *reinterpret_cast<float4*>(T.m + e) = m; *reinterpret_cast<float4*>(T.v + e) = v;
            } else {
                for (int64_t k = e; k < hi; ++k) {                               // the 1..3 floats behind the last whole quad
                    float p = T.p[k], m = T.m[k], v = T.v[k];
                    adam_one(p, T.g[k], m, v, T, A);
                    T.p[k] = p; T.m[k] = m; T.v[k] = v;
                }
            }
        }
    } else {
        for (int64_t e = lo + threadIdx.x; e < hi; e += SW_ADAM_THREADS) {
            float p = T.p[e], m = T.m[e], v = T.v[e];
            adam_one(p, T.g[e], m, v, T, A);
            T.p[e] = p; T.m[e] = m; T.v[e] = v;
        }
    }
}

// ---- the planner ------------------------------------------------------------------------------------------------------
// One launch: tensors first .. first + count - 1 of the list (count <= SWNERF_ADAM_MAX_TENSORS), each from element base[k] on, in
// blocks of `chunk` elements (<= SWNERF_ADAM_MAX_BLOCKS of them), in list order.  chunk is SWNERF_ADAM_CHUNK, except in a launch that
// the rest of ONE tensor fills alone: there it is the smallest multiple of SWNERF_ADAM_CHUNK (at most 16 of them) with which that
// rest fits the block cap, so a tensor of 2^26 floats takes 4 launches and not 52.  The cursor (tensor, element) goes from (0, 0)
// to (n_tensors, 0); a launch cut inside a tensor leaves the cursor there, always at a multiple of SWNERF_ADAM_CHUNK.
struct AdamCursor { int tensor; int64_t off; };

static inline int64_t adam_chunks(int64_t n, int64_t chunk) { return (n + chunk - 1) / chunk; }

// fills base / block_tensor / block_chunk (tensor indices relative to *first) and returns the number of blocks; 0 = the list is done
static int adam_plan_next(int n_tensors, const int64_t* n, AdamCursor* cur, int* first, int* count, int64_t* chunk, int64_t* base,
                          uint8_t* block_tensor, uint16_t* block_chunk) {
    while (cur->tensor < n_tensors && n[cur->tensor] == 0) cur->tensor++;       // (an empty tensor is never cut: off is 0 here)
    if (cur->tensor >= n_tensors) return 0;
    *first = cur->tensor;
    *chunk = SWNERF_ADAM_CHUNK;
    const int64_t rest = n[cur->tensor] - cur->off;
    if (adam_chunks(rest, SWNERF_ADAM_CHUNK) >= SWNERF_ADAM_MAX_BLOCKS) {       // this launch is this tensor's alone
        int64_t mult = adam_chunks(rest, (int64_t)SWNERF_ADAM_CHUNK * SWNERF_ADAM_MAX_BLOCKS);
        if (mult > SW_ADAM_CHUNK_MULT_MAX) mult = SW_ADAM_CHUNK_MULT_MAX;
        *chunk = mult * SWNERF_ADAM_CHUNK;
        int64_t blocks = adam_chunks(rest, *chunk);
        if (blocks > SWNERF_ADAM_MAX_BLOCKS) blocks = SWNERF_ADAM_MAX_BLOCKS;
        base[0] = cur->off;
        for (int64_t b = 0; b < blocks; ++b) { block_tensor[b] = 0; block_chunk[b] = (uint16_t)b; }
        *count = 1;
        cur->off += blocks * *chunk;
        if (cur->off >= n[cur->tensor]) { cur->tensor++; cur->off = 0; }
        return (int)blocks;
    }
    int blocks = 0;
    while (cur->tensor < n_tensors && cur->tensor - *first < SWNERF_ADAM_MAX_TENSORS && blocks < SWNERF_ADAM_MAX_BLOCKS) {
        const int k = cur->tensor - *first;
        int64_t take = adam_chunks(n[cur->tensor] - cur->off, SWNERF_ADAM_CHUNK);
        if (take > SWNERF_ADAM_MAX_BLOCKS - blocks) take = SWNERF_ADAM_MAX_BLOCKS - blocks;
        base[k] = cur->off;
        for (int64_t c = 0; c < take; ++c) { block_tensor[blocks] = (uint8_t)k; block_chunk[blocks++] = (uint16_t)c; }
        cur->off += take * SWNERF_ADAM_CHUNK;
        if (cur->off < n[cur->tensor]) { *count = k + 1; return blocks; }       // cut inside this tensor
        cur->tensor++; cur->off = 0;
    }
    *count = cur->tensor - *first;
    return blocks;
}

extern "C" void swnerf_adam_caps(int* max_tensors, int* max_blocks, int64_t* chunk, size_t* descriptor_bytes) {
    if (max_tensors) *max_tensors = SWNERF_ADAM_MAX_TENSORS;
    if (max_blocks) *max_blocks = SWNERF_ADAM_MAX_BLOCKS;
    if (chunk) *chunk = SWNERF_ADAM_CHUNK;
    if (descriptor_bytes) *descriptor_bytes = sizeof(AdamLaunch);
}

extern "C" int64_t swnerf_adam_plan(int n_tensors, const int64_t* n, int64_t capacity, int32_t* launch, int32_t* tensor, int64_t* start,
                                    int64_t* count) {
    if (n_tensors < 0 || capacity < 0) return sw_fail(SWNERF_E_ARG, "adam_plan: negative n_tensors or capacity");
    if (n_tensors > 0 && !n) return sw_fail(SWNERF_E_ARG, "adam_plan: NULL pointer");
    for (int i = 0; i < n_tensors; ++i)
        if (n[i] < 0 || n[i] > SWNERF_ADAM_MAX_ELEMS) return sw_fail(SWNERF_E_ARG, "adam_plan: tensor %d has %lld elements (0 .. 2^40)", i, (long long)n[i]);
    AdamCursor cur = {0, 0};
    uint8_t bt[SWNERF_ADAM_MAX_BLOCKS];
    uint16_t bc[SWNERF_ADAM_MAX_BLOCKS];
    int first, cnt;
    int64_t chunk, rows = 0, base[SWNERF_ADAM_MAX_TENSORS];
    for (int l = 0;; ++l) {
        const int blocks = adam_plan_next(n_tensors, n, &cur, &first, &cnt, &chunk, base, bt, bc);
        if (blocks == 0) return rows;
        for (int b = 0; b < blocks; ++b, ++rows) {
            if (rows >= capacity) continue;                                     // counted, not written: the caller sizes and calls again
            if (!launch || !tensor || !start || !count) return sw_fail(SWNERF_E_ARG, "adam_plan: NULL output with capacity > 0");
            const int64_t lo = base[bt[b]] + (int64_t)bc[b] * chunk, nn = n[first + bt[b]];
            launch[rows] = l; tensor[rows] = first + bt[b]; start[rows] = lo; count[rows] = (nn - lo < chunk) ? nn - lo : chunk;
        }
    }
}

extern "C" int swnerf_adam_step(int n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* n,
                                const double* step, const double* lr, const double* weight_decay, double beta1, double beta2, double eps,
                                int decoupled, float grad_scale, void* stream) {
    if (n_tensors < 0) return sw_fail(SWNERF_E_ARG, "adam_step: negative n_tensors");
    if (!(beta1 >= 0. && beta1 < 1.) || !(beta2 >= 0. && beta2 < 1.))
        return sw_fail(SWNERF_E_ARG, "adam_step: betas (%g, %g) outside [0, 1)", beta1, beta2);
    if (!(eps >= 0.) || !isfinite(eps)) return sw_fail(SWNERF_E_ARG, "adam_step: eps %g must be finite and >= 0", eps);
    if (!isfinite(grad_scale)) return sw_fail(SWNERF_E_ARG, "adam_step: grad_scale %g is not finite", (double)grad_scale);
    if (n_tensors == 0) return 0;
    if (!p || !g || !m || !v || !n || !step || !lr || !weight_decay) return sw_fail(SWNERF_E_ARG, "adam_step: NULL pointer");
    for (int i = 0; i < n_tensors; ++i) {
        if (n[i] < 0 || n[i] > SWNERF_ADAM_MAX_ELEMS)
            return sw_fail(SWNERF_E_ARG, "adam_step: tensor %d has %lld elements (0 .. 2^40)", i, (long long)n[i]);
        if (!(lr[i] >= 0.) || !isfinite(lr[i])) return sw_fail(SWNERF_E_ARG, "adam_step: tensor %d: lr %g must be finite and >= 0", i, lr[i]);
        if (!(weight_decay[i] >= 0.) || !isfinite(weight_decay[i]))
            return sw_fail(SWNERF_E_ARG, "adam_step: tensor %d: weight_decay %g must be finite and >= 0", i, weight_decay[i]);
        if (!(step[i] >= 1.) || !isfinite(step[i])) return sw_fail(SWNERF_E_ARG, "adam_step: tensor %d: step %g must be finite and >= 1", i, step[i]);
        if (n[i] > 0 && (!p[i] || !g[i] || !m[i] || !v[i])) return sw_fail(SWNERF_E_ARG, "adam_step: tensor %d: NULL pointer", i);
    }
    AdamLaunch A;
    A.omb1 = (float)(1. - beta1); A.b2 = (float)beta2; A.omb2 = (float)(1. - beta2); A.eps = (float)eps;
    A.grad_scale = grad_scale; A.decoupled = decoupled ? 1 : 0;
    AdamCursor cur = {0, 0};
    int first, count;
    int64_t base[SWNERF_ADAM_MAX_TENSORS];
    for (;;) {
        const int blocks = adam_plan_next(n_tensors, n, &cur, &first, &count, &A.chunk, base, A.block_tensor, A.block_chunk);
        if (blocks == 0) return 0;
        for (int k = 0; k < count; ++k) {
            const int i = first + k;
            AdamTensor& T = A.t[k];
            T.p = p[i]; T.g = g[i]; T.m = m[i]; T.v = v[i]; T.n = n[i]; T.base = base[k];
            T.decay_mul = (float)(1. - lr[i] * weight_decay[i]);
            T.wd = decoupled ? 0.f : (float)weight_decay[i];
            T.neg_step = (float)-(lr[i] / (1. - pow(beta1, step[i])));
            T.bc2_sqrt = (float)sqrt(1. - pow(beta2, step[i]));
            T.vec = ((((uintptr_t)p[i] | (uintptr_t)g[i] | (uintptr_t)m[i] | (uintptr_t)v[i]) & 15) == 0) ? 1 : 0;
            T.pad_ = 0;
        }
        hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)blocks), dim3(SW_ADAM_THREADS), 0, (hipStream_t)stream, A);
        const int rc = sw_check(hipGetLastError(), "adam_step launch");
        if (rc != 0) return rc;
    }
}
