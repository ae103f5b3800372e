// host_util.h - error reporting, the embedder-band check and the per-row launch shared by the extern "C" entry points.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/swnerf.h"
#include <stdarg.h>
#include <stdio.h>

char* sw_errbuf();                       // thread-local message buffer (capi.hip)
#define SW_ERRBUF_LEN 512

static inline int sw_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(sw_errbuf(), SW_ERRBUF_LEN, fmt, ap);
    va_end(ap);
    return code;
}

static inline int sw_check(hipError_t e, const char* what) {
    if (e == hipSuccess) return 0;
    snprintf(sw_errbuf(), SW_ERRBUF_LEN, "%s: %s", what, hipGetErrorString(e));
    return (int)e;
}

// The embedder bands the kernels are built for: positions and time 0..10, directions 0..4.  n: how many embedders the entry
// point has (1 positions, 2 + directions, 3 + time); the message lists exactly those.
static inline int sw_check_bands(const char* name, int n, int L_pos, int L_dir = 0, int L_time = 0) {
    if (L_pos >= 0 && L_pos <= 10 && L_dir >= 0 && L_dir <= 4 && L_time >= 0 && L_time <= 10) return 0;
    if (n == 3) return sw_fail(SWNERF_E_UNSUPP, "%s: embedder bands (%d,%d,%d) exceed (10,4,10)", name, L_pos, L_dir, L_time);
    if (n == 2) return sw_fail(SWNERF_E_UNSUPP, "%s: embedder bands (%d,%d) exceed (10,4)", name, L_pos, L_dir);
    return sw_fail(SWNERF_E_UNSUPP, "%s: %d position bands exceed 10", name, L_pos);
}

// Launch of a per-row kernel: one wave per 32 rows, four waves per workgroup; `what` names the launch in the error text.
template <typename Kernel, typename Dev>
static inline int sw_launch_rows(Kernel kernel, const Dev& P, int64_t M, size_t lds_bytes, void* stream, const char* what) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((M + 127) / 128)), dim3(256), lds_bytes, (hipStream_t)stream, P);
    return sw_check(hipGetLastError(), what);
}
