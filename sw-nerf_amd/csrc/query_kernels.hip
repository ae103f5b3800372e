// query_kernels.hip - the grid query of the two time-conditioned nets at ONE frame time (mesh extraction of a dynamic scene:
// nerf/extract_mesh.py sample_grid :27-90 with d_nerf/run_dnerf.py run_network :46-83 / t_nerf/run_tnerf.py run_network :48-87
// in place of the static network_query_fn).  Inference translation unit: ring depth 8, like render_kernels.hip.
//
// D-NeRF (DirectTemporalNeRF.forward, model.py:138-151): one wave per 32 points, 4 waves per workgroup, as query_points_kernel.
// The frame time is a constant of the LAUNCH, so the gamma(t) columns of _time.0 are evaluated once per wave (time_bias_tile:
// the TIME segment of the stream) and the deformation net's layer 0 starts from that tile - the same sequence of additions as the
// in-line form of mlp_forward_kernel<true>, so dx and sigma carry the same bits as the op path.  Then gamma(x + dx), the
// canonical trunk and the density ONCE per point and only the view branch V times (the views loop of the blob's CANON part).
//
// T-NeRF: tnerf_query_kernel (tnerf_kernels.hip), next to the pass whose device functions it uses.
#include <hip/hip_runtime.h>
#include "../../include/swnerf.h"
#include "swnerf_common.h"
#include "mlp_core.h"
#include "host_util.h"
#include "mlp_kernels.h"

struct QueryTimeDev {
    const float* pts; int64_t M; const float* dirs; int64_t V; int shared;
    const float* w0; const float* b0; int nbias; int two_pass; const float* wvl;
    float ft;               // the launch's frame time, as the kernels read it (float32)
    int tb_off;             // floats: where the four waves' TIME tiles sit in the dynamic LDS (behind the fixed layout; two_pass only)
    float* out; float* dx;
};

__global__ void __launch_bounds__(256, 1) query_points_dnerf_kernel(QueryTimeDev P) {
    extern __shared__ __attribute__((aligned(16))) float lds_bias[];
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* lds_ring = lds_bias + SW_LDS_BIAS_FLOATS + wv * SW_LDS_RING_FLOATS;
    float* lds_emb = lds_ring + SW_RING * SW_STEP_FLOATS;
    float* lds_tb = lds_bias + P.tb_off + wv * SW_TB_LDS_FLOATS;
    const int64_t tile = (int64_t)blockIdx.x * 4 + wv;
    bias_to_lds(lds_bias, P.b0, P.nbias);
    if (tile * 32 >= P.M) return;
    const int64_t row = tile * 32 + j;
    const bool live = row < P.M;
    const int64_t rr = live ? row : P.M - 1;
    const float x0 = P.pts[rr * 3], x1 = P.pts[rr * 3 + 1], x2 = P.pts[rr * 3 + 2];
    f32x16 emb[2], in[8], out[8];
    float head[3];
    pe_pos(x0, x1, x2, h, emb);
    WStream ws;
    // directions vary per loop turn: skip the stream's per-ray DIR prefix (and its b_vf tiles), as mlp_forward_kernel does
    ws_start(ws, P.w0 + SW_STEPS_DIR * SW_STEP_FLOATS, lds_bias + SW_DIR_BIAS_TILES * SW_BIAS_TILE_FLOATS, lds_ring, lane);
    // the stream's TIME segment, once per wave: _time.0.bias + its gamma(t) columns (mlp_core.h)
    if (P.two_pass) time_bias_tile(P.ft, h, lds_tb, lane, ws);
    float ex = 0.f, ey = 0.f, ez = 0.f;                       // run_deform == 0: dx = 0 (model.py:143-145)
#pragma nounroll
    for (int pass = P.two_pass ? 0 : 1; pass < 2; ++pass) {
        trunk_pass<true, false, false, false, true>(emb, lds_emb, P.ft, pass == 0, h, in, out, head, ws, nullptr, nullptr, false, nullptr, nullptr, lds_tb);
        if (pass == 0) {
            ex = head[0]; ey = head[1]; ez = head[2];
            pe_pos(x0 + ex, x1 + ey, x2 + ez, h, emb);        // embed_fn(input_pts_orig + dx) (model.py:148-149)
        }
    }
    const float* hb_rgb = ws.bias - SW_BIAS_TILE_FLOATS;      // [b_alpha, b_r, b_g, b_b]
    const float* rgb_tiles = ws.bias;                         // rgb_linear.weight as bias-style tiles: re-read on every turn
    ws_restart(ws, P.wvl);
    float sr = 0.f, sg = 0.f, sb = 0.f;
    const int64_t nv = P.shared ? P.V : 1;
#pragma nounroll
    for (int64_t v = 0; v < nv; ++v) {
        const float* dp = P.dirs + (P.shared ? v : rr) * 3;
        f32x16 demb, hv[4];
        pe_dir(dp[0], dp[1], dp[2], h, demb);
        ws.bias = rgb_tiles;
        ws.base = reinterpret_cast<const char*>(P.wvl);
        canon_tail_rows(in, demb, hv, lds_bias + h * 16, ws);
        float c3[3];
        head_valu<3, 4>(hv, ws, c3);
        sr += c3[0] + hb_rgb[1]; sg += c3[1] + hb_rgb[2]; sb += c3[2] + hb_rgb[3];
    }
    if (live && h == 0) {
        const float inv = 1.f / (float)nv;
        f32x4 r4 = {sr * inv, sg * inv, sb * inv, head[0]};
        *reinterpret_cast<f32x4*>(P.out + row * 4) = r4;
        if (P.dx) { P.dx[row * 3 + 0] = ex; P.dx[row * 3 + 1] = ey; P.dx[row * 3 + 2] = ez; }
    }
}

int sw_tnerf_query_launch(const float* packed, const float* pts, int64_t M, const float* dirs, int64_t n_dirs, float ft,
                          float* out, hipStream_t st);                       // tnerf_kernels.hip

extern "C" int swnerf_query_points_time(int kind, const float* packed, const float* pts, int64_t M, const float* dirs, int64_t n_dirs,
                                        int shared_dirs, double frame_time, int run_deform, int L_pos, int L_dir, int L_time,
                                        float* out, float* dx_out, void* stream) {
    if (kind != SWNERF_NET_DNERF && kind != SWNERF_NET_TNERF)
        return sw_fail(SWNERF_E_ARG, "query_points_time: net kind %d has no frame time (SWNERF_NET_DNERF or SWNERF_NET_TNERF)", kind);
    if (M == 0 && packed) return 0;
    if (!packed || !pts || !dirs || !out || M < 0) return sw_fail(SWNERF_E_ARG, "query_points_time: NULL pointer or negative M");
    if (L_pos < 0 || L_pos > 10 || L_dir < 0 || L_dir > 4 || L_time < 0 || L_time > 10)
        return sw_fail(SWNERF_E_UNSUPP, "query_points_time: embedder bands (%d,%d,%d) exceed (10,4,10)", L_pos, L_dir, L_time);
    if (shared_dirs ? n_dirs < 1 : n_dirs != M)
        return sw_fail(SWNERF_E_ARG, "query_points_time: need %s directions, got %lld for %lld points", shared_dirs ? ">= 1 shared" : "one per point", (long long)n_dirs, (long long)M);
    hipStream_t st = (hipStream_t)stream;
    if (kind == SWNERF_NET_TNERF) {
        if (!shared_dirs) return sw_fail(SWNERF_E_UNSUPP, "query_points_time: the T-NeRF query takes shared directions only (its stream has no per-row direction columns)");
        if (dx_out) return sw_fail(SWNERF_E_ARG, "query_points_time: T-NeRF has no position_delta output");
        if (L_dir == 0) return sw_fail(SWNERF_E_UNSUPP, "query_points_time: T-NeRF needs view directions (L_dir >= 1; TNeRF.forward reads vdir)");
        return sw_tnerf_query_launch(packed, pts, M, dirs, n_dirs, (float)frame_time, out, st);
    }
    QueryTimeDev P;
    P.pts = pts; P.M = M; P.dirs = dirs; P.V = n_dirs; P.shared = shared_dirs ? 1 : 0; P.out = out; P.dx = dx_out;
    P.ft = (float)frame_time;
    int rc = stream_ptrs(kind, packed, run_deform, &P.w0, &P.b0, &P.nbias, &P.two_pass);
    if (rc) return rc;
    P.wvl = views_loop_ptr(kind, packed);
    size_t lds = SW_LDS_FIXED_FLOATS * sizeof(float);
    P.tb_off = (int)(lds / sizeof(float));
    if (P.two_pass) lds += 4 * SW_TB_LDS_FLOATS * sizeof(float);             // the four waves' TIME tiles, behind everything else
    const dim3 grid((unsigned)((M + 127) / 128)), block(256);
    hipLaunchKernelGGL(query_points_dnerf_kernel, grid, block, lds, st, P);
    return sw_check(hipGetLastError(), "query_points_time launch");
}
