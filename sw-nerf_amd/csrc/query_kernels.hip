// query_kernels.hip - the grid query of the two time-conditioned nets at ONE frame time (mesh extraction of a dynamic scene:
// nerf/extract_mesh.py sample_grid :27-90 with d_nerf/run_dnerf.py run_network :46-83 / t_nerf/run_tnerf.py run_network :48-87
// in place of the static network_query_fn).  Inference translation unit: ring depth 8, like render_kernels.hip.
//
// D-NeRF (DirectTemporalNeRF.forward, model.py:138-151): one wave per 32 points, 4 waves per workgroup, as query_points_kernel.
// The frame time is a constant of the LAUNCH, so the gamma(t) columns of _time.0 are evaluated once per wave (ray_init_tile:
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
    RowTile rt;
    if (!row_tile(rt, lds_bias, P.b0, P.nbias, P.M)) return;
    const int h = rt.h;
    float* lds_tb = lds_bias + P.tb_off + rt.wv * SW_TB_LDS_FLOATS;
    const float x0 = P.pts[rt.rr * 3], x1 = P.pts[rt.rr * 3 + 1], x2 = P.pts[rt.rr * 3 + 2];
    f32x16 emb[2], in[8], out[8];
    float head[3];
    pe_pos(x0, x1, x2, h, emb);
    WStream ws;
    // directions vary per loop turn: skip the stream's per-ray DIR prefix (and its b_vf tiles), as mlp_forward_kernel does
    ws_start(ws, P.w0 + SW_STEPS_DIR * SW_STEP_FLOATS, lds_bias + SW_DIR_BIAS_TILES * SW_BIAS_TILE_FLOATS, rt.lds_ring, rt.lane);
    // the stream's TIME segment, once per wave: _time.0.bias + its gamma(t) columns (mlp_core.h)
    if (P.two_pass) {
        f32x16 temb;
        pe_time(P.ft, h, temb);
        ray_init_tile<8>(temb, lds_tb, rt.lane, ws);
    }
    float ex = 0.f, ey = 0.f, ez = 0.f;                       // run_deform == 0: dx = 0 (model.py:143-145)
#pragma nounroll
    for (int pass = P.two_pass ? 0 : 1; pass < 2; ++pass) {
        trunk_pass<true, false, false, false, true>(emb, rt.lds_emb, P.ft, pass == 0, h, in, out, head, ws, TrunkSide{}, lds_tb);
        if (pass == 0) {
            ex = head[0]; ey = head[1]; ez = head[2];
            pe_pos(x0 + ex, x1 + ey, x2 + ez, h, emb);        // embed_fn(input_pts_orig + dx) (model.py:148-149)
        }
    }
    float rgb[3];
    views_mean(in, ws, P.wvl, P.dirs, P.V, P.shared, rt.rr, h, lds_bias, rgb);
    if (rt.live && h == 0) {
        f32x4 r4 = {rgb[0], rgb[1], rgb[2], head[0]};
        *reinterpret_cast<f32x4*>(P.out + rt.row * 4) = r4;
        if (P.dx) { P.dx[rt.row * 3 + 0] = ex; P.dx[rt.row * 3 + 1] = ey; P.dx[rt.row * 3 + 2] = ez; }
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
    if (int rc = sw_check_bands("query_points_time", 3, L_pos, L_dir, L_time)) return rc;
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
    return sw_launch_rows(query_points_dnerf_kernel, P, M, lds, st, "query_points_time launch");
}
