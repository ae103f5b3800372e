// render_kernels.hip - the inference translation unit (ring depth 8): the entry points of the fused render pass (render_pass.h
// describes the pass), the point query, coarse sampling and model.forward on embedded rows.
#include <hip/hip_runtime.h>
#include "../../include/swnerf.h"
#include "swnerf_common.h"
#include "mlp_core.h"
#include "host_util.h"
#include "mlp_kernels.h"

#include "render_pass.h"

// ------------------------------------------------------------------------------------------
// network_query_fn on bare points (nerf/load_model.py:56-74) with V view directions per point
// (nerf/extract_mesh.py:27-90): trunk + density once, view branch V times.
struct QueryDev {
    const float* pts; int64_t M; const float* dirs; int64_t V; int shared;
    const float* w0; const float* b0; int nbias; const float* wvl; float* out;
};

__global__ void __launch_bounds__(256, 1) query_points_kernel(QueryDev P) {
    extern __shared__ __attribute__((aligned(16))) float lds_bias[];
    RowTile rt;
    if (!row_tile(rt, lds_bias, P.b0, P.nbias, P.M)) return;
    f32x16 emb[2], in[8], out[8];
    float head[3];
    pe_pos(P.pts[rt.rr * 3], P.pts[rt.rr * 3 + 1], P.pts[rt.rr * 3 + 2], rt.h, emb);
    WStream ws;
    // directions vary per point / per loop turn: skip the stream's per-ray DIR prefix (and its b_vf tiles)
    ws_start(ws, P.w0 + SW_STEPS_DIR * SW_STEP_FLOATS, lds_bias + SW_DIR_BIAS_TILES * SW_BIAS_TILE_FLOATS, rt.lds_ring, rt.lane);
    trunk_pass<false>(emb, rt.lds_emb, 0.f, false, rt.h, in, out, head, ws);
    float rgb[3];
    views_mean(in, ws, P.wvl, P.dirs, P.V, P.shared, rt.rr, rt.h, lds_bias, rgb);
    if (rt.live && rt.h == 0) {
        f32x4 r4 = {rgb[0], rgb[1], rgb[2], head[0]};
        *reinterpret_cast<f32x4*>(P.out + rt.row * 4) = r4;
    }
}

int sw_tnerf_render_launch(const swnerf_pass_args& a, hipStream_t st);     // tnerf_kernels.hip
// colour_kernels.hip: phases B and C of a launch whose tiles stashed their live rows (view_ws.h, the deferred colour branch)
int sw_colour_split_launch(const swnerf_pass_args& a, const ViewWs& vw, const float* b0, int nbias, const float* wvl, hipStream_t st);

extern "C" int swnerf_render_pass_ws(const swnerf_pass_args* args, float* view_ws, int64_t view_ws_floats, void* stream) {
    static const PassAccepts accepts = {"render_pass", {SW_COLS(11) | SW_COLS(12), SW_COLS(11) | SW_COLS(12), SW_COLS(8), ~0u /* checked by its launch */},
        SWNERF_E_ARG, "%s: ray_batch must have 11 or 12 columns (use_viewdirs) or 8 (SWNERF_NET_NOVIEW), got %d for kind %d", true, 0};
    if (!args) return sw_fail(SWNERF_E_ARG, "render_pass: NULL args");
    const swnerf_pass_args& a = *args;
    if (a.kind < 0 || a.kind > SWNERF_NET_TNERF) return sw_fail(SWNERF_E_ARG, "unknown net kind %d", a.kind);
    int rc = pass_check(accepts, a);
    if (rc) return rc;
    if (a.kind == SWNERF_NET_TNERF) return sw_tnerf_render_launch(a, (hipStream_t)stream);      // its own translation unit (tnerf_kernels.hip)
    const bool noview = a.kind == SWNERF_NET_NOVIEW;
    if (a.kind == SWNERF_NET_DNERF && a.cols != 12) return sw_fail(SWNERF_E_ARG, "render_pass: D-NeRF needs the frame_time column");
    if (noview && a.dx) return sw_fail(SWNERF_E_ARG, "render_pass: a static net has no position_delta output here");
    PassDev P = pass_dev(a);
    rc = noview ? stream_ptrs_noview(a.packed, a.out_ch, &P.w0, &P.b0, &P.nbias, &P.two_pass)
                : stream_ptrs(a.kind, a.packed, a.run_deform, &P.w0, &P.b0, &P.nbias, &P.two_pass);
    if (rc) return rc;
    P.dir_steps = noview ? 0 : SW_STEPS_DIR;
    P.time_steps = (a.kind == SWNERF_NET_DNERF && P.two_pass) ? SW_STEPS_TIME : 0;
    size_t lds = SW_LDS_FIXED_FLOATS * sizeof(float);
    if ((rc = pass_resampling(accepts.name, a, P, lds))) return rc;
    // the deferred colour branch (view_ws.h): static net, no `raw` (which needs every row's colour) and a sample count whose
    // bookkeeping leaves rows in the least workspace; every other launch runs the view layer in line
    if (view_ws && view_ws_floats < a.n_rays * (int64_t)SW_DEFER_WS_FLOATS)
        return sw_fail(SWNERF_E_ARG, "render_pass: view_ws holds %lld floats, %lld rays need %lld", (long long)view_ws_floats,
                       (long long)a.n_rays, (long long)(a.n_rays * (int64_t)SW_DEFER_WS_FLOATS));
    if (view_ws && a.kind == SWNERF_NET_CANON && !a.raw && a.n_samples <= SW_DEFER_SMAX) P.vw = view_ws_layout(view_ws, view_ws_floats, a.n_rays, a.n_samples);
    if (a.n_rays == 0) return 0;
    if (P.time_steps) {                          // the four waves' per-ray TIME tiles, behind everything else
        P.tb_off = (int)(lds / sizeof(float));
        lds += 4 * SW_TB_LDS_FLOATS * sizeof(float);
    }
    const dim3 grid((unsigned)((a.n_rays + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
    pass_startup_args(P, grid.x, noview ? SW_NOVIEW_STEPS : (a.kind == SWNERF_NET_DNERF && P.two_pass ? SW_DEFORM_STEPS + SW_CANON_STEPS : SW_CANON_STEPS));
    if (noview) hipLaunchKernelGGL((render_pass_kernel<false, false, 0, false>), grid, block, lds, st, P);
    else if (a.kind == SWNERF_NET_DNERF) hipLaunchKernelGGL(render_pass_kernel<true>, grid, block, lds, st, P);
    else {
        // a canonical-only net has no deformation: position_delta is zeros (NeRFOriginal.forward, model.py:273-296
        // returns torch.zeros_like(input_pts[:, :3])); the static kernel has no dx store, so fill it here
        if (a.dx) {
            rc = sw_check(hipMemsetAsync(a.dx, 0, (size_t)a.n_rays * a.n_samples * 3 * sizeof(float), st), "render_pass dx fill");
            if (rc) return rc;
        }
        hipLaunchKernelGGL(render_pass_kernel<false>, grid, block, lds, st, P);
        // the stashed rows' colours and rgb_map (nobody reads the colours of a launch without rgb_map)
        if (P.vw.base && a.rgb_map) {
            if ((rc = sw_check(hipGetLastError(), "render_pass launch"))) return rc;
            return sw_colour_split_launch(a, P.vw, P.b0, P.nbias, views_loop_ptr(a.kind, a.packed), st);
        }
    }
    return sw_check(hipGetLastError(), "render_pass launch");
}

extern "C" int swnerf_render_pass(const swnerf_pass_args* args, void* stream) { return swnerf_render_pass_ws(args, nullptr, 0, stream); }

extern "C" int64_t swnerf_view_ws_floats(int64_t n_rays, int n_samples) {
    if (n_rays <= 0 || n_samples <= 0) return 0;
    const int64_t full = view_ws_full(n_rays, n_samples), least = n_rays * (int64_t)SW_DEFER_WS_FLOATS;
    return full > least ? full : least;
}

// Coarse sampling alone (nerf/run.py:355-385; API parity for the op-by-op path - the fused pass does this in
// registers): z_vals [N,S] and, when asked, pts = o + d*z [N,S,3].  Same device functions as the fused pass.
__global__ void __launch_bounds__(256) sample_coarse_kernel(swnerf_pass_args a, float* z_out, float* pts) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int S = a.n_samples;
    if (idx >= a.n_rays * S) return;
    const int64_t ray = idx / S;
    const int s = (int)(idx - ray * S);
    const float* rb = a.ray_batch + ray * a.cols;
    const float z = z_sample(a, ray, rb[6], rb[7], s);
    z_out[idx] = z;
    if (pts) {
        pts[idx * 3 + 0] = rb[0] + rb[3] * z;
        pts[idx * 3 + 1] = rb[1] + rb[4] * z;
        pts[idx * 3 + 2] = rb[2] + rb[5] * z;
    }
}

extern "C" int swnerf_sample_coarse(const float* ray_batch, int64_t n_rays, int cols, int n_samples, int lindisp,
                                    const float* t_rand, float* z_vals, float* pts, void* stream) {
    if (n_rays == 0) return 0;                           // empty tensors have NULL data pointers
    if (!ray_batch || !z_vals || n_rays < 0 || n_samples < 1 || cols < 8)
        return sw_fail(SWNERF_E_ARG, "sample_coarse: NULL pointer, n_rays %lld, n_samples %d or cols %d < 8", (long long)n_rays, n_samples, cols);
    swnerf_pass_args a = {};
    a.ray_batch = ray_batch; a.n_rays = n_rays; a.cols = cols; a.n_samples = n_samples; a.lindisp = lindisp; a.t_rand = t_rand;
    const int64_t total = n_rays * n_samples;
    hipLaunchKernelGGL(sample_coarse_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, z_vals, pts);
    return sw_check(hipGetLastError(), "sample_coarse launch");
}

extern "C" int swnerf_query_points(const float* packed, const float* pts, int64_t M, const float* dirs, int64_t n_dirs,
                                   int shared_dirs, int L_pos, int L_dir, float* out, void* stream) {
    if (M == 0 && packed) return 0;
    if (!packed || !pts || !dirs || !out || M < 0) return sw_fail(SWNERF_E_ARG, "query_points: NULL pointer or negative M");
    if (int rc = sw_check_bands("query_points", 2, L_pos, L_dir)) return rc;
    if (shared_dirs ? n_dirs < 1 : n_dirs != M)
        return sw_fail(SWNERF_E_ARG, "query_points: need %s directions, got %lld for %lld points", shared_dirs ? ">= 1 shared" : "one per point", (long long)n_dirs, (long long)M);
    QueryDev P;
    P.pts = pts; P.M = M; P.dirs = dirs; P.V = n_dirs; P.shared = shared_dirs ? 1 : 0; P.out = out;
    P.w0 = packed; P.b0 = packed + SW_CANON_W_FLOATS; P.nbias = SW_CANON_BIAS_TILES * SW_BIAS_TILE_FLOATS;
    P.wvl = packed + SW_CANON_VL_OFFSET;
    return sw_launch_rows(query_points_kernel, P, M, SW_LDS_FIXED_FLOATS * sizeof(float), stream, "query_points launch");
}

extern "C" int swnerf_mlp_forward(int kind, const float* packed, const float* x, int64_t M, int L_pos, int L_dir,
                                  const float* t_emb, int L_time, int run_deform, float* out, float* dx_out, void* stream) {
    if (M == 0 && packed) return 0;
    if (!packed || !x || !out || M < 0) return sw_fail(SWNERF_E_ARG, "mlp_forward: NULL pointer or negative M");
    if (int rc = sw_check_bands("mlp_forward", 3, L_pos, L_dir, L_time)) return rc;
    if (kind == SWNERF_NET_DNERF && run_deform && !t_emb) return sw_fail(SWNERF_E_ARG, "mlp_forward: D-NeRF deformation needs t_emb");
    MlpDev P;
    P.x = x; P.M = M; P.Lp = L_pos; P.Ld = L_dir; P.Lt = L_time;
    P.Cpos = 3 * (1 + 2 * L_pos); P.C = P.Cpos + 3 * (1 + 2 * L_dir);
    P.t_emb = t_emb; P.Ct = 1 + 2 * L_time;
    P.out = out; P.dx = dx_out; P.act = nullptr; P.bits = nullptr;
    int rc = stream_ptrs(kind, packed, run_deform, &P.w0, &P.b0, &P.nbias, &P.two_pass);
    if (rc) return rc;
    P.wvl = views_loop_ptr(kind, packed);
    return sw_launch_rows(kind == SWNERF_NET_DNERF ? mlp_forward_kernel<true> : mlp_forward_kernel<false>, P, M,
                          SW_LDS_FIXED_FLOATS * sizeof(float), stream, "mlp_forward launch");
}

// model.forward(x) for the net WITHOUT view directions (SWNERF_NET_NOVIEW; model.py:39-47, 59-60): x [M, C_pos] (any
// further columns of a wider row are ignored, like torch.split's second half with input_ch_views = 0), out [M, out_ch].
struct MlpNoviewDev { const float* x; int64_t M; int C; int Lp; const float* w0; const float* b0; int nbias; int out_ch; float* out; };

__global__ void __launch_bounds__(256, 1) mlp_forward_noview_kernel(MlpNoviewDev P) {
    extern __shared__ __attribute__((aligned(16))) float lds_bias[];
    RowTile rt;
    if (!row_tile(rt, lds_bias, P.b0, P.nbias, P.M)) return;
    f32x16 emb[2], in[8], out[8];
    float head[3];
    gather_pos(P.x + rt.rr * P.C, rt.h, P.Lp, emb);
    WStream ws;
    ws_start(ws, P.w0, lds_bias, rt.lds_ring, rt.lane);
    trunk_pass<false, false, false, true>(emb, rt.lds_emb, 0.f, false, rt.h, in, out, head, ws);
    float rgb[3], extra;
    noview_heads(in, ws, P.out_ch, P.out_ch, rgb, head, extra);
    if (rt.live && rt.h == 0) {
        float* o = P.out + rt.row * P.out_ch;
        o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2]; o[3] = head[0];
        if (P.out_ch == 5) o[4] = extra;
    }
}

// vallina_NeRF.forward on embedded rows for use_viewdirs=False (model.py:39-47, 59-60): x [M, ldx >= C_pos] -> out [M, out_ch]
extern "C" int swnerf_mlp_forward_noview(const float* packed, const float* x, int64_t M, int ldx, int L_pos, int out_ch, float* out, void* stream) {
    if (M == 0 && packed) return 0;
    if (!packed || !x || !out || M < 0) return sw_fail(SWNERF_E_ARG, "mlp_forward_noview: NULL pointer or negative M");
    if (int rc = sw_check_bands("mlp_forward_noview", 1, L_pos)) return rc;
    if (ldx < 3 * (1 + 2 * L_pos)) return sw_fail(SWNERF_E_ARG, "mlp_forward_noview: rows of %d floats cannot hold %d embedded columns", ldx, 3 * (1 + 2 * L_pos));
    MlpNoviewDev P;
    P.x = x; P.M = M; P.C = ldx; P.Lp = L_pos; P.out_ch = out_ch; P.out = out;
    int two = 0;
    int rc = stream_ptrs_noview(packed, out_ch, &P.w0, &P.b0, &P.nbias, &two);
    if (rc) return rc;
    return sw_launch_rows(mlp_forward_noview_kernel, P, M, SW_LDS_FIXED_FLOATS * sizeof(float), stream, "mlp_forward_noview launch");
}
