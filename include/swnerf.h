/* swnerf.h - C ABI of libswnerf_hip.so: the MI355X (gfx950) NeRF volumetric renderer.
 *
 * Drop-in boundary for the render hot path of daihangpku/SW-NeRF.
 * The reference has no FFI layer: its "operator API" is the Python symbols of ray.py,
 * embedder.py, model.py and the render_rays/run_network functions of the runner scripts.
 * Each entry point below names the reference symbol (file:line under /root/reference)
 * whose arithmetic it replaces; sw-nerf_amd/swnerf/ binds them with ctypes and
 * re-exports the reference's Python names/signatures.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous float32 unless marked HOST;
 *     the caller (torch) allocates inputs AND outputs; nothing is retained after return
 *   - sizes are int64_t, flags int; `stream` is a hipStream_t passed as void*
 *     (torch.cuda.current_stream().cuda_stream); all work is enqueued asynchronously
 *   - return 0 on success, a negative SWNERF_E_* for argument errors, or a positive
 *     hipError_t; swnerf_last_error() returns a thread-local message
 *   - an optional output/input may be NULL where the comment says so
 */
#ifndef SWNERF_H
#define SWNERF_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWNERF_VERSION 112

#define SWNERF_E_ARG      (-1)   /* bad size / NULL pointer / unsupported shape */
#define SWNERF_E_UNSUPP   (-2)   /* valid in the reference, not built here (message says what) */
#define SWNERF_E_DATA     (-3)   /* the bytes of a file are corrupt (message says where) */

/* packed-network kinds (swnerf_packed_floats / swnerf_pack_*) */
#define SWNERF_NET_CANON   0     /* vallina_NeRF == NeRFOriginal: 8x256, skip@4, view branch */
#define SWNERF_NET_DNERF   1     /* DirectTemporalNeRF: deformation net then canonical net   */
#define SWNERF_NET_NOVIEW  2     /* vallina_NeRF with use_viewdirs=False (the reference's argparse default, utils.py:43;
                                    model.py:59-60): 8x256, skip@4, outputs = output_linear(h), 4 or 5 channels */
#define SWNERF_NET_TNERF   3     /* TNeRF (model.py:152-210; t_nerf/run_tnerf.py): 8x128 ELU trunk, skip [gamma(x)|gamma(t)] @5,
                                    density, feature -> layer_9 (64, ELU) -> color (3, ReLU); fused render pass only */

/* SWNERF_NET_TNERF packing: `params` = the 24 TNeRF tensors in named_parameters() order (model.py:155-190):
 *   [0..15]  layers.{0..7}.0.{weight,bias}       layer 0 [128, C_pos + C_time], layer 5 [128, C_pos + C_time + 128], others [128,128]
 *   [16,17]  density.0.{weight,bias}             [1,128]
 *   [18,19]  feature.0.{weight,bias}             [128,128]
 *   [20,21]  layer_9.0.{weight,bias}             [64, 128 + C_dir]
 *   [22,23]  color.0.{weight,bias}               [3,64]
 * swnerf_pack_net(SWNERF_NET_TNERF, params, L_pos, L_dir, L_time, packed, stream); L_dir >= 1.
 * swnerf_packed_floats(SWNERF_NET_TNERF) = (steps + 16) * 256 + 45 * 32 + 64 * 160 + 64 = 165344 floats, steps = 40 per-ray
 * prefix steps + 544 per-tile steps (1 step = 256 floats = the A operands of 4 MFMAs; 16 = the ring tail; 45 bias-style tiles of
 * 32 floats; the folded layer_9, [64][160] + its bias).  The pack step folds feature into layer_9 (fp64 product, one rounding). */

int         swnerf_version(void);
const char* swnerf_last_error(void);

/* ---- weights -------------------------------------------------------------------------
 * The fused kernels stream weights in MFMA-fragment order (DESIGN.md "packed layout").
 * Repack after every optimizer step.  `params` is a HOST array of DEVICE pointers in
 * state_dict order of model.py:22-37 / 251-269:
 *   [0..15]  pts_linears.{0..7}.{weight,bias}   (weight [out,in] row-major as in torch)
 *   [16,17]  views_linears.0.{weight,bias}      [128, 256+C_dir]
 *   [18,19]  feature_linear.{weight,bias}       [256,256]
 *   [20,21]  alpha_linear.{weight,bias}         [1,256]
 *   [22,23]  rgb_linear.{weight,bias}           [3,128]
 * and for SWNERF_NET_DNERF additionally (model.py:108-126)
 *   [24..39] _time.{0..7}.{weight,bias}         layer 0 is [256, C_pos + C_time]
 *   [40,41]  _time_out.{weight,bias}            [3,256]
 * L_pos / L_dir / L_time = number of frequency bands of the embedders
 * (embedder.py:44-59: multires=10 -> C_pos 63, multires_views=4 -> C_dir 27,
 * time multires=10 -> C_time 21).  Limits: L_pos <= 10, L_dir <= 4, L_time <= 10.
 * Since version 109 the pack step FOLDS feature_linear into views_linears.0 (model.py:49-53: feature_linear has no
 * activation, so views_linears.0(cat[feature_linear(h), dirs]) = [Wv[:, :256] W_f | Wv[:, 256:]] . cat[h, dirs] + (Wv[:, :256] b_f
 * + b_v); the product is formed in double and rounded once): the kernels run ONE 128 x (256 + C_dir) layer where the
 * reference runs a 256 x 256 and a 128 x (256 + C_dir) one - 11 % fewer MFMAs per row, same function.  The caller's
 * tensors, their gradients (swnerf_feature_finish) and checkpoints are untouched.
 * Since version 110 a SWNERF_NET_DNERF blob carries layer 0 of the deformation net (model.py:129: _time.0 on cat[gamma(x),
 * gamma(t)]) as two segments - bias + the gamma(t) columns, then the gamma(x) columns: the fused passes evaluate the first ONCE PER
 * RAY (one frame time per ray, run_dnerf.py:354-360), the per-row entry points (swnerf_mlp_forward, deform_forward_train) in line.
 * Same function, same blob size; blobs are not interchangeable across versions (they are made per process, never stored). */
size_t swnerf_packed_floats(int kind);
int swnerf_pack_net(int kind, const float* const* params /*HOST*/, int L_pos, int L_dir,
                    int L_time, float* packed, void* stream);
/* SWNERF_NET_NOVIEW (model.py:22-37 with use_viewdirs=False): params =
 *   [0..15]  pts_linears.{0..7}.{weight,bias}
 *   [16,17]  output_linear.{weight,bias}        [out_ch,256], out_ch = 4 or 5 (nerf/run.py:231)
 * packed: swnerf_packed_floats(SWNERF_NET_NOVIEW) floats. */
int swnerf_pack_net_noview(const float* const* params /*HOST*/, int L_pos, int out_ch, float* packed, void* stream);
/* vallina_NeRF.forward for that net (model.py:39-47, 59-60) on embedded rows: x [M, ldx] whose first 3(1+2 L_pos) columns are
 * gamma(x) -> out [M, out_ch] = output_linear(h).  The op-by-op form (run_network, nerf/run.py:73-87); the fused render pass
 * takes the same packed blob with kind SWNERF_NET_NOVIEW. */
int swnerf_mlp_forward_noview(const float* packed, const float* x, int64_t M, int ldx, int L_pos, int out_ch, float* out, void* stream);

/* ---- ray.py -------------------------------------------------------------------------- */

/* get_rays (ray.py:10-38) for the pixel range [ray0, ray0+n) of an HxW image in row-major
 * order.  focal_branch!=0 selects the float-focal branch (:26-29: cx=W/2, cy=H/2, fy=fx).
 * c2w: HOST, 12 floats, row-major [3,4].  rays_o may be NULL. */
int swnerf_get_rays(int H, int W, double fx, double fy, double cx, double cy, int focal_branch,
                    const float* c2w /*HOST*/, int64_t ray0, int64_t n,
                    float* rays_o /*[n,3]*/, float* rays_d /*[n,3]*/, void* stream);

/* ndc_rays (ray.py:75-92).  In-place allowed (o_out==rays_o, d_out==rays_d). */
int swnerf_ndc_rays(int H, int W, double focal, double near, const float* rays_o, const float* rays_d,
                    int64_t n, float* o_out, float* d_out, void* stream);

/* The ray-batch packing inside render() (nerf/run.py:137-158, d_nerf/run_dnerf.py:137-160):
 * viewdirs = d/|d| taken BEFORE the optional NDC warp; rows = [o(3) d(3) near far (t) viewdirs(3)].
 * has_time!=0 -> 12 columns with frame_time at column 8, else 11 columns. */
int swnerf_pack_ray_batch(const float* rays_o, const float* rays_d, int64_t n, double near, double far,
                          int has_time, double frame_time, int ndc, int H, int W, double ndc_focal,
                          float* ray_batch, void* stream);

/* raw2outputs (ray.py:155-198).  noise: NULL or [N,S] already multiplied by raw_noise_std.
 * Any output may be NULL.  disp is NaN where acc==0, like the reference. */
int swnerf_raw2outputs(const float* raw /*[N,S,4]*/, const float* z_vals /*[N,S]*/,
                       const float* rays_d /*[N,3]*/, const float* noise, int64_t N, int S,
                       int white_bkgd, float* rgb_map /*[N,3]*/, float* disp_map, float* acc_map,
                       float* weights /*[N,S]*/, float* depth_map, void* stream);

/* Gradient of raw2outputs w.r.t. raw (autograd of ray.py:155-198; the loss of nerf/run.py:688-697
 * reaches it through rgb_map / rgb0).  g_*: upstream gradients of the five outputs, each may be NULL;
 * d_raw [N,S,4] is overwritten.  z_vals and rays_d get no gradient (they are detached inputs of the
 * render path).  2 <= S <= 1024. */
int swnerf_raw2outputs_backward(const float* raw, const float* z_vals, const float* rays_d, const float* noise,
                                int64_t N, int S, int white_bkgd, const float* g_rgb /*[N,3]*/,
                                const float* g_disp /*[N]*/, const float* g_acc /*[N]*/, const float* g_depth /*[N]*/,
                                const float* g_weights /*[N,S]*/, float* d_raw /*[N,S,4]*/, void* stream);

/* sample_pdf (ray.py:96-153).  bins [N,nb], weights [N,nb-1]; u: NULL -> det linspace(0,1,n_samples)
 * (det=True), else [N,n_samples] uniforms (replaces torch.rand).  samples [N,n_samples].
 * If z_vals ([N,S]) and z_sorted ([N,S+n_samples]) are given, also writes
 * sort(cat[z_vals, samples]) (nerf/run.py:400); z_std ([N], std of samples, :416) may be NULL. */
int swnerf_sample_pdf(const float* bins, const float* weights, int64_t N, int nb, int n_samples,
                      const float* u, float* samples, const float* z_vals, int S, float* z_sorted,
                      float* z_std, void* stream);

/* ---- embedder.py --------------------------------------------------------------------- */

/* Embedder.embed (embedder.py:33-42): x [M,d] -> [M, d*(1+2L)], frequency-major, sin before cos.
 * 1 <= d <= 16, 0 <= L <= 24 (else SWNERF_E_ARG).  Every sin / cos within 1.2e-7 of the exact value of the float x * 2^k for
 * |x * 2^k| < 3e9 (all 24 bands at |x| <= 6 are tested: |y| <= 5.1e7): bands k < 10 are the float arithmetic of the fused
 * passes, bit for bit; bands k >= 10 reduce their argument in double. */
int swnerf_embed(const float* x, int64_t M, int d, int L, float* out, void* stream);

/* ---- model.py ------------------------------------------------------------------------ */

/* vallina_NeRF.forward / NeRFOriginal.forward (model.py:39-62, 273-296), use_viewdirs=True:
 * x [M, C_pos+C_dir] already-embedded rows -> out [M,4] = [rgb(3), sigma].
 * DirectTemporalNeRF.forward (model.py:138-151): packed kind DNERF, t_emb [M,C_time] = embedded
 * frame time (ts[0]); run_deform==0 takes the `t==0 and zero_canonical` branch (dx=0);
 * dx_out [M,3] may be NULL. */
int swnerf_mlp_forward(int kind, const float* packed, const float* x, int64_t M, int L_pos, int L_dir,
                       const float* t_emb, int L_time, int run_deform,
                       float* out /*[M,4]*/, float* dx_out /*[M,3]*/, void* stream);

/* ---- training path of the MLP (autograd of model.py:39-62) -----------------
 * forward_train: as swnerf_mlp_forward (SWNERF_NET_CANON) and additionally saves, per row, the
 *   activations the weight-gradient GEMMs need: act [M, swnerf_act_floats_per_row()] row-major
 *   (h_l post-ReLU at column 256*l, l=0..7; columns 2048..2303 unused - feature_linear's output is never formed, see
 *   swnerf_pack_net; views hidden at 2304), and the
 *   ReLU bit masks of every 32-row tile: bits [swnerf_mask_floats(M)] (1 KiB per tile and layer; opaque,
 *   only the backward_dx entry points read it).
 * pack_net_bwd: the transposed weight stream of the dX chain (params as for swnerf_pack_net, first 24).
 * backward_dx: bits from forward_train, d_out [M,4] = d raw -> grad [M, same layout as act] =
 *   d(pre-activation) of every layer.
 * gemm_tn: C[No,ldc] += A[M,lda]^T . B[M,ldb] (first No / Ni columns), bias[No] += column sums of A
 *   (bias may be NULL): dW and db of one Linear layer from `grad` and `act`/inputs.  C and bias accumulate:
 *   zero them first.  No <= 256. */
size_t swnerf_packed_bwd_floats(void);
size_t swnerf_act_floats_per_row(void);
size_t swnerf_mask_floats(int64_t M);
int swnerf_mlp_forward_train(const float* packed, const float* x, int64_t M, int L_pos, int L_dir,
                             float* out /*[M,4]*/, float* act, float* bits, void* stream);
int swnerf_pack_net_bwd(const float* const* params /*HOST*/, int L_pos, int L_dir, float* packed_bwd, void* stream);
int swnerf_mlp_backward_dx(const float* packed_bwd, const float* bits, const float* d_out /*[M,4]*/, int64_t M,
                           float* grad, void* stream);
int swnerf_gemm_tn(const float* A, int lda, int No, const float* B, int ldb, int Ni, int64_t M,
                   float* C, int ldc, float* bias, void* stream);
/* gemm_tn for a 256 x 256 block (No = Ni = 256) with up to two riders that share one of its operands (each may be NULL):
 *   B2 [M, Ni2 <= 64]:  C2[256, ldc2] += A^T . B2            (the gamma(x) columns of a skip layer: same A; rides on the
 *                       block's own pass over the rows)
 *   A2 [M, No2 <= 32]:  C3[No2, ldc3] += A2^T . B,  bias3[No2] += column sums of A2   (a convenience: it costs its own launch,
 *                       the swnerf_gemm_tn call it stands for, on the same stream)
 * Equivalent to the corresponding separate swnerf_gemm_tn calls (which it falls back to for small or unaligned M). */
int swnerf_gemm_tn_fused(const float* A, int lda, const float* B, int ldb, int64_t M, float* C, int ldc, float* bias,
                         const float* B2, int ldb2, int Ni2, float* C2, int ldc2,
                         const float* A2, int lda2, int No2, float* C3, int ldc3, float* bias3, void* stream);
/* Several swnerf_gemm_tn_fused problems over the SAME M rows (the weight-gradient GEMMs of one row chunk of a training step:
 * loss.backward() of nerf/run.py:700) as ONE launch: the workgroups are dealt out over the items in proportion to their work,
 * so the chunk pays one launch ramp and one atomic epilogue instead of one per layer.  Field meaning as the arguments of
 * swnerf_gemm_tn_fused (riders may be NULL; an A2 rider is a launch of its own here too).  Every item's arguments are checked before the first
 * launch.  Results equal the separate calls' (split-K atomics add in a different order). */
typedef struct swnerf_gemm_item {
    const float* A; int lda; const float* B; int ldb; float* C; int ldc; float* bias;
    const float* B2; int ldb2; int Ni2; float* C2; int ldc2;
    const float* A2; int lda2; int No2; float* C3; int ldc3; float* bias3;
} swnerf_gemm_item;
int swnerf_gemm_tn_group(const swnerf_gemm_item* items /*HOST*/, int n_items, int64_t M, void* stream);
/* swnerf_gemm_tn_group in "bf16x3" arithmetic (opt-in): the main 256 x 256 product of every item that qualifies for
 * the LDS-DMA kernel (16-byte aligned rows, M >= 4096; the first 16 such items) is evaluated as A_hi.B_hi + A_hi.B_lo + A_lo.B_hi on
 * split-bf16 operands with fp32 accumulation, all of them as ONE launch; per entry |error| <= (2^-14 + n u) |A|^T |B| + n u |C0|, n = 3 M + 514.
 * Bias column sums, both riders, and every item that does not qualify are fp32, as in swnerf_gemm_tn_group.  Same argument checks. */
int swnerf_gemm_tn_group_x3(const swnerf_gemm_item* items /*HOST*/, int n_items, int64_t M, void* stream);

/* ---- training path of DirectTemporalNeRF (autograd of model.py:128-151; the loss of
 * d_nerf/run_dnerf.py:690-725 needs d/d(position_delta) too).  The forward is the composition the
 * reference runs: deformation net -> dx; gamma(x + dx) (swnerf_embed); canonical net
 * (swnerf_mlp_forward_train on [gamma(x+dx), gamma(d)]).  Backward: canonical dX chain that also returns
 * the gradient w.r.t. the re-embedded positions (through the sin/cos of gamma), then the deformation dX chain
 * seeded with d dx = d pts + d position_delta.
 * Backward stream kinds for swnerf_packed_bwd_floats_kind / swnerf_pack_net_bwd_kind:
 *   SWNERF_BWD_CANON            what swnerf_pack_net_bwd writes (params: the 24 canonical tensors)
 *   SWNERF_BWD_CANON_INPUT_GRAD the same plus the position-embedding columns of pts_linears.0/.5
 *   SWNERF_BWD_DEFORM           `_time.1..7` trunk columns + `_time_out.weight` (params: the 18 tensors
 *                               _time.0.weight, _time.0.bias, ..., _time_out.weight, _time_out.bias)
 * deform_forward_train: packed = a SWNERF_NET_DNERF blob; x [M,C] as for swnerf_mlp_forward, t_emb [M,1+2*L_time];
 *   writes dx [M,3], act_d [M, swnerf_act_floats_per_row()] (h_l of `_time` at column 256*l) and
 *   bits_d [swnerf_mask_floats(M)].
 * backward_dx_pts: as swnerf_mlp_backward_dx with a SWNERF_BWD_CANON_INPUT_GRAD stream; pts [M,3] = the
 *   positions that were embedded (x + dx); also writes d_pts [M,3].
 * deform_backward_dx: bits_d, d_dx [M,3] -> grad_d [M, same layout as act_d] = d(pre-activation) of `_time.l`. */
#define SWNERF_BWD_CANON 0
#define SWNERF_BWD_CANON_INPUT_GRAD 1
#define SWNERF_BWD_DEFORM 2
#define SWNERF_BWD_DNERF_FUSED       3   /* CANON_INPUT_GRAD then DEFORM as ONE stream (params: the 42 DirectTemporalNeRF tensors) */
size_t swnerf_packed_bwd_floats_kind(int bwd_kind);
int swnerf_pack_net_bwd_kind(int bwd_kind, const float* const* params /*HOST*/, int L_pos, int L_dir,
                             float* packed_bwd, void* stream);
int swnerf_deform_forward_train(const float* packed, const float* x, const float* t_emb, int64_t M,
                                int L_pos, int L_dir, int L_time, float* dx /*[M,3]*/, float* act_d, float* bits_d, void* stream);
int swnerf_mlp_backward_dx_pts(const float* packed_bwd, const float* bits, const float* d_out /*[M,4]*/,
                               const float* pts /*[M,3]*/, int64_t M, int L_pos,
                               float* grad, float* d_pts /*[M,3]*/, void* stream);
int swnerf_deform_backward_dx(const float* packed_bwd, const float* bits_d, const float* d_dx /*[M,3]*/, int64_t M,
                              float* grad_d, void* stream);

/* network_query_fn on bare points (nerf/load_model.py:56-74; nerf/extract_mesh.py:27-90, :155-175):
 * pts [M,3] world positions, packed = a SWNERF_NET_CANON blob; the positional encodings are
 * evaluated in registers.  shared_dirs == 0: dirs [M,3], one direction per point -> out [M,4] = raw
 * [rgb(3), sigma].  shared_dirs != 0: dirs [V,3] shared by every point -> out [M,4] =
 * [mean over the V directions of the raw rgb, sigma] (what sample_grid averages); the trunk and
 * the density are evaluated once per point, only the view branch V times. */
int swnerf_query_points(const float* packed, const float* pts, int64_t M, const float* dirs, int64_t n_dirs,
                        int shared_dirs, int L_pos, int L_dir, float* out /*[M,4]*/, void* stream);

/* The same query for the two time-conditioned nets at ONE frame time (a grid of a dynamic scene at time t: nerf/extract_mesh.py
 * sample_grid :27-90 with the runner's own query in place of the static one).  frame_time is a constant of the call, the
 * reference's "Only accepts all points from same time" (d_nerf/run_dnerf.py:53, t_nerf/run_tnerf.py:52).
 *   SWNERF_NET_DNERF  run_network (d_nerf/run_dnerf.py:46-83) + DirectTemporalNeRF.forward (model.py:128-151): the deformation
 *                     net -> dx, gamma(x + dx), the canonical trunk and the density once per point, the view branch once per
 *                     direction.  run_deform == 0 takes the `t == 0 and zero_canonical` branch (model.py:143-145: the canonical
 *                     net alone, dx = 0).  dx_out [M,3] (position_delta) may be NULL.  dirs / shared_dirs / out as above.
 *   SWNERF_NET_TNERF  run_network (t_nerf/run_tnerf.py:48-87) + TNeRF.forward (model.py:192-210): out [M,4] = [mean over the V
 *                     directions of rgb (after `color`'s ReLU), density].  Shared directions only (shared_dirs == 0 is
 *                     SWNERF_E_UNSUPP), no dx_out (non-NULL is SWNERF_E_ARG), run_deform is ignored, L_dir >= 1.
 * Any other kind is SWNERF_E_ARG.  Limits: L_pos <= 10, L_dir <= 4, L_time <= 10 (else SWNERF_E_UNSUPP). */
int swnerf_query_points_time(int kind, const float* packed, const float* pts, int64_t M, const float* dirs, int64_t n_dirs,
                             int shared_dirs, double frame_time, int run_deform, int L_pos, int L_dir, int L_time,
                             float* out /*[M,4]*/, float* dx_out /*[M,3] or NULL*/, void* stream);

/* Marching cubes (nerf/extract_mesh.py generate_mesh :92-131, in place of skimage.measure.marching_cubes): the iso-surface
 * f = level of a scalar field of nx * ny * nz points in C order (i slowest), consecutive points `ld` floats apart (ld = 1: a
 * dense [nx,ny,nz] array; ld = 4: the sigma column of swnerf_query_points' [M,4] output).  A corner is inside iff f > level
 * (strict, fp32; NaN is outside).  Every dimension must be >= 2.  Two calls on one workspace of
 * swnerf_mc_workspace_bytes(nx,ny,nz) bytes (0 for a dimension < 2):
 *   swnerf_mc_count  classifies the grid and writes totals[2] = {vertices, triangles} (DEVICE int64); the caller reads them
 *                    once (the only host synchronisation) to size the outputs
 *   swnerf_mc_emit   same field / level / workspace; writes verts [V,3], normals [V,3] (unit, pointing toward lower f; (0,0,0)
 *                    where the interpolated gradient is zero or not finite), faces [F,3] int32 wound outward from the dense
 *                    side, and with colors != NULL (3 floats per point, `colors_ld` floats apart) vertex_colors [V,3] = the
 *                    colour of the edge end point nearer the vertex.  spacing / origin are HOST float[3]: vertex coordinate
 *                    = index * spacing + origin.  V or F above INT32_MAX is an error; V = F = 0 writes nothing.
 * Vertices are shared per grid edge (ordered by owner point, then axis x < y < z), so the mesh is indexed and, away from the
 * grid faces, closed.  Deterministic: no atomics. */
size_t swnerf_mc_workspace_bytes(int64_t nx, int64_t ny, int64_t nz);
int swnerf_mc_count(const float* field, int64_t nx, int64_t ny, int64_t nz, int64_t ld, float level,
                    void* workspace, int64_t* totals /*[2]*/, void* stream);
int swnerf_mc_emit(const float* field, const float* colors, int64_t nx, int64_t ny, int64_t nz, int64_t ld, int64_t colors_ld,
                   float level, const float* spacing /*HOST [3]*/, const float* origin /*HOST [3]*/, void* workspace,
                   int64_t n_verts, int64_t n_tris, float* verts /*[V,3]*/, int32_t* faces /*[F,3]*/, float* normals /*[V,3]*/,
                   float* vertex_colors /*[V,3] or NULL*/, void* stream);

/* Coarse sampling of render_rays on its own (nerf/run.py:355-385): z_vals [N,S] = near(1-t)+far*t with t = linspace(0,1,S)
 * (or the lindisp form, :365), stratified jitter when t_rand [N,S] is given (:369-383: replaces torch.rand);
 * pts [N,S,3] = rays_o + rays_d * z (:385) may be NULL.  ray_batch as for swnerf_render_pass (columns 0-7 are read). */
int swnerf_sample_coarse(const float* ray_batch, int64_t n_rays, int cols, int n_samples, int lindisp,
                         const float* t_rand, float* z_vals /*[N,S]*/, float* pts /*[N,S,3]*/, void* stream);

/* ---- fused render pass (render_rays, nerf/run.py:316-422, d_nerf/run_dnerf.py:354-480) -------
 * One wavefront owns one ray: sampling -> positional encoding -> MLP (MFMA, register
 * resident) -> alpha compositing -> optional hierarchical resampling, with no HBM traffic
 * for pts / embeddings / activations / raw. */
typedef struct swnerf_pass_args {
    /* inputs */
    const float* ray_batch;   /* [N, cols]  cols = 11, or 12 with frame_time at column 8; SWNERF_NET_NOVIEW: 8 = [o, d, near, far]
                                 (rays without view directions, nerf/run.py:152-157) */
    int64_t      n_rays;
    int          cols;
    int          kind;        /* SWNERF_NET_CANON / SWNERF_NET_DNERF / SWNERF_NET_NOVIEW */
    const float* packed;      /* packed net of that kind */
    int          run_deform;  /* DNERF only: 0 = `t==0 and zero_canonical` branch */
    int          L_pos, L_dir, L_time;
    int          n_samples;   /* S of THIS pass */
    const float* z_vals;      /* NULL: coarse sampling from near/far (nerf/run.py:361-367);
                                 else [N,S] given depths (fine pass, or run_dnerf.py:408) */
    int          lindisp;
    const float* t_rand;      /* NULL or [N,S] stratified jitter (perturb>0, nerf/run.py:369-383) */
    const float* noise;       /* NULL or [N,S] density noise, pre-scaled (ray.py:176-184) */
    int          white_bkgd;
    /* per-ray outputs, any may be NULL */
    float* rgb_map;           /* [N,3] */
    float* disp_map;          /* [N]   */
    float* acc_map;           /* [N]   */
    float* depth_map;         /* [N]   */
    /* per-sample outputs, any may be NULL */
    float* weights;           /* [N,S]   */
    float* raw;               /* [N,S,4]  (SWNERF_NET_NOVIEW: [N,S,out_ch]) */
    float* dx;                /* [N,S,3] position_delta (DNERF) */
    float* z_out;             /* [N,S]   the depths this pass sampled */
    /* hierarchical resampling after compositing (nerf/run.py:394-400), n_importance==0: off */
    int          n_importance;
    const float* u;           /* NULL: det (perturb==0); else [N,n_importance] uniforms */
    float* z_fine;            /* [N, S+n_importance] sorted union */
    float* z_std;             /* [N] std of the new samples, may be NULL */
    int          out_ch;      /* SWNERF_NET_NOVIEW: channels of output_linear (4 or 5); ignored otherwise */
} swnerf_pass_args;

int swnerf_render_pass(const swnerf_pass_args* args /*HOST*/, void* stream);

/* swnerf_render_pass with a workspace for its deferred colour branch: view_ws = view_ws_floats floats of scratch, or NULL
 * (= swnerf_render_pass).  With it the launch evaluates the view layer and the rgb head only on a ray's sample 0 and on its
 * samples with alpha != 0 - a sample with alpha == 0 enters no output with its colour; without it on every sample.  Three
 * kernels on `stream`: the pass itself stashes those rows' last trunk activations in the workspace and writes every output
 * but rgb_map; a persistent kernel runs the view layer and the rgb head on the stashed rows of the whole launch, packed 32
 * to an MFMA segment across rays; a last one forms each ray's colour sums and writes rgb_map.  Same outputs either way
 * (bit for bit unless a colour that was left out is non-finite).
 * The workspace's size decides how many rows a ray can stash; a 32-sample tile whose rows are not certain to fit runs the view
 * layer in line.  swnerf_view_ws_floats(n_rays, n_samples) is the size at which every tile stashes (n_samples rows of 257
 * floats per ray plus bookkeeping); n_rays * 64 * 256 floats is the least accepted (about 60 rows per ray): view_ws != NULL
 * with fewer is SWNERF_E_ARG.  view_ws must be 16-byte aligned; its contents are scratch before and after (the layout:
 * csrc/view_ws.h).
 * Used for SWNERF_NET_CANON launches without `raw` and with n_samples <= 240; every other launch ignores it and runs as
 * swnerf_render_pass does.  Launches that may overlap (different streams) need a workspace each. */
int swnerf_render_pass_ws(const swnerf_pass_args* args /*HOST*/, float* view_ws, int64_t view_ws_floats, void* stream);
int64_t swnerf_view_ws_floats(int64_t n_rays, int n_samples);

/* ---- opt-in reduced-cost precision: "bf16x3" ----------------------------------------------------------------
 * swnerf_render_pass with the MLPs on the bf16 matrix pipe: every fp32 weight and activation is split into two bf16
 * halves (hi + lo, 16 significant bits) and each product is three v_mfma_f32_32x32x16_bf16 with fp32 accumulation
 * (W_hi.x_hi + W_hi.x_lo + W_lo.x_hi).  Sampling, encodings, heads, compositing and resampling stay fp32 and are the
 * same code as swnerf_render_pass.  NOT the parity path (that is fp32 MFMA, bit-comparable to torch's CPU kernels up to
 * summation order); measured deviation from it: DESIGN.md 7c.  Inference only; both net kinds.
 * args->packed = a blob from swnerf_pack_net_x3_kind (swnerf_packed_x3_floats_kind(kind) floats), built from the same
 * tensors plus the fp32 blob of swnerf_pack_net for that kind (its bias tiles are copied).
 * terms: 3 = bf16x3, 1 = plain bf16 (hi halves only; a yardstick, ~37 dB).
 * swnerf_packed_x3_floats / swnerf_pack_net_x3: the SWNERF_NET_CANON forms. */
size_t swnerf_packed_x3_floats_kind(int kind);
int swnerf_pack_net_x3_kind(int kind, const float* const* params /*HOST*/, int L_pos, int L_dir, int L_time,
                            const float* packed_fp32, float* packed_x3, void* stream);
size_t swnerf_packed_x3_floats(void);
int swnerf_pack_net_x3(const float* const* params /*HOST*/, int L_pos, int L_dir, const float* packed_canon,
                       float* packed_x3, void* stream);
int swnerf_render_pass_x3(const swnerf_pass_args* args /*HOST*/, int terms, void* stream);

/* ---- the fused pass under autograd: loss.backward() of the reference's training step --------------------------
 * (nerf/run.py:684-708: render -> img2mse(rgb) + img2mse(rgb0) -> backward -> optimizer.step)
 * Static net (SWNERF_NET_CANON, 11-column ray batch), 2 <= n_samples <= 256.
 *
 * render_pass_train: exactly swnerf_render_pass (same sampling / encoding / MLP / compositing / resampling
 * arithmetic, same outputs) and additionally saves what the backward needs.  Rows of the saved buffers are the
 * (ray, sample) rows PADDED to whole 32-sample tiles per ray: rows = swnerf_train_rows(N, S) = N * ceil(S/32) * 32,
 * row = (ray * ceil(S/32) + s/32) * 32 + s%32.
 *   act  [rows, swnerf_act_floats_per_row()]   post-ReLU activations (as swnerf_mlp_forward_train)
 *   bits [swnerf_mask_floats(rows)]            ReLU bit masks
 *   xs   [rows, swnerf_xs_floats_per_row()]    gamma(x) (64 slots) and gamma(d) (32 slots) in the kernel's operand
 *                                              slot order; swnerf_unslot_grad maps slot columns back
 * args->raw and the depths (args->z_vals given, or args->z_out) are required: the backward recomputes the
 * compositing from them.
 *
 * render_pass_backward: gradients of (rgb_map, disp_map, acc_map) -> d raw [rows,4] (padded rows; zeros past S) and
 * the gradient of every layer's pre-activation grad [rows, act floats] (as swnerf_mlp_backward_dx), one wavefront
 * per ray: compositing backward in the wave's LDS slice, then the dX chain tile by tile.  packed_bwd:
 * swnerf_pack_net_bwd_kind(SWNERF_BWD_CANON).  g_* may each be NULL; g_raw = upstream gradient of the returned raw
 * (retraw=True: the reference's trainers ask for it, nerf/run.py:685) is added to d raw.  z_vals [N,S]: the depths the forward used. */
int64_t swnerf_train_rows(int64_t n_rays, int n_samples);
int swnerf_xs_floats_per_row(void);
int swnerf_render_pass_train(const swnerf_pass_args* args /*HOST*/, float* act, float* bits, float* xs, void* stream);
int swnerf_render_pass_backward(const float* packed_bwd, const float* bits, const float* raw /*[N,S,4]*/,
                                const float* z_vals /*[N,S]*/, const float* ray_batch, int cols, const float* noise,
                                int64_t n_rays, int n_samples, int white_bkgd, const float* g_rgb /*[N,3]*/,
                                const float* g_disp /*[N]*/, const float* g_acc /*[N]*/, const float* g_raw /*[N,S,4] or NULL*/,
                                float* grad, float* d_raw, void* stream);
/* The same pair for the net WITHOUT view directions (SWNERF_NET_NOVIEW; use_viewdirs=False is the reference's argparse
 * default, nerf/run.py:461, and its create_nerf then builds output_ch = 5 when N_importance > 0, nerf/run.py:231):
 * swnerf_render_pass_train takes kind SWNERF_NET_NOVIEW with an 8-column ray batch (raw is [N,S,out_ch]; act holds h0..h7
 * in its first 2048 columns; xs gamma(x) in its first 64 slots), and this backward is its counterpart: packed_bwd =
 * swnerf_pack_net_bwd_noview (pts_linears.7..1 transposed + output_linear.weight), raw / g_raw [N,S,out_ch], and d_raw8
 * [rows, 8] = d raw in columns 0..out_ch-1, zeros behind - the 16-byte aligned A operand of output_linear's weight-
 * gradient GEMM (swnerf_gemm_tn with No = 8).  grad: d pre-activation of pts_linears.0..7 in columns 0..2047. */
size_t swnerf_packed_bwd_noview_floats(void);
int swnerf_pack_net_bwd_noview(const float* const* params /*HOST; as swnerf_pack_net_noview*/, int L_pos, int out_ch,
                               float* packed_bwd, void* stream);
int swnerf_render_pass_backward_noview(const float* packed_bwd, const float* bits, const float* raw /*[N,S,out_ch]*/,
                                       const float* z_vals /*[N,S]*/, const float* ray_batch, int cols, const float* noise,
                                       int64_t n_rays, int n_samples, int white_bkgd, int out_ch, const float* g_rgb /*[N,3]*/,
                                       const float* g_disp /*[N]*/, const float* g_acc /*[N]*/,
                                       const float* g_raw /*[N,S,out_ch] or NULL*/, float* grad, float* d_raw8, void* stream);
/* The same pair for DirectTemporalNeRF at t != 0 (model.py:128-151; the loss of d_nerf/run_dnerf.py:690-725 puts
 * gradients on the image AND on position_delta).  No resampling in the training pass (n_importance must be 0: the
 * one-model configuration's coarse pass is a no_grad inference pass, run_dnerf.py:417-421).  args->dx (position_delta
 * [N,S,3]) and args->raw are required outputs.  *_d: the deformation net's buffers, sized like the canonical ones
 * (act_d uses the first 2048 columns; xs_d = gamma(x) 64 slots + gamma(t) 32 slots).
 * backward: packed_bwd_fused = swnerf_pack_net_bwd_kind(SWNERF_BWD_DNERF_FUSED); dx = the forward's position_delta;
 * g_position_delta [N,S,3] its upstream gradient or NULL; outputs grad / grad_d [rows, act floats], d_raw [rows,4],
 * g_dx [rows,4] = d dx (4th column 0) - the A operand of the `_time_out` weight-gradient GEMM.
 * The backward takes L_pos alone and checks it with cols: L_pos outside 0..10 is SWNERF_E_ARG there ("cols %d / L_pos %d"),
 * not SWNERF_E_UNSUPP as at the entry points that take the bands of a net. */
int swnerf_render_pass_train_dnerf(const swnerf_pass_args* args /*HOST*/, float* act, float* bits, float* xs,
                                   float* act_d, float* bits_d, float* xs_d, void* stream);
int swnerf_render_pass_backward_dnerf(const float* packed_bwd_fused, const float* bits, const float* bits_d, const float* raw,
                                      const float* z_vals, const float* ray_batch, int cols, const float* noise, const float* dx,
                                      const float* g_position_delta, int64_t n_rays, int n_samples, int white_bkgd, int L_pos,
                                      const float* g_rgb, const float* g_disp, const float* g_acc, const float* g_raw,
                                      float* grad, float* grad_d, float* d_raw, float* g_dx, void* stream);
/* Cs [rows_w, nslots] holds weight-gradient columns in slot order (a TN GEMM against xs[:, slot0 : slot0+nslots]):
 * W[o][col0 + column(slot0 + f)] = Cs[o][f] for every real slot f; pad slots are dropped. */
int swnerf_unslot_grad(const float* Cs, int ld_s, int rows_w, int slot0, int nslots, int L_pos, int L_dir,
                       float* W, int ldw, int col0, void* stream);
/* No training pass (fused or op by op) stores `feature` or d feature or runs feature_linear's weight-gradient GEMM
 * (feature_linear has no activation, model.py:50-51; the forward and dX kernels run it folded into the view layer).  From G [128,256] = sum_rows d pre_hv (x) h7 (swnerf_gemm_tn of the
 * gradient rows' view-hidden columns against h7), db_hv [128] (its bias output) and the CURRENT weights this adds
 *   dWv[u][o] += sum_i G[u][i] W_f[o][i] + db_hv[u] b_f[o]      (d views_linears.0.weight[:, :256]; Wv/dWv: [128, ld >= 256])
 *   dW_f[o][i] += sum_u Wv[u][o] G[u][i],   db_f[o] += sum_u Wv[u][o] db_hv[u]      (d feature_linear.weight / .bias)
 *   dW_alpha[i] += a4w[3][i],  db_alpha += a4b[3]      (alpha_linear from the 4-row form: a4w [4,256] = d raw^T . h7, a4b [4]) */
int swnerf_feature_finish(const float* G, const float* db_hv, const float* Wv, int ldwv, const float* W_f, const float* b_f,
                          const float* a4w, const float* a4b, float* dWv, int ld_dwv, float* dW_f, float* db_f,
                          float* dW_alpha, float* db_alpha, void* stream);
/* The five narrow weight-gradient products of the canonical net's fused training pass in ONE pass over M rows (instead of five
 * swnerf_gemm_tn calls that read h7, d pre_hv and the xs rows twice each).  grad / act: the fused pass's gradient and activation
 * rows [M, ld >= 2432] (columns: d pre_0 0..255, d pre_hv 2304..2431; h7 1792..2047, hv 2304..2431), xs [M, 96], d_out [M, 4].
 * Accumulates (+=): c0s [256,64] = d pre_0^T xs[:, :64];  cvs [128,32] = d pre_hv^T xs[:, 64:96];  G [128,256] = d pre_hv^T h7;
 * a4w [4,256] = d_out^T h7;  rgb4 [4,128] = d_out^T hv;  b_l0 [256], b_hv [128], a4b [4], rgb4b [4] = the column sums of d pre_0,
 * d pre_hv and d_out (each may be NULL). */
int swnerf_canon_narrow_grads(const float* grad, int ldg, const float* act, int lda, const float* xs, const float* d_out, int64_t M,
                              float* c0s, float* cvs, float* G, float* a4w, float* rgb4, float* b_l0, float* b_hv, float* a4b,
                              float* rgb4b, void* stream);
/* The same for the deformation net (one launch per chunk; table-driven narrow_plan_kernel, csrc/wgrad_kernels.hip):
 * `_time.0` = [gamma(x) | gamma(t)], `_time_out` (model.py:128-136): grad_d / act_d [M, ld >= 2432] (d pre_0 at
 *   column 0, h7 at 1792), xs_d [M, 96] (gamma(x) slots 0..63, gamma(t) slots 64..95), g_dx [M, 4] = d dx with a zero 4th column:
 *   c0s [256,64] += d pre_0^T xs_d[:, :64], cts [256,32] += d pre_0^T xs_d[:, 64:], w4 [4,256] += g_dx^T h7; b_l0 [256], b4 [4]
 * All operands 16-byte aligned, leading dimensions multiples of 4; outputs accumulate (atomics). */
int swnerf_deform_narrow_grads(const float* grad_d, int ldg, const float* act_d, int lda, const float* xs_d, const float* g_dx, int64_t M,
                               float* c0s, float* cts, float* w4, float* b_l0, float* b4, void* stream);
/* ... for xs_d: slots 64..95 hold gamma(t) (L_time bands) instead of gamma(d); L_time outside 0..10 is one of its bad
 * arguments (SWNERF_E_ARG, the message gives L_time), not SWNERF_E_UNSUPP */
int swnerf_unslot_grad_time(const float* Cs, int ld_s, int rows_w, int nslots, int L_time, float* W, int ldw, int col0, void* stream);

/* ---- the fused T-NeRF pass under autograd (TNeRF, model.py:152-210; the step of t_nerf/run_tnerf.py:646-720) ----------------
 * SWNERF_NET_TNERF, 12-column ray batch, 2 <= n_samples <= 256, no resampling.  swnerf_render_pass_train refuses this kind (its
 * saved buffers are the 8 x 256 nets'); this pair is the T-NeRF counterpart.
 *
 * render_pass_train_tnerf: exactly swnerf_render_pass with kind SWNERF_NET_TNERF (same arithmetic, bit-equal outputs) and
 * additionally saves, per padded row (rows = swnerf_train_rows(N, S), the row rule above):
 *   act [rows, swnerf_tnerf_act_floats_per_row() = 1088]  post-ELU h_l at column 128*l (l = 0..7), the layer_9 hidden at 1024.
 *                                                         ELU' needs y itself (1 for y > 0, y + 1 otherwise), so no bit masks.
 *   xs  [rows, swnerf_tnerf_xs_floats_per_row() = 128]    the encodings in the kernel's operand slot order: gamma(x) slots 0..63,
 *                                                         gamma(t) 64..95, gamma(d) 96..127 (the ray's tiles repeated in every row
 *                                                         of the ray: the weight-gradient GEMMs run over rows)
 * args->raw and the depths (args->z_vals given, or args->z_out) are required.  act, xs and raw 16-byte aligned.
 *
 * pack_net_bwd_tnerf: the transposed stream of the dX chain (params as for swnerf_pack_net(SWNERF_NET_TNERF)): the folded layer_9
 * W9f^T, layers.7 .. layers.1 (layer 5: its h4 columns), density.weight and color.weight rows; swnerf_packed_bwd_tnerf_floats()
 * floats.
 *
 * render_pass_backward_tnerf: gradients of (rgb_map, disp_map, acc_map) and g_raw = the upstream gradient of the returned raw
 * (retraw=True), each NULL or given -> d_raw [rows, 4] = [d(pre-ReLU colour)(3), d sigma] (padded rows; zeros past S; the colour
 * head's ReLU mask comes from raw) and grad [rows, act floats] = d(pre-activation) of every layer in the layout of act.  One
 * wavefront per ray: compositing backward in the wave's LDS slice, then the dX chain tile by tile, the saved activations fetched
 * one layer ahead through LDS.  cols must be 12; z_vals [N,S]: the depths the forward used; noise as in the forward.
 *
 * tnerf_feature_finish: `feature` is folded into layer_9 in both kernels.  From G [64,128] = sum_rows d pre_9 (x) h7, db9 [64] and
 * the CURRENT weights this adds
 *   dW9[u][o] += sum_i G[u][i] Wf[o][i] + db9[u] bf[o]      (d layer_9.weight[:, :128]; W9 / dW9: [64, ld >= 128])
 *   dWf[o][i] += sum_u W9[u][o] G[u][i],   dbf[o] += sum_u W9[u][o] db9[u]      (d feature.weight / .bias)
 *   dW_density[i] += a4w[3][i],  db_density += a4b[3]      (density from the 4-row form: a4w [4,128] = d_raw^T . h7, a4b [4]) */
size_t swnerf_tnerf_act_floats_per_row(void);
size_t swnerf_tnerf_xs_floats_per_row(void);
int swnerf_render_pass_train_tnerf(const swnerf_pass_args* args /*HOST*/, float* act, float* xs, void* stream);
size_t swnerf_packed_bwd_tnerf_floats(void);
int swnerf_pack_net_bwd_tnerf(const float* const* params /*HOST*/, int L_pos, int L_dir, int L_time, float* packed_bwd, void* stream);
int swnerf_render_pass_backward_tnerf(const float* packed_bwd, const float* act, const float* raw /*[N,S,4]*/,
                                      const float* z_vals /*[N,S]*/, const float* ray_batch, int cols, const float* noise,
                                      int64_t n_rays, int n_samples, int white_bkgd, const float* g_rgb /*[N,3]*/,
                                      const float* g_disp /*[N]*/, const float* g_acc /*[N]*/, const float* g_raw /*[N,S,4] or NULL*/,
                                      float* grad, float* d_raw, void* stream);
int swnerf_tnerf_feature_finish(const float* G, const float* db9, const float* W9, int ld9, const float* Wf, const float* bf,
                                const float* a4w, const float* a4b, float* dW9, int ld_dw9, float* dWf, float* dbf,
                                float* dW_density, float* db_density, void* stream);

/* ---- any-shape MLP layers (model.py:10-62, 93-151, 227-296 at shapes the fused kernels are not built for:
 * use_viewdirs=False - the reference's argparse default, utils.py:26-29 / model.py:59-60 -, other D / W / skips) -------
 * linear   : y[M,N] = act(x[M,K] . weight[N,K]^T + bias)   torch.nn.functional.linear (+ relu if relu != 0); bias may be NULL
 * gemm_nn  : c[M,N] = a[M,K] . b[K,N]                       input gradient of a linear layer: dX = dY . weight
 * relu_mask: dy[e] = y[e] > 0 ? dy[e] : 0, in place        relu backward
 * The weight gradient is swnerf_gemm_tn.  Any leading dimensions >= the row length; fp32 MFMA, fp32 accumulate.
 * A NaN at x[r, k] makes exactly row r of y NaN without an activation and under ELU; with relu that row is 0, because fmaxf
 * returns the non-NaN operand (the fused passes' v_max does the same). */
int swnerf_linear(const float* x, int ldx, int64_t M, int K, const float* weight /*[N,K]*/, const float* bias /*[N]*/,
                  int N, int relu, float* y, int ldy, void* stream);
int swnerf_gemm_nn(const float* a, int lda, int64_t M, int K, const float* b, int ldb, int N, float* c, int ldc,
                   void* stream);
int swnerf_relu_mask(float* dy, const float* y, int64_t n, void* stream);
/* swnerf_gemm_tn with a reproducible sum, for any No, Ni up to 65536: every row slice stores its own partial product into
 * ws and the slices are added in slice order (no atomics), and the split depends on (M, No, Ni) alone, so two equal calls give
 * equal bits.  C and bias are accumulated into, as by swnerf_gemm_tn; bias may be NULL.  ws: DEVICE scratch of at least
 * swnerf_gemm_tn_ordered_ws_floats(M, No, Ni) floats (0 for M == 0 or a shape that is not accepted): up to 256 partial
 * products, as many as fit into 16 MiB, at least one. */
size_t swnerf_gemm_tn_ordered_ws_floats(int64_t M, int No, int Ni);
int swnerf_gemm_tn_ordered(const float* A, int lda, int No, const float* B, int ldb, int Ni, int64_t M,
                           float* C, int ldc, float* bias, float* ws, size_t ws_floats, void* stream);

/* The same GEMM with a choice of epilogue, and the ELU backward (TNeRF, model.py:152-210, on the op path):
 * linear_act: y = act(x . weight^T + bias), act = SWNERF_ACT_NONE / SWNERF_ACT_RELU / SWNERF_ACT_ELU (alpha = 1; an
 *             expm1-accurate form, max abs error 1.2e-7 against expm1 on [-20, 0]; the fused T-NeRF pass uses the same one)
 * elu_grad  : dy[e] *= (y[e] > 0 ? 1 : y[e] + 1), in place   ELU backward from its output (elu'(x) = exp(x) = y + 1 for x <= 0) */
#define SWNERF_ACT_NONE 0
#define SWNERF_ACT_RELU 1
#define SWNERF_ACT_ELU  2
int swnerf_linear_act(const float* x, int ldx, int64_t M, int K, const float* weight /*[N,K]*/, const float* bias /*[N]*/,
                      int N, int act, float* y, int ldy, void* stream);
int swnerf_elu_grad(float* dy, const float* y, int64_t n, void* stream);

/* ---- image-quality metrics (nerf/run.py calculate_metrics :49-61 = skimage.metrics PSNR / SSIM; d_nerf/metrics.ipynb
 * MSE / PSNR / SSIM) --------------------------------------------------------------------------------------------------
 * pred, gt: [n, h, w, 3] fp32 HWC RGB.  Per image: mse = mean((pred' - gt)^2) (squared fp32 differences summed in fp64),
 * range = R, psnr = 10 log10(R^2 / mse), ssim = mean of the per-pixel S over every valid window position and the 3 channels
 * (skimage's crop by 3 keeps exactly those pixels), with pred' = clip(pred, 0, 1) when clip_pred != 0.
 *   SWNERF_SSIM_SKIMAGE  uniform 7x7 window, sample covariance (x 49/48)        structural_similarity(win_size=7, channel_axis=2)
 *   SWNERF_SSIM_GAUSS11  11x11 Gaussian (sigma 1.5, normalised), population cov  metrics.ipynb SSIM
 * C1 = (0.01 R)^2, C2 = (0.03 R)^2; R from range_mode:
 *   SWNERF_RANGE_FIXED      fixed_range
 *   SWNERF_RANGE_GT         per image gt.max() - gt.min() (a float32 difference, as in the reference)
 *   SWNERF_RANGE_PRED_RULE  over the whole batch of pred': (max > 128 ? 255 : 1) - (min < -0.5 ? -1 : 0)
 * NaN propagates like np.max / np.mean; R = 0 gives the IEEE values of the formulas.  h or w below the window is
 * SWNERF_E_ARG.  ssim_map (may be NULL): [n, h-win+1, w-win+1, 3] the per-pixel S.  mse / psnr / range / ssim: DEVICE double [n].
 * workspace: DEVICE, swnerf_metrics_workspace_bytes(n, h, w, mode) bytes (0 for arguments the call refuses).
 * Four launches, no host synchronisation, no atomics: bit-identical from run to run. */
#define SWNERF_SSIM_SKIMAGE 0
#define SWNERF_SSIM_GAUSS11 1
#define SWNERF_RANGE_FIXED     0
#define SWNERF_RANGE_GT        1
#define SWNERF_RANGE_PRED_RULE 2
size_t swnerf_metrics_workspace_bytes(int64_t n, int64_t h, int64_t w, int mode);
int swnerf_image_metrics(const float* pred, const float* gt, int64_t n, int64_t h, int64_t w, int mode, int range_mode,
                         double fixed_range, int clip_pred, void* workspace, double* mse, double* psnr, double* range,
                         double* ssim, float* ssim_map /* may be NULL */, void* stream);

/* ---- Laplacian pyramid (multires_dnerf/pyramid.py) ------------------------------------------------------------------
 * Images are [n, h, w, c] fp32 NHWC, contiguous, c in 1..4, sides in 1..2^20; every element offset is 64-bit.  n == 0 is
 * a successful no-op.  One launch each, no workspace, no host synchronisation, no atomics: bit-identical from run to run.
 *   down        dst[n, h/2, w/2, c] = box2x2(blur_k(src)): blur_k is the k x k cross-correlation with zero padding k/2
 *               (weights: DEVICE float [k*k], row-major; k odd, k <= 7), box2x2 the mean of pixels (2i, 2j) .. (2i+1, 2j+1)
 *               = F.interpolate(scale_factor=0.5, bilinear, align_corners=False).  An odd last row / column is dropped by
 *               the box but seen by its neighbours' taps.  h, w >= 2.
 *   up_axpy     out[n, H, W, c] = base + alpha * up(coarse[n, h, w, c]); base may be NULL (out = alpha * up(coarse)).  up is
 *               bilinear with align_corners=False: per axis s = max(scale * (d + 0.5) - 0.5, 0), scale = (float)n_in / n_out,
 *               i0 = floor(s), i1 = min(i0 + 1, n_in - 1), lambda = s - i0, all fp32.  (h, w) == (H, W): exactly
 *               base + alpha * coarse.  out may be base itself.
 *   up_adjoint  g_coarse[n, h, w, c] = the transpose of up applied to g_out[n, H, W, c], gathered in a fixed order. */
int swnerf_pyramid_down(const float* src, int64_t n, int64_t h, int64_t w, int c, const float* weights, int k, float* dst,
                        void* stream);
int swnerf_pyramid_up_axpy(const float* coarse, int64_t n, int64_t h, int64_t w, int c, const float* base /* may be NULL */,
                           float alpha, int64_t H, int64_t W, float* out, void* stream);
int swnerf_pyramid_up_adjoint(const float* g_out, int64_t n, int64_t H, int64_t W, int c, int64_t h, int64_t w,
                              float* g_coarse, void* stream);

/* ---- 2-D image fitting (2d_pos_encoding/: encoding.py, model.py, utils.py) ---------------------------------------------
 * The net: n_layers x (Linear -> ReLU -> BatchNorm1d) at width `hidden`, then Linear(hidden, 3), on encode(pos, L).
 *
 * encode2d (encoding.py:22-40): pos [N, 2] -> out [N, 4L + 2] = [x, y, then per band i: sin(a_i x), sin(a_i y), cos(a_i x),
 *   cos(a_i y)] with (x, y) = 2 * (pos / (max_x, max_y)) - 1 (a correctly rounded fp32 division and two more roundings) and the
 *   argument fl32(2^i pi) * x as ONE fp32 product; sin / cos by a double-precision argument reduction in every band (max abs
 *   error 1.2e-7).  0 <= L <= 23; max_x, max_y > 0 (the reference divides by zero for a 1-pixel-wide picture: SWNERF_E_ARG here).
 *
 * BatchNorm1d on [M, C] fp32 rows, any C >= 1, with an optional ReLU IN FRONT (relu != 0: x = max(a, 0), and the backward
 * masks with a > 0).  Column sums are fp64 in a fixed order without atomics: two equal calls give equal bits.
 *   bn_forward_train  mean and BIASED variance over the M >= 2 rows (M == 1: SWNERF_E_ARG, as torch raises);
 *                     y = gamma (x - mean) invstd + beta, invstd = 1 / sqrt(var + eps); save_mean / save_invstd [C];
 *                     running_mean / running_var (both or neither NULL) updated in place:
 *                     r = (1 - momentum) r + momentum * (mean | var * M / (M - 1)).
 *   bn_backward       dbeta = sum dy, dgamma = sum dy xhat, dx = gamma invstd / M (M dy - dbeta - xhat dgamma), then the ReLU mask.
 *   bn_apply          the eval form y = x s + t, s = gamma / sqrt(running_var + eps), t = beta - running_mean s.
 * ws: DEVICE scratch of bn_workspace_bytes(M, C) bytes (0 up to 512 rows, where one launch does everything; above, the rows
 * are split over the grid and added in a second fixed-order stage), may be NULL when that is 0.
 *
 * fit2d_loss (utils.py:13,56,62-64): out, target [M, 3]; sums (DEVICE double [2]): [0] = mse + reg * mean(max(max(0, x - 1),
 *   max(-x, 0))), [1] = the grey-scale mse (weights 0.2989 / 0.5870 / 0.1140); grad [M, 3] = d sums[0] / d out (may be NULL).
 *   One launch, fp64 sums in a fixed order.  At the ties x == 0 and x == 1 the clip term's subgradient is 0 (torch: a quarter).
 *
 * pack_fit2d: hidden == 256 only.  params: HOST array of 6 n_layers + 2 DEVICE pointers - per hidden layer the Linear weight
 *   [256, in] and bias, the BatchNorm1d weight, bias, running_mean, running_var; then the head's weight [3, 256] and bias.
 *   Every BatchNorm1d is folded into the NEXT Linear: W . diag(s), b + W . t (fp64 product, one rounding; the fold is behind the
 *   ReLU, so the sign of s needs no care).  packed: fit2d_packed_floats(n_layers) floats = (96 + 256 (n_layers - 1) + 16) * 256
 *   + (8 n_layers + 25) * 32; 1 <= n_layers <= 64.  Repack whenever a parameter OR a running buffer changes.
 * fit2d_forward: Model.forward in eval mode on encoded rows x [M, ldx >= 4L + 2] -> out [M, 3].
 * fit2d_picture: get_picture (utils.py:103-126) - pixel (x, y) of an H x W picture is encoded in registers from its index
 *   (max_x = W - 1, max_y = H - 1; H, W >= 2) and run through the net; out_f32 [H, W, 3] = clip(., 0, 1) and / or out_u8
 *   [H, W, 3] = to8b of it (at least one non-NULL).  Nothing is read but the weights.  Both passes: one wave per 32 rows,
 *   one encoder and one trunk, so the same pixel gives the same bits in both. */
int swnerf_encode2d(const float* pos, int64_t N, float max_x, float max_y, int L, float* out, void* stream);
size_t swnerf_bn_workspace_bytes(int64_t M, int C);
int swnerf_bn_forward_train(const float* a, int64_t M, int C, int relu, const float* gamma, const float* beta, double eps,
                            double momentum, float* y, float* save_mean, float* save_invstd, float* running_mean /* may be NULL */,
                            float* running_var /* may be NULL */, void* ws, void* stream);
int swnerf_bn_backward(const float* dy, const float* a, int64_t M, int C, int relu, const float* gamma, const float* save_mean,
                       const float* save_invstd, float* dx, float* dgamma, float* dbeta, void* ws, void* stream);
int swnerf_bn_apply(const float* x, int64_t M, int C, int relu, const float* gamma, const float* beta, const float* running_mean,
                    const float* running_var, double eps, float* y, void* stream);
int swnerf_fit2d_loss(const float* out, const float* target, int64_t M, float reg, double* sums, float* grad /* may be NULL */,
                      void* stream);
size_t swnerf_fit2d_packed_floats(int n_layers);
int swnerf_pack_fit2d(const float* const* params /*HOST*/, int n_layers, int L, double eps, float* packed, void* stream);
int swnerf_fit2d_forward(const float* packed, const float* x, int64_t M, int ldx, int L, int n_layers, float* out, void* stream);
int swnerf_fit2d_picture(const float* packed, int64_t H, int64_t W, int L, int n_layers, float* out_f32 /* may be NULL */,
                         unsigned char* out_u8 /* may be NULL */, void* stream);

/* ---- the data side of a training step (nerf/run.py:598-696, d_nerf/run_dnerf.py:648-683; csrc/batch_kernels.hip) -----------
 * perm_indices: out[i] = perm(key, n, k0 + i), i < count - a keyed bijection of [0, n), 1 <= n < 2^40, any 64-bit key; a batch
 *   drawn without replacement is its image of a run of consecutive k.  A balanced 6-round Feistel network over the smallest even
 *   bit-width covering n with cycle walking; integer arithmetic only, defined by swnerf.batching.perm_index_np.
 *   k0 >= 0, k0 + count <= n (else SWNERF_E_ARG).
 *
 * train_batch: ONE launch, 256 rays per workgroup.  Ray i of the batch is pixel id_i of the domain [0, n_train * h * w):
 *   id_i = perm(key, domain, k0 + i) (k0 + n <= domain), or ids_in[i] when ids_in (DEVICE int64 [n]) is not NULL;
 *   id -> (slot, y, x) = (id / (h w), y0 + (id % (h w)) / w, x0 + id % w) inside the crop window (y0, x0, h, w) of an H x W image;
 *   image = i_train[slot] (DEVICE int64 [n_train], values in [0, n_images)).  The pose is c2w[image] (DEVICE [n_images, 3, 4]), the
 *   ray that of get_rays (fx .. focal_branch as there), the row that of pack_ray_batch: cols = 8 [o d near far], 11 (+ viewdirs,
 *   taken before the NDC warp) or 12 (+ the frame time times[image], DEVICE [n_images], in column 8).  ndc != 0: the warp of
 *   pack_ray_batch at ndc_focal.  target [n, 3] = the pixel of images (DEVICE [n_images, H, W, channels], channels 3 or 4,
 *   float32, or bytes with images_u8 != 0: (float)((double)u / 255.)); with 4 channels and white_bkgd != 0 c * a + (1 - a) in
 *   float32, each operation rounded.  ids_out (DEVICE int64 [n], may be NULL) receives the ids.  An id outside the domain or an
 *   i_train value outside [0, n_images) gives a NaN row and a NaN target and reads nothing.
 *   SWNERF_E_ARG: NULL table, empty window or one outside the image, cols / channels not as above, k0 + n > domain without ids_in.
 *
 * photo_loss: rgb, rgb0 (may be NULL), target [N, 3].  sums (DEVICE double [2]) = sum (rgb - target)^2, sum (rgb0 - target)^2
 *   (0 without rgb0), added in fp64 in a fixed order: equal bits on every run.  losses (DEVICE float [3], may be NULL) =
 *   [mse + mse0, mse, mse0], each formed in fp64 and rounded once.  d_rgb / d_rgb0 (may be NULL) = d losses[0] / d rgb, rgb0 =
 *   2 (x - target) / (3 N), formed in fp64 and rounded once.  One launch. */
int swnerf_perm_indices(uint64_t key, int64_t n, int64_t k0, int64_t count, int64_t* out, void* stream);
int swnerf_train_batch(const void* images, int images_u8, int channels, int64_t n_images, int H, int W,
                       const float* c2w, const float* times /* may be NULL unless cols == 12 */, const int64_t* i_train, int64_t n_train,
                       int y0, int x0, int h, int w, double fx, double fy, double cx, double cy, int focal_branch,
                       double near, double far, int cols, int ndc, double ndc_focal, int white_bkgd,
                       uint64_t key, int64_t k0, int64_t n, const int64_t* ids_in /* may be NULL */,
                       float* ray_batch, float* target, int64_t* ids_out /* may be NULL */, void* stream);
int swnerf_photo_loss(const float* rgb, const float* rgb0 /* may be NULL */, const float* target, int64_t N, double* sums,
                      float* losses /* may be NULL */, float* d_rgb /* may be NULL */, float* d_rgb0 /* may be NULL */, void* stream);

/* ---- the optimizer: one Adam / AdamW step over a list of tensors (csrc/optim_kernels.hip) ---------------------
 * adam_step: tensor i of the list is p[i], g[i], m[i] (exp_avg), v[i] (exp_avg_sq): DEVICE float [n[i]], fp32, dense; the pointer
 *   arrays, n, step, lr and weight_decay are HOST arrays of n_tensors entries.  step[i] >= 1 is tensor i's step count INCLUDING this
 *   update (torch's state['step'] after its increment); the bias corrections are formed from it in double.  In fp32, each operation
 *   rounded, the lines of torch's single-tensor Adam:
 *     g' = g * grad_scale;   decoupled != 0 (AdamW): p = p (1 - lr wd)   else with wd != 0 (L2): g' = g' + wd p
 *     m = m + (g' - m)(1 - beta1);   v = beta2 v + (1 - beta2) g' g'
 *     p = p - (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 *   amsgrad, maximize and capturable are not built.  The list is cut into launches of at most SWNERF_ADAM_MAX_TENSORS tensors and
 *   SWNERF_ADAM_MAX_BLOCKS blocks of SWNERF_ADAM_CHUNK elements each (a launch that one tensor fills alone: up to 16 x that), each
 *   launch described by ONE by-value kernel argument; nothing is copied to the device.  A thread moves 4 floats per 16-byte access
 *   when p, g, m and v of its tensor are all 16-byte aligned, else 1; tails are masked.  n_tensors == 0 and n[i] == 0 launch nothing.
 *   SWNERF_E_ARG before anything touches the device: NULL pointer (of a tensor with n[i] > 0), negative count, n[i] > 2^40, lr,
 *   weight_decay or eps negative or not finite, beta outside [0, 1), step < 1, grad_scale not finite.
 * adam_plan: the same cut without a device, one row per block: launch[r], tensor[r], start[r] (first element), count[r] (elements).
 *   Returns the number of rows (rows beyond `capacity` are counted, not written), or SWNERF_E_ARG.
 * adam_caps: the three constants below and the size of the kernel argument in bytes (each pointer may be NULL). */
#define SWNERF_ADAM_MAX_TENSORS 32
#define SWNERF_ADAM_MAX_BLOCKS  320
#define SWNERF_ADAM_CHUNK       4096
#define SWNERF_ADAM_MAX_ELEMS   ((int64_t)1 << 40)
int swnerf_adam_step(int n_tensors, float* const* p /*HOST*/, const float* const* g /*HOST*/, float* const* m /*HOST*/,
                     float* const* v /*HOST*/, const int64_t* n /*HOST*/, const double* step /*HOST*/, const double* lr /*HOST*/,
                     const double* weight_decay /*HOST*/, double beta1, double beta2, double eps, int decoupled, float grad_scale,
                     void* stream);
int64_t swnerf_adam_plan(int n_tensors, const int64_t* n /*HOST*/, int64_t capacity, int32_t* launch, int32_t* tensor, int64_t* start,
                         int64_t* count);
void swnerf_adam_caps(int* max_tensors, int* max_blocks, int64_t* chunk, size_t* descriptor_bytes);

/* ---- the joint iteration of the MultiRes D-NeRF runner (csrc/patch_kernels.hip, DESIGN.md 6g "Training") ---------------------
 * Both take the levels of the pyramid, finest first, as HOST arrays of n_levels entries (1 <= n_levels <= SWNERF_PATCH_MAX_LEVELS)
 * whose pointer entries are DEVICE pointers; the levels reach the kernel as one by-value argument.  One launch each.
 * patch_batch: for every level l the patch of frame img_i with corner (y, x) = corner[2l], corner[2l+1] and side patch[l], CLIPPED to
 *   the level as a slice is: ph = min(patch[l], H_l - y), pw = min(patch[l], W_l - x), (H_l, W_l) = level_hw[2l], level_hw[2l+1].
 *   ray_batches[l] [ph * pw, 12] = the rows of pack_ray_batch (origin, direction, near, far, times[img_i], unit direction) of the
 *   pixels (y .. y + ph - 1) x (x .. x + pw - 1), row-major, of get_rays(H_l, W_l, focal[l], c2w[img_i]) - the focal branch, the
 *   same device code (csrc/ray_rows.h), bit for bit.  targets[l] [ph, pw, 3] = that window of pyr_images[l] [n_images, H_l, W_l, 3];
 *   full_patch [ph_0, pw_0, 3] = the level-0 window of images [n_images, H_0, W_0, 3].  c2w [n_images, 3, 4], times [n_images].
 *   SWNERF_E_ARG: a corner outside its level, an empty level, a patch side outside 1..4096, img_i outside the table, NULL pointer.
 * multires_loss: level l has rgb[l], targets[l], d_rgb[l] [ph_l * pw_l, 3] (patch_hw[2l], patch_hw[2l+1] = ph_l, pw_l, each
 *   1..SWNERF_PATCH_MAX_SIDE) and optionally rgb0[l] with d_rgb0[l] (rgb0 may be NULL, and so may any entry).
 *   m_l = mean (rgb_l - target_l)^2, m0_l likewise; r = rgb_{L-1}, r = rgb_l + up(r) for l = L-2 .. 0, up = the bilinear upsample of
 *   swnerf_pyramid_up_axpy between the patch sizes (bit for bit that kernel); g = mean (r - full_patch)^2.
 *   losses (DEVICE float [SWNERF_MULTIRES_LOSSES]) = [sum_l (m_l + m0_l) + (add_global ? g : 0), g, 10 log10(1 / g), m_0 .. m_3,
 *   m0_0 .. m0_3] (absent entries 0), sums in fp64 in a fixed order, each value rounded once.  reconstructed [ph_0, pw_0, 3] = r.
 *   d_rgb[l] = 2 (rgb_l - target_l) / (3 ph_l pw_l), formed in fp64 and rounded once, plus, with add_global, (up^T)^l of
 *   2 (r - full_patch) / (3 ph_0 pw_0) (up^T = the gather of swnerf_pyramid_up_adjoint), added in fp32; d_rgb0[l] likewise without
 *   the second term: the gradient of losses[0].  One workgroup, no atomics: equal bits on every run. */
#define SWNERF_PATCH_MAX_LEVELS 4
#define SWNERF_PATCH_MAX_SIDE   32
#define SWNERF_MULTIRES_LOSSES  11
int swnerf_patch_batch(int n_levels, const float* const* pyr_images /*HOST*/, const int* level_hw /*HOST*/, const double* focal /*HOST*/,
                       const int* corner /*HOST*/, const int* patch /*HOST*/, const float* images, int64_t n_images, const float* c2w,
                       const float* times, int64_t img_i, double near, double far, float* const* ray_batches /*HOST*/,
                       float* const* targets /*HOST*/, float* full_patch, void* stream);
int swnerf_multires_loss(int n_levels, const int* patch_hw /*HOST*/, const float* const* rgb /*HOST*/,
                         const float* const* rgb0 /*HOST, may be NULL*/, const float* const* targets /*HOST*/, const float* full_patch,
                         int add_global, float* losses, float* reconstructed, float* const* d_rgb /*HOST*/,
                         float* const* d_rgb0 /*HOST, may be NULL*/, void* stream);

/* ---- dataset images (the loaders under dataloader/: imageio.imread, cv2.resize INTER_AREA; csrc/image_kernels.hip) ---
 * png_unfilter: filtered = DEVICE uint8 [n][H * (1 + W * bpp)], the inflated scanlines of n PNGs of equal size, every row led
 *   by its filter-type byte; out = DEVICE uint8 [n, H, W, bpp], bpp 3 or 4 (else SWNERF_E_ARG).  The five filters of the PNG
 *   specification: a, b, c = the unfiltered bytes to the left, above and above-left, 0 outside the image; Average adds
 *   (a + b) >> 1 of the 9-bit sum, Paeth prefers a, then b, then c on ties; everything mod 256.  status = DEVICE int32 [n]:
 *   0, or 1 + row of the first row of that image whose type byte is above 4 (the rest of that image is then unspecified; the
 *   other images are not affected).  One workgroup per image, rows on a skewed wavefront.  H, W in 1..2^20.
 * area_resize: src [n, H, W, c] uint8 (src_u8 != 0) or float32, c in 1..4 -> dst float32 [n, h, w, c], 1 <= h <= H and
 *   1 <= w <= W (larger is SWNERF_E_ARG).  A byte converts as (float)((double)u / 255.).  dst(i, j) is the area mean that
 *   INTER_AREA defines for down-scaling: source cell (y, x) weighs overlap([i H/h, (i+1) H/h), [y, y+1)) *
 *   overlap([j W/w, (j+1) W/w), [x, x+1)) * h w / (H W); the overlaps are exact integers over h and w, the sum is fp64 and each
 *   output is rounded once.  h | H and w | W: a plain fp64 sum of the block divided by its size (exact for power-of-two
 *   factors); h == H and w == W is the plain conversion. */
int swnerf_png_unfilter(const uint8_t* filtered, int64_t n, int64_t H, int64_t W, int bpp, uint8_t* out, int32_t* status,
                        void* stream);
int swnerf_area_resize(const void* src, int src_u8, int64_t n, int64_t H, int64_t W, int c, int64_t h, int64_t w, float* dst,
                       void* stream);

/* ---- baseline JPEG frames (the LLFF scenes' .JPG camera files, the .jpg pictures of 2d_pos_encoding; imageio.imread ends in libjpeg's default
 * decode, and these entries give its pixels byte for byte; csrc/jpeg_host.h, jpeg_math.h, jpeg_kernels.hip, DESIGN.md 6k "JPEG") ---
 * The host reads markers and the Huffman stream, the device dequantises, inverts the DCT, up-samples chroma and converts colour.
 * Decodable here: 8-bit, Huffman-coded, ONE interleaved scan, 1 component or 3 that libjpeg takes for YCbCr (a JFIF marker; or
 *   an Adobe marker with transform 1; or neither and component ids other than 'R','G','B'), luma sampled 1x1, 2x1 or 2x2 with
 *   chroma 1x1.  Anything else - progressive, arithmetic, 12-bit, 4 components, RGB-coded, other ratios, several scans, a header
 *   that cannot be read - returns SWNERF_E_UNSUPP ("not decodable here", the message says why): the caller hands the file to
 *   another decoder.  A single component is always SWNERF_JPEG_444.
 * jpeg_header (HOST only, no GPU call): data = the file's bytes.  info [SWNERF_JPEG_INFO_LEN] = H, W, components (1 or 3),
 *   sampling (SWNERF_JPEG_*), restart interval in MCUs (0: none), offset of the entropy-coded segment, 0, 0.  qt
 *   [SWNERF_JPEG_QT_LEN] = one 64-entry table per component in natural (row-major, de-zigzagged) order, 8- and 16-bit tables alike.
 * jpeg_coef_count: 64 * the blocks of all components, each plane padded to whole MCUs (MCU = 8 hs x 8 vs pixels); 0 for a
 *   geometry jpeg_decode refuses.
 * jpeg_entropy (HOST only, no GPU call, no global state: safe from several threads): coef [coef_count] int16 = one
 *   [blocks_y][blocks_x][64] plane per component, natural order, every entry written.  Resets the DC predictors at restart
 *   markers and checks their sequence.  SWNERF_E_DATA: the segment is truncated, holds an unassigned code, runs a coefficient
 *   index past 63 or lacks the RSTn it should have (libjpeg's "pad with zeros and warn" is not copied).  Reads nothing past
 *   data + len and writes nothing outside coef; coef_count must be jpeg_coef_count of the file's header (else SWNERF_E_ARG).
 * jpeg_decode: n images of one geometry.  coef = DEVICE int16 [n][jpeg_coef_count] (16-byte aligned), qt = DEVICE uint16
 *   [n][ncomp][64] (16-byte aligned; every image has its own tables), scratch_planes = DEVICE uint8 [n][jpeg_coef_count] (8-byte
 *   aligned; the component planes, overwritten), out = DEVICE uint8 [n, H, W, channels_out], channels_out 3 or 4 (alpha = 255).
 *   coef * q; libjpeg's "islow" inverse DCT (13-bit constants, columns descaled by 11 bits, rows by 18, + 128, clamped); its
 *   "fancy" triangle up-sampling, plain replication when a chroma plane is at most 2 samples wide; its 16-bit fixed-point
 *   YCbCr -> RGB; a single component gives R = G = B.  32-bit arithmetic with unsigned wrap-around: a crafted file gives defined
 *   pixels.  Two launches, no atomics, no host synchronisation; n == 0 is a successful no-op; H, W in 1..65535. */
#define SWNERF_JPEG_444 0
#define SWNERF_JPEG_422 1
#define SWNERF_JPEG_420 2
#define SWNERF_JPEG_INFO_LEN 8
#define SWNERF_JPEG_QT_LEN 192
int     swnerf_jpeg_header(const uint8_t* data /*HOST*/, int64_t len, int32_t* info /*HOST*/, uint16_t* qt /*HOST*/);
int64_t swnerf_jpeg_coef_count(int64_t H, int64_t W, int ncomp, int sampling);
int     swnerf_jpeg_entropy(const uint8_t* data /*HOST*/, int64_t len, int16_t* coef /*HOST*/, int64_t coef_count);
int     swnerf_jpeg_decode(const int16_t* coef, const uint16_t* qt, int64_t n, int64_t H, int64_t W, int ncomp, int sampling,
                           int channels_out, uint8_t* scratch_planes, uint8_t* out, void* stream);

/* ---- baseline JPEG frames of the render videos (the reference's imageio.mimwrite(..., to8b(rgbs), fps=30, quality=8); these entries
 * write what libjpeg's default encoder writes for the same pixels, quality and sampling, byte for byte; csrc/jpeg_enc_math.h,
 * jpeg_enc_host.h, jpeg_enc_kernels.hip, DESIGN.md 6k "JPEG encode") --------------------------------------------------------------
 * The device converts, down-samples, transforms and quantises; the host writes the markers and the Huffman stream.
 * jpeg_quant_tables (HOST only): qt [2][64] natural order = the Annex K.1 (luma) and K.2 (chroma) tables scaled as libjpeg's
 *   jpeg_set_quality does: quality clipped to 1..100, scale = 5000 / quality below 50 and 200 - 2 quality otherwise, each entry
 *   clamp((base * scale + 50) / 100, 1, 255).
 * jpeg_file_bound: an upper bound on the bytes jpeg_write makes of this geometry (every coefficient at its longest code plus
 *   value bits, every byte stuffed); 0 for a geometry jpeg_write refuses.
 * jpeg_write (HOST only, no GPU call, no global state: safe from several threads): coef [coef_count] int16 in the layout of
 *   jpeg_entropy (coef_count = jpeg_coef_count of the geometry, else SWNERF_E_ARG), qt [2][64] natural order with entries 1..255
 *   (the chroma table is read only for 3 components).  Writes SOI, APP0 (JFIF 1.01, density 1 x 1), one DQT per table, SOF0
 *   (components 1, 2, 3; luma hs x vs, chroma 1 x 1), the Annex K.3 Huffman tables as DC0, AC0, DC1, AC1 (one DHT each), SOS, the
 *   interleaved scan (0xFF stuffed, the last byte padded with 1-bits) and EOI: no restart markers, no optimised tables.
 *   Returns the bytes written; SWNERF_E_ARG when they do not fit into `cap` (nothing outside out[0..cap) is written);
 *   SWNERF_E_DATA for a coefficient no baseline code expresses.
 * jpeg_encode: n frames of one size.  frames = DEVICE uint8 (src_u8 != 0) or float32 [n, H, W, channels_in], channels_in 1 (R = G
 *   = B), 3 or 4 (alpha ignored).  A float sample x becomes (uint8)(255.0f * min(max(x', 0), 1)), truncated, NaN -> 0, with
 *   x' = x when divisor == 0 and the correctly rounded x / divisor otherwise (the reference's to8b(disps / np.max(disps))).
 *   qt = DEVICE uint16 [ncomp][64] natural order (16-byte aligned), one set for all frames.  ncomp 3 (YCbCr) or 1 (needs
 *   channels_in 1; SWNERF_JPEG_444).  scratch_planes = DEVICE uint8 [n][jpeg_coef_count] (8-byte aligned; the component planes,
 *   overwritten), coef = DEVICE int16 [n][jpeg_coef_count] (16-byte aligned) in exactly the layout of jpeg_entropy, so
 *   jpeg_decode(jpeg_encode(x)) composes.  libjpeg's RGB -> YCbCr, its 2:1 down-sampling without smoothing, edge replication
 *   (columns before the averaging, rows after it), the "islow" forward DCT and sign(c) ((|c| + 4 q) / (8 q)); a block wholly outside
 *   the component's real blocks has zero ACs and the DC of the block it continues.  Two launches, no atomics, no host
 *   synchronisation; n == 0 is a successful no-op; H, W in 1..65535. */
int     swnerf_jpeg_quant_tables(int quality, uint16_t* qt /*HOST*/);
int64_t swnerf_jpeg_file_bound(int64_t H, int64_t W, int ncomp, int sampling);
int64_t swnerf_jpeg_write(const int16_t* coef /*HOST*/, int64_t coef_count, const uint16_t* qt /*HOST*/, int64_t H, int64_t W, int ncomp,
                          int sampling, uint8_t* out /*HOST*/, int64_t cap);
int     swnerf_jpeg_encode(const void* frames, int src_u8, int64_t n, int64_t H, int64_t W, int channels_in, float divisor,
                           const uint16_t* qt, int ncomp, int sampling, uint8_t* scratch_planes, int16_t* coef, void* stream);

/* ---- LPIPS (nerf/run.py:49-61 lpips.LPIPS(net='alex'); d_nerf/metrics.ipynb lpips.LPIPS(net='vgg'); csrc/lpips_kernels.hip,
 * DESIGN.md 6f "LPIPS") -----------------------------------------------------------------------------------------------
 * Activations are [n, h, w, c] fp32 NHWC, contiguous; sides in 1..2^20, channels in 1..2^20; every element offset is 64-bit.
 * n == 0 is a successful no-op.  No host synchronisation, no atomics: bit-identical from run to run.
 * conv2d_pack: weight = torch's [cout, cin, ksz, ksz] -> packed [ksz * ksz * cin, cout], K in (ky, kx, ci) order: the stream
 *   conv2d_nhwc reads.  Pack once per weight tensor.
 * conv2d_nhwc: out[n, oy, ox, co] = act(bias[co] + sum_{ky,kx,ci} in[n, oy s - p + ky, ox s - p + kx, ci] packed[(ky, kx, ci), co]),
 *   zero padding, out [n, ho, wo, cout] with ho = (h + 2 pad - ksz) / stride + 1 (floor), wo likewise.  An implicit GEMM on the
 *   fp32 MFMA (fp32 operands and accumulation; the k-ordered sum is cut into segments of 128 k), no im2col buffer.  Square
 *   kernels 1..11, stride 1..4, pad 0..5, any cin and cout >= 1, act = SWNERF_ACT_NONE or SWNERF_ACT_RELU (a NaN stays a NaN);
 *   bias may be NULL.  Anything else, or an image with no window, is SWNERF_E_ARG.  16-byte loads along cin when cin % 4 == 0 and
 *   `in` is 16-byte aligned, along cout when cout % 4 == 0 and `packed` is; 4-byte loads otherwise.  One launch.
 * maxpool2d_nhwc: window 2 or 3, stride 2, floor mode, no padding (torchvision's MaxPool2d(2, 2) / (3, 2)):
 *   out [n, (h - window) / 2 + 1, (w - window) / 2 + 1, c].  A NaN in the window gives a NaN, as torch.max_pool2d does.
 * lpips_layer: one tap.  f0, f1 [n, h, w, c], lin [c]: per pixel d = sum_c lin_c (f0_c / (|f0|_2 + 1e-10) - f1_c / (|f1|_2 +
 *   1e-10))^2 in fp32; out (DEVICE double [n]) = the mean of d over the h w pixels, summed in fp64 in a fixed order (block
 *   partials, then one finishing pass); accumulate != 0 adds it to out instead.  map (may be NULL): [n, h, w] the per-pixel d.
 *   workspace: DEVICE, swnerf_lpips_layer_workspace_bytes(n, h, w) bytes (0 for arguments the call refuses).  Two launches. */
int swnerf_conv2d_pack(const float* weight, int cout, int cin, int ksz, float* packed, void* stream);
int swnerf_conv2d_nhwc(const float* in, int64_t n, int64_t h, int64_t w, int cin, const float* packed,
                       const float* bias /* may be NULL */, int cout, int ksz, int stride, int pad, int act, float* out,
                       void* stream);
int swnerf_maxpool2d_nhwc(const float* in, int64_t n, int64_t h, int64_t w, int c, int window, float* out, void* stream);
size_t swnerf_lpips_layer_workspace_bytes(int64_t n, int64_t h, int64_t w);
int swnerf_lpips_layer(const float* f0, const float* f1, const float* lin, int64_t n, int64_t h, int64_t w, int c,
                       int accumulate, void* workspace, double* out, float* map /* may be NULL */, void* stream);

/* ---- square markers (nerf/transform_mesh.py: cv2.aruco's detectMarkers on images_ori/; csrc/marker_math.h, marker_kernels.hip,
 * DESIGN.md 6k "Markers") ---------------------------------------------------------------------------------------------
 * A marker is a 6 x 6 grid of cells: a one-cell black border round a 4 x 4 payload, on a lighter surround (ArUco's 4X4 family).
 * Pixel coordinates: pixel (i, j) covers [j, j + 1) x [i, i + 1), its centre is (j + 0.5, i + 0.5) - cv2's coordinates plus 0.5.
 * frames = DEVICE uint8 [n, H, W, c], c = 1, 3 (RGB) or 4 (alpha ignored); H, W in 1..16384, n in 0..65535 (0: a successful no-op).
 * workspace = DEVICE, 256-byte aligned, swnerf_marker_workspace_bytes(n, H, W) bytes (0 for sizes the calls refuse; about 30 bytes
 *   per pixel).  Nothing is allocated, the host is never synchronised, the launches depend on n, H, W only.  Every stage up to the
 *   coarse corners is integer arithmetic with order-independent integer atomics: the same bits on every run.
 * marker_mask: grey [n, H, W] = (4899 R + 9617 G + 1868 B + 8192) >> 14 (c == 1: a copy); mask [n, H, W] = 1 where
 *   g cnt < s - C cnt, s and cnt the exact sum and pixel count of the (2 radius + 1)^2 window clipped to the image; radius 1..64,
 *   C -255..255.
 * marker_label: mask [n, H, W] (non-zero = dark) -> labels int32 [n, H, W]: -1 on light pixels, else the smallest frame-local linear
 *   index i W + j of the pixel's 8-connected component.  Needs no workspace.
 * marker_candidates: labels exactly as marker_label wrote them -> count [n] = the components of at least min_area (>= 16) pixels,
 *   rows int32 [n, capacity, 11] = the first `capacity` of them in ascending label order: label, area, flags, x0 y0 .. x3 y3.  The
 *   corners are pixel indices, clockwise with y down: P1 (farthest from the centroid rounded to half pixels), the pixel farthest on
 *   the negative side of P1P2, P2 (farthest from P1), the pixel farthest on the positive side; the smallest linear index wins a tie.
 *   Flags: SWNERF_MARKER_BORDER touches the image border, SWNERF_MARKER_ONE_SIDED no pixel on one side of P1P2 (that corner is 0 0),
 *   SWNERF_MARKER_SMALL_QUAD integer quad area below min_area.
 * marker_detect: all stages for each of the nradii (1..4, ascending) radii (HOST array): candidates without flags are refined (24
 *   points per side at t in [0.15, 0.85], mid-level crossing of a bilinear profile along the normal at -4 .. 4 px, contrast >= 40, a
 *   total-least-squares line through >= 8 crossings, corners where adjacent lines meet) and decoded (the 36 cell centres through the
 *   homography, threshold (min + max) / 2, contrast >= 40, all 20 border cells dark).  A survivor whose centre lies within 4 px of
 *   a survivor of a smaller radius is dropped.  count [n] = the markers found, also when that exceeds K; the first K in (radius,
 *   label) order are stored: quads float32 [n, K, 4, 2] (x, y; clockwise with y down) and payload int32 [n, K] = the 16 payload
 *   cells row-major from corner 0 with corner 1 to the right, the first cell in bit 15, white = 1.  Entries past count are not
 *   written. */
#define SWNERF_MARKER_BORDER 1
#define SWNERF_MARKER_ONE_SIDED 2
#define SWNERF_MARKER_SMALL_QUAD 4
#define SWNERF_MARKER_CAND_INTS 11
int64_t swnerf_marker_workspace_bytes(int64_t n, int64_t H, int64_t W);
int     swnerf_marker_mask(const uint8_t* frames, int64_t n, int64_t H, int64_t W, int c, int radius, int C, void* workspace,
                           uint8_t* grey, uint8_t* mask, void* stream);
int     swnerf_marker_label(const uint8_t* mask, int64_t n, int64_t H, int64_t W, int32_t* labels, void* stream);
int     swnerf_marker_candidates(const int32_t* labels, int64_t n, int64_t H, int64_t W, int min_area, void* workspace,
                                 int64_t capacity, int32_t* rows, int32_t* count, void* stream);
int     swnerf_marker_detect(const uint8_t* frames, int64_t n, int64_t H, int64_t W, int c, const int* radii /*HOST*/, int nradii, int C,
                             int min_area, int K, void* workspace, float* quads, int32_t* payload, int32_t* count, void* stream);

/* ---- mesh clean-up and measurement (what a trimesh user does after nerf/extract_mesh.py and nerf/transform_mesh.py: split, smooth,
 * area / volume; csrc/meshops_math.h, meshops_kernels.hip, DESIGN.md 6b "Clean-up and measurement") ------------------------------
 * verts = DEVICE float32 [V,3], faces = DEVICE int32 [F,3] (0-based), contiguous: what swnerf_mc_emit writes.  V = 0 or F = 0 is a
 * successful no-op with empty / zero results.  V >= 2^31 or 3 F >= 2^31 is SWNERF_E_ARG (corner ids 3 f + k are int32).
 * workspace = DEVICE, 256-byte aligned, swnerf_mesh_workspace_bytes of (V, F) bytes (0 for refused sizes; about 12 bytes a vertex
 *   and 4 a face); every call may use the same one.  Nothing is allocated and the host is never synchronised; each phase is its
 *   own launch (no grid-wide barrier, no spin-wait), and all counts come from order-independent integer atomics.
 * A face index outside 0..V-1 is never dereferenced: the first kernel that reads `faces` counts such indices into a status word,
 *   the later kernels of the call see it and write nothing further; the caller reads the word and refuses the mesh.
 * mesh_components: lock-free union-find over the vertices joining (a, b) and (b, c) of every face.  vlabel int32 [V] = the smallest
 *   vertex index of the vertex's component.  table int32 [V,3] (capacity; the first C rows are written) = (label, faces, vertices)
 *   in ascending label order; a face belongs to the label of its first vertex, an unreferenced vertex is a component of 0 faces.
 *   counts int32 [2] = {C, bad indices}.  With bad indices vlabel and table hold nothing meaningful and C = 0.
 * mesh_compact: keep the vertices whose label is in kept (DEVICE int32 [n_kept], ascending) and the faces whose first vertex is;
 *   verts_out [V_out,3] = verts[mask], faces_out [F_out,3] = remap[faces[fmask]], normals / colors (either pair may be NULL) like
 *   verts; the original relative order is kept.  V_out and F_out are the table's sums over the kept rows: rows past them are
 *   never written.
 * mesh_incidence: CSR of the corners at each vertex.  offsets int32 [V+1], items int32 [3F]: vertex v's slice
 *   items[offsets[v] .. offsets[v+1]) holds the corner ids 3 f + k with faces[f][k] == v in ascending order, for any valence
 *   (short slices by insertion, long ones by an in-place heap sort).  A face may repeat an index.  status int32 [1] = bad indices.
 * mesh_smooth_step: one umbrella step, out [V,3] != verts.  For vertex v at p with slice c_1 < .. < c_n, in fp64 without
 *   contraction: S = sum over the slice, in that order, of P[faces[f][(k+1)%3]] then P[faces[f][(k+2)%3]] (f = c / 3, k = c % 3);
 *   out = (float)(p + (double)s * (S / (double)(2 n) - p)); n = 0: out = p.  On a closed manifold every neighbour counts twice
 *   (the uniform umbrella); at a boundary the interior neighbours weigh double.  A pure function of its inputs: the same bits on
 *   every run.  Taubin smoothing alternates s = lambda and s = mu.
 * mesh_vertex_normals: normals [V,3] = the sum over the slice, in order, of the fp64 cross(p1 - p0, p2 - p0) of each incident
 *   face (area weighting), divided by its fp64 length and rounded to float32; a zero or non-finite sum gives (0,0,0).
 * mesh_measure: values double [16] = area (sum of sqrt((cx cx + cy cy) + cz cz) / 2, c = cross(p1 - p0, p2 - p0) in fp64), signed
 *   volume (sum of p0 . cross(p1, p2) / 6), the three first moments (sum of the volume term times (p0 + p1 + p2) / 4), bbox min
 *   [5..7] and max [8..10] over the referenced vertices (exact; +inf / -inf when there is none), the rest 0.  The fp64 sums are
 *   per-workgroup partials over contiguous face ranges added in index order by one workgroup: no float atomics, the same bits on
 *   every run.  counts int64 [8] = referenced vertices, undirected edges E, boundary edges (in exactly one face), non-manifold
 *   edges (in more than two faces, or twice in one direction), components with at least one face, Euler characteristic
 *   V_ref - E + F, closed (no boundary and no non-manifold edge), bad indices.  An edge is counted at the smallest corner id that
 *   carries it, found by scanning the incidence slice of its end point of lower valence. */
int64_t swnerf_mesh_workspace_bytes(int64_t V, int64_t F);
int     swnerf_mesh_components(const int32_t* faces, int64_t V, int64_t F, void* workspace, int32_t* vlabel, int32_t* table,
                               int32_t* counts, void* stream);
int     swnerf_mesh_compact(const float* verts, const int32_t* faces, const float* normals /* may be NULL */,
                            const float* colors /* may be NULL */, const int32_t* vlabel, int64_t V, int64_t F, const int32_t* kept,
                            int64_t n_kept, void* workspace, int64_t V_out, int64_t F_out, float* verts_out, int32_t* faces_out,
                            float* normals_out, float* colors_out, void* stream);
int     swnerf_mesh_incidence(const int32_t* faces, int64_t V, int64_t F, void* workspace, int32_t* offsets, int32_t* items,
                              int32_t* status, void* stream);
int     swnerf_mesh_smooth_step(const float* verts, const int32_t* faces, const int32_t* offsets, const int32_t* items, int64_t V,
                                int64_t F, float s, float* out, void* stream);
int     swnerf_mesh_vertex_normals(const float* verts, const int32_t* faces, const int32_t* offsets, const int32_t* items, int64_t V,
                                   int64_t F, float* normals, void* stream);
int     swnerf_mesh_measure(const float* verts, const int32_t* faces, const int32_t* offsets, const int32_t* items, int64_t V,
                            int64_t F, void* workspace, double* values, int64_t* counts, void* stream);

/* ---- mesh welding and decimation by vertex clustering (trimesh's process=True merge and simplify_*; csrc/meshops_math.h,
 * meshsimp_kernels.hip, DESIGN.md 6b "Welding and decimation") ----------------------------------------------------------------
 * The same conventions as above (nothing allocated, no host synchronisation, one launch per phase, integer atomics only), with a
 * workspace of its own: swnerf_mesh_simplify_workspace_bytes of (V, F) bytes (0 for refused sizes; mesh_cluster needs that of
 * (V, 0)).  It holds an open-addressing table of 64-bit cell keys with a power-of-two capacity of at least 2 V (all ones = empty;
 * a slot is claimed by atomicCAS and takes the atomicMin of its vertex indices; at most `capacity` probes, then counts[2] is set)
 * and the per-label lists.  No result depends on which slot a key landed in: the same bits on every run.
 * Cell of a vertex p for the origin o (float32 [3]) and the cell size h (float32, finite, > 0), in fp64: i_k = floor((p_k - o_k) / h);
 *   valid iff 0 <= i_k < 2^21 on every axis (a NaN or an infinity is not); key = i_x | i_y << 21 | i_z << 42.
 * mesh_cluster: vlabel int32 [V] = the smallest vertex index that shares the vertex's cell (every vertex, referenced or not).
 *   origin = DEVICE float32 [3], or NULL: the per-axis minimum over all V vertices (integer atomicMin on ordered keys).
 *   origin_out float32 [3] = the origin used.  counts int32 [3] = {clusters, invalid vertices, table overflow}.  With an invalid
 *   vertex (or an overflow) vlabel and origin_out are not written.
 * mesh_collapse: g = (vlabel[a], vlabel[b], vlabel[c]) for every face.  A face with two equal entries is degenerate; of the
 *   others, those with the same triple after rotating the smallest label to the front are duplicates (the reversed triple is a
 *   different face) and the smallest face index survives.  fpos int32 [F+1] = exclusive scan of the survivor flags, vmap int32
 *   [V+1] = exclusive scan of "label of a surviving face": element i is in use iff its scan value differs from the next one's,
 *   and that value is its output row.  counts int32 [5] = {V', F', degenerate, duplicate, bad indices}.  A face index (or a label)
 *   outside 0..V-1 is counted and never followed; then vmap and fpos are not written and V' = F' = 0.
 * mesh_collapse_emit: faces_out [F_out,3] = vmap[g] of the surviving faces in input order with their own corner order;
 *   verts_out [V_out,3] (colors_out likewise when colors is given) = one row per label in use, ascending, by `placement`:
 *   SWNERF_MESH_WELD     the rows of vertex l itself, bit for bit; normals_out too when normals is given
 *   SWNERF_MESH_MEAN     per coordinate the fp64 sum over the members of l (all vertices labelled l, ascending) divided by their
 *                        number, rounded once to float32
 *   SWNERF_MESH_QUADRIC  colours as MEAN; the position minimises the sum of squared area-weighted plane distances of every input
 *                        face with a corner labelled l (each once, ascending), regularised by eps times the trace toward the mean
 *                        and solved by adjugate over determinant in fp64, in the term order csrc/meshops_math.h
 *                        (meshops_quadric_point) writes down; the mean instead when the trace or the determinant is not a finite
 *                        positive number, the result is not finite, or it leaves the closed cell of l
 *   MEAN and QUADRIC write no normals (recompute them with mesh_incidence + mesh_vertex_normals on the output).  origin and cell are
 *   those of mesh_cluster; V_out and F_out are counts[0] and counts[1] of mesh_collapse: rows past them are never written.
 *   status int32 [1] = bad indices; nothing else is written then. */
#define SWNERF_MESH_WELD 0
#define SWNERF_MESH_MEAN 1
#define SWNERF_MESH_QUADRIC 2
int64_t swnerf_mesh_simplify_workspace_bytes(int64_t V, int64_t F);
int     swnerf_mesh_cluster(const float* verts, int64_t V, const float* origin /* may be NULL */, float cell, void* workspace,
                            int32_t* vlabel, float* origin_out, int32_t* counts, void* stream);
int     swnerf_mesh_collapse(const int32_t* faces, const int32_t* vlabel, int64_t V, int64_t F, void* workspace, int32_t* vmap,
                             int32_t* fpos, int32_t* counts, void* stream);
int     swnerf_mesh_collapse_emit(const float* verts, const int32_t* faces, const float* normals /* may be NULL */,
                                  const float* colors /* may be NULL */, const int32_t* vlabel, const int32_t* vmap,
                                  const int32_t* fpos, const float* origin, float cell, int64_t V, int64_t F, int placement, double eps,
                                  void* workspace, int64_t V_out, int64_t F_out, float* verts_out, int32_t* faces_out,
                                  float* normals_out, float* colors_out, int32_t* status, void* stream);

/* ---- mesh hole filling: boundary loops and fan caps (trimesh's fill_holes; csrc/meshops_math.h, meshfill_kernels.hip, DESIGN.md 6b
 * "Hole filling"; tests/meshfill_ref.py is the numpy replay) -------------------------------------------------------------------
 * This block was added without a step of SWNERF_VERSION: it only adds entry points, nothing above changes, and the version is
 * what a binding compares against the library it loads, where a missing symbol is an error of its own.
 * The same conventions as above (nothing allocated, no host synchronisation, one launch per phase, integer atomics only, nothing
 * depends on scheduling), with a workspace of its own: swnerf_mesh_fill_workspace_bytes of (V, F) bytes (0 for refused sizes, else
 * a multiple of 256; every phase starts at its first byte).  The inputs are never written.
 * Half-edge c = 3 f + k runs from faces[f][k] (tail) to faces[f][(k+1)%3] (head).  It is a boundary half-edge iff tail != head and
 *   its undirected edge occurs exactly once over all faces: their number is mesh_measure's boundary-edge count (which has no
 *   tail != head clause: it also counts the edge x - x of a face that repeats an index, when that occurs once).
 * A vertex is simple iff exactly one boundary half-edge leaves it and exactly one enters it.  next(c) is the boundary half-edge
 *   leaving head(c), defined iff that head is simple.  A loop is a cycle of next (n >= 3 always); its leader is its smallest
 *   half-edge id, which has rank 0, and ranks follow next; p_r is the tail of the rank-r half-edge.  Boundary half-edges on no
 *   cycle (a bow-tie, a chain through a pinched vertex) are unfillable: counted, never touched.
 * mesh_boundary: builds the corner list of every vertex in the workspace (unsorted: an edge's occurrences are counted from the
 *   shorter list of its two end points, whatever their order) and classifies every half-edge.  bhe int32 [3F] (capacity; the first
 *   nb are written) = the boundary half-edges in ascending order; bnext int32 [3F] likewise = next as an index into bhe, or -1.
 *   counts int32 [2] = {nb, bad indices}.  A face index outside 0..V-1 is counted by the first kernel that reads `faces` and never
 *   followed; then nb = 0 and nothing else is written.  V = 0 or F = 0: counts = {0, 0}.  6 memsets and 11 launches.
 * mesh_boundary_loops: nb = counts[0] of mesh_boundary.  Pointer jumping over bnext between two buffers, one launch per round,
 *   ceil(log2 nb) rounds carrying (jump target, smallest id seen): every element of a cycle ends with its leader, every element of
 *   a chain with "none".  Each cycle is cut in front of its leader and the same rounds run again carrying the distance to the end,
 *   which gives the ranks.  2 ceil(log2 nb) + 16 launches whatever the loops' lengths.  Loops are numbered in ascending leader
 *   order.  table int32 [nb/3, 2] (capacity; L rows written) = (leader, n); loop_offsets int32 [nb/3 + 1] (L + 1 written) and
 *   loop_vertices int32 [nb] (loop_offsets[L] written) = the CSR of p_0 .. p_{n-1} per loop.  A loop is filled iff max_edges == 0
 *   or n <= max_edges (max_edges 0 or >= 3); loop_vnew / loop_fnew int32 [nb/3 + 1] = the exclusive scans of "gets a new vertex"
 *   (filled and n >= 4) and of the new faces (1 for n == 3, else n), so the totals stand at [L].  counts int32 [8] = {L, listed
 *   vertices, filled loops, filled edges, new vertices, new faces, 0, 0}.  nb = 0: counts = 0 and the three [0] entries are 0.
 * mesh_fill_emit: L, M = counts[0], counts[1]; V_out = V + new vertices, F_out = F + new faces.  The first V rows of verts_out
 *   (colors_out when colors is given) and the first F of faces_out are the inputs, bit for bit.  Loop i with a new vertex gets row
 *   V + loop_vnew[i]; its new faces follow from row F + loop_fnew[i] in rank order: n == 3 adds the one face (p_1, p_0, p_2) and no
 *   vertex, n >= 4 the fan (p_{(r+1) % n}, p_r, new vertex) for r = 0 .. n-1.  Every new face holds the reverse of a boundary
 *   half-edge, so the winding continues the surface.  The new vertex is, per coordinate, the fp64 sum of p_0 .. p_{n-1} taken as
 *   partial sums over consecutive runs of 64 ranks (each added in rank order from 0.0), the partial sums added in run order from
 *   0.0, divided by (double)n and rounded once to float32; colours likewise.  The partial sums are one thread each, parallel over
 *   the runs; one thread per loop adds them.  Normals are not written (mesh_incidence + mesh_vertex_normals on the output).
 *   status int32 [1] = entries of loop_vertices outside 0..V-1 (never followed).  Rows past V_out / F_out are never written. */
int64_t swnerf_mesh_fill_workspace_bytes(int64_t V, int64_t F);
int     swnerf_mesh_boundary(const int32_t* faces, int64_t V, int64_t F, void* workspace, int32_t* bhe, int32_t* bnext, int32_t* counts,
                             void* stream);
int     swnerf_mesh_boundary_loops(const int32_t* faces, const int32_t* bhe, const int32_t* bnext, int64_t V, int64_t F, int64_t nb,
                                   int64_t max_edges, void* workspace, int32_t* table, int32_t* loop_offsets, int32_t* loop_vertices,
                                   int32_t* loop_vnew, int32_t* loop_fnew, int32_t* counts, void* stream);
int     swnerf_mesh_fill_emit(const float* verts, const int32_t* faces, const float* colors /* may be NULL */, int64_t V, int64_t F,
                              const int32_t* loop_offsets, const int32_t* loop_vertices, const int32_t* loop_vnew,
                              const int32_t* loop_fnew, int64_t L, int64_t M, void* workspace, int64_t V_out, int64_t F_out,
                              float* verts_out, int32_t* faces_out, float* colors_out, int32_t* status, void* stream);

/* ---- mesh rendering from the project's cameras (what a trimesh user does with mesh.obj in a viewer, and the check of a mesh against
 * the frames and depth maps it was made from; csrc/meshrender_math.h, meshrender_kernels.hip, DESIGN.md 6b "Mesh rendering";
 * tests/meshrender_ref.py is the numpy replay) ------------------------------------------------------------------------------------
 * This block was added without a step of SWNERF_VERSION, like the hole-filling block: it only adds entry points.
 * The same conventions as above (nothing allocated, no host synchronisation, integer atomics only, nothing depends on scheduling,
 * the inputs are never written).  verts / faces as above; normals, colors = DEVICE float32 [V,3]; c2w = DEVICE float32 [N,3,4] as
 * in swnerf_train_batch; H, W, fx, fy, cx, cy, focal_branch as in swnerf_get_rays (NDC cameras are not rendered).  N H W < 2^31.
 * workspace = DEVICE, 8-byte aligned, swnerf_mesh_render_workspace_bytes(N, H, W) bytes: the z-buffer, one 64-bit word per pixel
 *   (0 for refused sizes - a negative N, H or W < 1, N H W >= 2^31 - else a multiple of 256).
 * The ray of pixel (px, py) of view n: d = the float32 rays_d swnerf_get_rays writes for it, bit for bit, o = c2w[n][:, 3], both
 *   widened to fp64.  For the face (v0, v1, v2): A = v0 - o, B = v1 - o, C = v2 - o, E(p, q) = d0 (p1 q2 - p2 q1) + d1 (p2 q0 - p0 q2)
 *   + d2 (p0 q1 - p1 q0) added left to right, U = E(B, C), V = E(C, A), W = E(A, B), det = (U + V) + W.  The ray hits the face iff
 *   det != 0 and U, V, W are all >= 0 or all <= 0.  E(q, p) = -E(p, q) exactly, so the two faces at an edge agree about it: no
 *   pinholes; a ray through an edge or a vertex hits every face around it.  t = ((U (A.d) + V (B.d)) + W (C.d)) / det / (d.d), rounded
 *   once to float32: depth is t along the UNNORMALISED rays_d, the unit of the depth_map of a non-NDC render.  A hit counts iff
 *   t_f is finite and near < t_f <= far (0 <= near < far; far may be +inf).  det < 0 is the outward (counter-clockwise) side; cull:
 *   SWNERF_MESH_CULL_NONE, _BACK (drop det > 0), _FRONT (drop det < 0).  Barycentrics = (U, V, W) / det, each rounded once.
 * A face with an index outside 0..V-1, a repeated index or a coordinate that is not finite is counted and never followed.
 * mesh_render_raster: two memsets (counts, the z-buffer to all ones = empty) and one launch over the (view, face) pairs.  Each
 *   pair's pixel box comes from its projected vertices (camera coordinates through the transpose of the rotation, dz = -z_c,
 *   px = cx + fx x_c / dz, py = cy - fy y_c / dz, widened by a pixel, clamped; the whole image when the face straddles the camera
 *   plane, a vertex is within 2^-12 of it relative to its distance, or the view's rotation is not orthonormal to 2^-20; nothing when
 *   every vertex is behind).  A box of at most 64 pixels is walked by its own lane, a larger one by the 64 lanes of its wave.  Every
 *   hit is one 64-bit atomicMin of (float bits of t_f) << 32 | face id: the nearest wins, the smallest face id on equal depth bits.
 *   counts int64 [4] = {bad faces, (view, face) pairs behind the camera, pairs with a box above 64 pixels, hits}; all 0 for N = 0.
 * mesh_render_resolve: one launch, one thread per pixel: decodes the face, recomputes U, V, W, det, t with the same function (the
 *   depth bits equal the key's) and writes face int32 [N,H,W] (-1 at a miss) and, where the pointer is not NULL, depth [N,H,W] = t_f
 *   (0 at a miss, as the depth_map of an empty ray), disp = 1 / t_f (0), acc = 1 (0), bary [N,H,W,3] (0), rgb [N,H,W,3]
 *   (background, HOST float [3]) by `shading`:
 *   SWNERF_MESH_SHADE_COLORS     the vertex colours by the fp64 barycentrics, clipped to [0, 1], one rounding (needs colors)
 *   SWNERF_MESH_SHADE_NORMALS    the interpolated vertex normal, normalised (0 when it has no direction), as 0.5 n + 0.5 (needs normals)
 *   SWNERF_MESH_SHADE_HEADLIGHT  the clipped colour (0.8 without colors) times |n . d / |d|| (needs normals)
 * mesh_view_compare: acc / depth of a render against a reference.  ref_alpha = DEVICE float32 (alpha_u8 == 0; covered iff > 0.5) or
 *   uint8 (covered iff >= 128), element alpha_stride * pixel + alpha_offset, so the alpha of [N,H,W,4] RGBA frames is read in place
 *   (stride 4, offset 3); NULL: covered iff ref_depth > 0.  The mesh covers a pixel iff acc > 0.5.  counts int64 [N,4] = {intersection,
 *   union, mesh pixels, reference pixels}; sums double [N,3] = {sum |depth - ref_depth|, sum (depth - ref_depth)^2, pixels} over
 *   the pixels covered by both (0 when depth or ref_depth is NULL), in fp64: one workgroup of 1024 per view, lane l adds its terms
 *   of pixels l, l + 1024, .. in order from 0.0, the lane sums fold in halves (s[l] += s[l + w], w = 512 .. 1): the same bits on
 *   every run.  One launch. */
#define SWNERF_MESH_CULL_NONE 0
#define SWNERF_MESH_CULL_BACK 1
#define SWNERF_MESH_CULL_FRONT 2
#define SWNERF_MESH_SHADE_COLORS 0
#define SWNERF_MESH_SHADE_NORMALS 1
#define SWNERF_MESH_SHADE_HEADLIGHT 2
int64_t swnerf_mesh_render_workspace_bytes(int64_t N, int64_t H, int64_t W);
int     swnerf_mesh_render_raster(const float* verts, const int32_t* faces, int64_t V, int64_t F, const float* c2w, int64_t N, int H, int W,
                                  double fx, double fy, double cx, double cy, int focal_branch, float near, float far, int cull,
                                  void* workspace, int64_t* counts, void* stream);
int     swnerf_mesh_render_resolve(const float* verts, const int32_t* faces, const float* normals /* may be NULL */,
                                   const float* colors /* may be NULL */, int64_t V, int64_t F, const float* c2w, int64_t N, int H, int W,
                                   double fx, double fy, double cx, double cy, int focal_branch, int shading,
                                   const float* background /*HOST*/, const void* workspace, float* rgb, float* depth, float* disp,
                                   float* acc, int32_t* face, float* bary, void* stream);
int     swnerf_mesh_view_compare(const float* acc, const float* depth /* may be NULL */, const void* ref_alpha /* may be NULL */,
                                 int alpha_u8, int64_t alpha_stride, int64_t alpha_offset, const float* ref_depth /* may be NULL */,
                                 int64_t N, int64_t H, int64_t W, int64_t* counts, double* sums, void* stream);

#ifdef __cplusplus
}
#endif
#endif
