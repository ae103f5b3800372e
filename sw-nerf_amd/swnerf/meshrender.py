"""A mesh seen from the project's own cameras, on the device (DESIGN.md 6b "Mesh rendering"; swnerf_mesh_render_* and
swnerf_mesh_view_compare of include/swnerf.h; csrc/meshrender_math.h, meshrender_kernels.hip); `swnerf.mesh` re-exports every name here.

  render_views(m, H, W, K, poses, ...)   colour, depth, disparity, coverage, face id and barycentrics per pixel of every pose
  render_views_arrays(verts, faces, ...) the same on device arrays
  compare_views(out, alpha, depth)       silhouette IoU and depth error of such a render against reference alpha / depth maps

The ray of a pixel is get_rays' (H, W, K or a float focal, c2w), and depth is t along the unnormalised rays_d: the unit of the
depth_map of a non-NDC render, so the two subtract directly.  A ray hits a face by exact-sign edge functions in fp64 - the two faces
at an edge agree about it, so a closed mesh has no pinholes - and the nearest hit wins through a 64-bit integer atomicMin, the smallest
face id on equal depth: the same bits on every run.  Every refusal below is a ValueError raised before any GPU work."""
import ctypes

import numpy as np
import torch

from . import _lib
from . import meshops

SHADINGS = {"colors": 0, "normals": 1, "headlight": 2}              # SWNERF_MESH_SHADE_*
CULLS = {None: 0, "none": 0, "back": 1, "front": 2}                 # SWNERF_MESH_CULL_*
OUTPUTS = ("rgb", "depth", "disp", "acc", "face", "bary")
COUNT_KEYS = ("bad_faces", "pairs_behind", "pairs_wide", "hits")


def _intrinsics(K, focal=None):
    """-> (fx, fy, cx, cy, focal_branch) as swnerf_get_rays takes them: K = None with a float focal, or a float in K's place, is the
    focal branch (centre W / 2, H / 2); else the [3,3] pinhole matrix"""
    if K is None:
        K = focal
    if isinstance(K, (float, int, np.floating, np.integer)) and not isinstance(K, bool):
        f = float(K)
        if not (np.isfinite(f) and f > 0):
            raise ValueError(f"swnerf.mesh.render_views: the focal length must be finite and positive, got {K!r}")
        return f, f, 0., 0., 1
    try:
        M = np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K, np.float64)
    except (TypeError, ValueError):
        M = None
    if M is None or M.shape != (3, 3):
        raise ValueError("swnerf.mesh.render_views: K must be a [3,3] pinhole matrix, or None with a float focal")
    return float(M[0, 0]), float(M[1, 1]), float(M[0, 2]), float(M[1, 2]), 0


def _check_view(H, W, shading, near, far, cull, outputs):
    for name, x in (("H", H), ("W", W)):
        if not (isinstance(x, (int, np.integer)) and not isinstance(x, bool) and x >= 1):
            raise ValueError(f"swnerf.mesh.render_views: {name} must be a positive integer, got {x!r}")
    if not isinstance(shading, str) or shading not in SHADINGS:
        raise ValueError(f"swnerf.mesh.render_views: unknown shading {shading!r} (one of {sorted(SHADINGS)})")
    if not (cull is None or isinstance(cull, str)) or cull not in CULLS:
        raise ValueError(f"swnerf.mesh.render_views: unknown cull {cull!r} (None, 'back' or 'front')")
    try:
        near, far = float(np.float32(near)), float(np.float32(far))
    except (TypeError, ValueError):
        raise ValueError(f"swnerf.mesh.render_views: near and far must be numbers, got {near!r}, {far!r}") from None
    if not near >= 0:
        raise ValueError(f"swnerf.mesh.render_views: near must be >= 0, got {near!r}")
    if not far > near:
        raise ValueError(f"swnerf.mesh.render_views: far must be above near, got near = {near!r}, far = {far!r}")
    outputs = tuple(outputs)
    extra = [o for o in outputs if o not in OUTPUTS]
    if extra:
        raise ValueError(f"swnerf.mesh.render_views: unknown output(s) {extra} (of {list(OUTPUTS)})")
    return near, far, outputs


def _poses_shape(poses):
    shape = tuple(poses.shape) if hasattr(poses, "shape") else np.asarray(poses).shape
    if len(shape) != 3 or shape[1:] not in ((3, 4), (4, 4)):
        raise ValueError(f"swnerf.mesh.render_views: poses must be [N,3,4] or [N,4,4], got {shape}")
    return shape


def _poses(poses, device):
    """-> contiguous float32 [N,3,4] on the device"""
    if isinstance(poses, torch.Tensor):
        p = poses.detach()
        if not p.dtype.is_floating_point:
            raise ValueError(f"swnerf.mesh.render_views: poses must be floating point, got {p.dtype}")
    else:
        p = torch.from_numpy(np.ascontiguousarray(np.asarray(poses), np.float32))
    return p[:, :3, :4].to(device, torch.float32).contiguous()


def _background(white_bkgd, background):
    if background is None:
        return (1., 1., 1.) if white_bkgd else (0., 0., 0.)
    try:
        b = tuple(float(np.float32(x)) for x in np.asarray(background, np.float64).reshape(-1))
    except (TypeError, ValueError):
        b = ()
    if len(b) != 3:
        raise ValueError(f"swnerf.mesh.render_views: background must be three numbers, got {background!r}")
    return b


def _check_pixels(N, H, W):
    if N * H * W >= 2 ** 31:
        raise ValueError(f"swnerf.mesh.render_views: {N} views of {H} x {W} pixels: one call renders fewer than 2^31 pixels")


def render_views_arrays(verts, faces, H, W, K, poses, normals=None, colors=None, shading="colors", near=0., far=float("inf"), cull=None,
                        white_bkgd=False, background=None, outputs=OUTPUTS, focal=None):
    """render_views() on device arrays: verts [V,3], faces [F,3] and, where the shading reads them, normals / colors [V,3] -> the
    same dict.  Nothing here synchronises with the host; `counts` stays a device tensor (int64 [4]: bad faces, (view, face) pairs
    behind the camera, pairs whose pixel box went to the wave tier, hits)."""
    near, far, outputs = _check_view(H, W, shading, near, far, cull, outputs)
    fx, fy, cx, cy, fb = _intrinsics(K, focal)
    N = _poses_shape(poses)[0]
    H, W = int(H), int(W)
    _check_pixels(N, H, W)
    bg = _background(white_bkgd, background)
    want_rgb = "rgb" in outputs
    if want_rgb and shading == "colors" and colors is None:
        raise ValueError("swnerf.mesh.render_views: shading='colors' needs vertex colours (the mesh has none)")
    v = meshops._rows3(verts, "verts")
    f = meshops._faces(faces, v.device).to(v.device)
    V, F, dev = v.shape[0], f.shape[0], v.device
    meshops._sizes(V, F)
    col = None if colors is None or not want_rgb or shading == "normals" else meshops._rows3(colors, "colors", like=v)
    nor = None
    if want_rgb and shading != "colors":
        nor = meshops.vertex_normals(v, f) if normals is None or len(normals) != V else meshops._rows3(normals, "normals", like=v)
    c2w = _poses(poses, dev)
    L, st = _lib.lib(), _lib.stream_of(v)
    ws = torch.empty(int(L.swnerf_mesh_render_workspace_bytes(N, H, W)), dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    _lib.check(L.swnerf_mesh_render_raster(_lib.ptr(v), _lib.ptr(f), V, F, _lib.ptr(c2w), N, H, W, fx, fy, cx, cy, fb, near, far, CULLS[cull],
                                           _lib.ptr(ws), _lib.ptr(counts), st), "mesh_render_raster")
    new = lambda *tail, dtype=torch.float32: torch.empty((N, H, W) + tail, dtype=dtype, device=dev)
    out = {"face": new(dtype=torch.int32)}
    for name in ("depth", "disp", "acc"):
        out[name] = new() if name in outputs else None
    out["bary"] = new(3) if "bary" in outputs else None
    out["rgb"] = new(3) if want_rgb else None
    _lib.check(L.swnerf_mesh_render_resolve(_lib.ptr(v), _lib.ptr(f), _lib.ptr(nor), _lib.ptr(col), V, F, _lib.ptr(c2w), N, H, W, fx, fy, cx, cy, fb,
                                            SHADINGS[shading], (ctypes.c_float * 3)(*bg), _lib.ptr(ws), _lib.ptr(out["rgb"]), _lib.ptr(out["depth"]),
                                            _lib.ptr(out["disp"]), _lib.ptr(out["acc"]), _lib.ptr(out["face"]), _lib.ptr(out["bary"]), st),
               "mesh_render_resolve")
    out = {k: t for k, t in out.items() if t is not None and k in outputs}
    out["counts"] = counts
    return out


def _mesh_rows(m, faces):
    """The mesh argument opened on the host, so that a refusal that depends on it (colours) needs no GPU"""
    raw = meshops._raw(m, faces)
    if faces is not None:
        return raw, faces, None, None
    if not (isinstance(raw, (tuple, list)) and len(raw) in (2, 4)):
        raise TypeError("swnerf.mesh: expected a Mesh, (verts, faces, normals, colors), an OBJ path, or verts and faces")
    return (raw[0], raw[1]) + ((raw[2], raw[3]) if len(raw) == 4 else (None, None))


def render_views(m, H, W, K, poses, faces=None, shading="colors", near=0., far=float("inf"), cull=None, white_bkgd=False, background=None,
                 outputs=OUTPUTS, focal=None):
    """Render a mesh from camera poses -> dict of device tensors: rgb [N,H,W,3], depth, disp, acc [N,H,W] float32, face int32 [N,H,W]
    (-1 where no face is hit), bary [N,H,W,3] - those named in `outputs` - and counts (int64 [4], see render_views_arrays).
    m: a Mesh, the tuple of marching_cubes, an OBJ path, or a vertex array with `faces`.  H, W, K and poses ([N,3,4] or [N,4,4], numpy
    or tensor) are get_rays' arguments; K = None with a float `focal` (or a float in K's place) is its focal branch.  A miss has depth,
    disp, acc 0 (an empty ray of the NeRF's maps) and the background colour (white_bkgd, or `background`).
    shading: 'colors' (vertex colours by the barycentrics; needs colours), 'normals' (0.5 n + 0.5 of the interpolated vertex normal),
    'headlight' (the colour, or 0.8 grey, times |n . view direction|).  near / far: only hits with near < depth <= far count (a
    clipping window in the depth's unit).  cull: None, 'back' (drop faces seen from inside) or 'front'."""
    _check_view(H, W, shading, near, far, cull, outputs)
    _intrinsics(K, focal)
    _check_pixels(_poses_shape(poses)[0], int(H), int(W))
    _background(white_bkgd, background)
    v, f, n, c = _mesh_rows(m, faces)
    if "rgb" in tuple(outputs) and shading == "colors" and c is None:
        raise ValueError("swnerf.mesh.render_views: shading='colors' needs vertex colours (the mesh has none)")
    return render_views_arrays(v, f, H, W, K, poses, n, c, shading, near, far, cull, white_bkgd, background, outputs, focal)


def _map(t, name, like=None):
    """a [N,H,W] map (or [N,H,W,C] frames) as a device tensor"""
    if not isinstance(t, torch.Tensor):
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(t)))
    if like is not None:
        t = t.to(like.device)
    return t


def compare_views(out, alpha=None, depth=None, alpha_channel=-1):
    """A render against reference maps -> dict of per-view numpy arrays: iou (intersection / union of the silhouettes; nan where both are
    empty), depth_mae and depth_rmse over the pixels both cover (nan where there is none, or without a depth on either side), and
    the raw counts: intersection, union, mesh_pixels, ref_pixels, depth_pixels, abs_sum, sq_sum.
    out: the dict of render_views (acc, and depth for the depth error).  alpha: [N,H,W] float (covered above 0.5) or uint8 (from 128),
    or frames [N,H,W,C] whose channel `alpha_channel` (the last by default) is read in place - the RGBA frames the loaders keep on
    the device.  depth: [N,H,W] float32 in the unit of the render's depth (a NeRF's depth_map); without an alpha the reference
    covers where it is above 0."""
    if alpha is None and depth is None:
        raise ValueError("swnerf.mesh.compare_views: needs a reference alpha or a reference depth")
    if not isinstance(out, dict) or out.get("acc") is None:
        raise ValueError("swnerf.mesh.compare_views: `out` must be a render_views dict with 'acc'")
    acc = out["acc"]
    shape = tuple(acc.shape)
    if len(shape) != 3:
        raise ValueError(f"swnerf.mesh.compare_views: acc must be [N,H,W], got {shape}")
    stride, offset, u8 = 1, 0, 0
    if alpha is not None:
        ashape = tuple(alpha.shape) if hasattr(alpha, "shape") else np.asarray(alpha).shape
        if ashape[:3] != shape or len(ashape) not in (3, 4):
            raise ValueError(f"swnerf.mesh.compare_views: alpha {ashape} does not match the render {shape}")
        if len(ashape) == 4:
            stride = ashape[3]
            if not -stride <= alpha_channel < stride:
                raise ValueError(f"swnerf.mesh.compare_views: alpha_channel {alpha_channel} of {stride} channels")
            offset = alpha_channel % stride
    if depth is not None:
        dshape = tuple(depth.shape) if hasattr(depth, "shape") else np.asarray(depth).shape
        if dshape != shape:
            raise ValueError(f"swnerf.mesh.compare_views: depth {dshape} does not match the render {shape}")
    acc = _lib.dev_f32(acc, "acc")
    dev = acc.device
    mine = out.get("depth")
    mine = None if mine is None or depth is None else _lib.dev_f32(mine, "depth")
    if alpha is not None:
        alpha = _map(alpha, "alpha", acc)
        u8 = int(alpha.dtype == torch.uint8)
        alpha = alpha.contiguous() if u8 else alpha.to(torch.float32).contiguous()
    ref = None if depth is None else _map(depth, "depth", acc).to(torch.float32).contiguous()
    N, H, W = shape
    counts = torch.zeros((N, 4), dtype=torch.int64, device=dev)
    sums = torch.zeros((N, 3), dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().swnerf_mesh_view_compare(_lib.ptr(acc), _lib.ptr(mine), _lib.ptr(alpha), u8, stride, offset, _lib.ptr(ref), N, H, W,
                                                   _lib.ptr(counts), _lib.ptr(sums), _lib.stream_of(acc)), "mesh_view_compare")
    c, s = counts.cpu().numpy(), sums.cpu().numpy()
    with np.errstate(all="ignore"):
        iou = np.where(c[:, 1] > 0, c[:, 0] / np.maximum(c[:, 1], 1), np.nan)
        have = (s[:, 2] > 0) & (mine is not None)
        mae = np.where(have, s[:, 0] / np.maximum(s[:, 2], 1), np.nan)
        rmse = np.where(have, np.sqrt(s[:, 1] / np.maximum(s[:, 2], 1)), np.nan)
    return dict(iou=iou, depth_mae=mae, depth_rmse=rmse, intersection=c[:, 0].copy(), union=c[:, 1].copy(), mesh_pixels=c[:, 2].copy(),
                ref_pixels=c[:, 3].copy(), depth_pixels=s[:, 2].astype(np.int64), abs_sum=s[:, 0].copy(), sq_sum=s[:, 1].copy())
