"""Metric scale from a square marker (nerf/transform_mesh.py): find the marker in the unsegmented photos images_ori/ on the
device (csrc/marker_kernels.hip, DESIGN.md 6k "Markers"), triangulate its four corners from the camera poses, compare the edge
length with the real one, and scale / turn the mesh so that the marker's normal is +z.  The reference does this with cv2.aruco,
scipy.optimize.least_squares and trimesh; none of them is needed here.

Pixel coordinates.  The detector's are continuous: pixel (i, j) covers [j, j + 1) x [i, i + 1), its centre is (j + 0.5, i + 0.5).
cv2 and get_rays put the centre of pixel (i, j) at (j, i).  detect_markers returns the detector's coordinates; triangulate_corners
takes cv2's, so cal_scale subtracts 0.5 in between."""
import ctypes
import json
import os
from collections import Counter

import numpy as np
import torch

from . import _lib
from .mesh import Mesh, load_obj

MIN_AREA_FLOOR = 16
MAX_RADII = 4


# ---- device stages -----------------------------------------------------------------------------------------------------
def _frames(frames):
    if not isinstance(frames, torch.Tensor):
        raise TypeError(f"swnerf.markers: frames must be a torch.Tensor, got {type(frames).__name__}")
    if not frames.is_cuda:
        raise RuntimeError(f"swnerf.markers: frames must live on the GPU (got device {frames.device}); there is no CPU path")
    if frames.dtype != torch.uint8:
        raise TypeError(f"swnerf.markers: frames must be uint8, got {frames.dtype}")
    if frames.dim() == 3:
        frames = frames[..., None]
    if frames.dim() != 4 or frames.shape[-1] not in (1, 3, 4):
        raise ValueError(f"swnerf.markers: frames must be [n,H,W] or [n,H,W,c] with c in (1, 3, 4), got {tuple(frames.shape)}")
    return frames.contiguous()


def workspace_bytes(n, H, W):
    return int(_lib.lib().swnerf_marker_workspace_bytes(int(n), int(H), int(W)))


def _workspace(n, H, W, device, workspace=None):
    need = workspace_bytes(n, H, W)
    if need == 0:
        raise ValueError(f"swnerf.markers: {n} frames of {H} x {W} are outside what the detector takes (sides 1..16384, 1..65535 frames)")
    if workspace is None:
        return torch.empty((need,), dtype=torch.uint8, device=device)
    if workspace.numel() * workspace.element_size() < need:
        raise ValueError(f"swnerf.markers: the workspace holds {workspace.numel() * workspace.element_size()} bytes, {need} are needed")
    return workspace


def dark_mask(frames, radius, C=7):
    """frames: device uint8 [n,H,W,c] -> (grey, mask) uint8 [n,H,W]: the luma and the adaptive-threshold mask of one radius"""
    frames = _frames(frames)
    n, H, W, c = (int(s) for s in frames.shape)
    grey = torch.empty((n, H, W), dtype=torch.uint8, device=frames.device)
    mask = torch.empty_like(grey)
    if n:
        ws = _workspace(n, H, W, frames.device)
        _lib.check(_lib.lib().swnerf_marker_mask(_lib.ptr(frames), n, H, W, c, int(radius), int(C), _lib.ptr(ws), _lib.ptr(grey),
                                                 _lib.ptr(mask), _lib.stream_of(frames)), "marker_mask")
    return grey, mask


def label(mask):
    """mask: device uint8 [n,H,W] -> int32 [n,H,W]: -1 on light pixels, else the smallest linear index of the 8-connected component"""
    mask = _frames(mask)[..., 0].contiguous()
    n, H, W = (int(s) for s in mask.shape)
    labels = torch.empty((n, H, W), dtype=torch.int32, device=mask.device)
    if n:
        _lib.check(_lib.lib().swnerf_marker_label(_lib.ptr(mask), n, H, W, _lib.ptr(labels), _lib.stream_of(mask)), "marker_label")
    return labels


def candidates(labels, min_area=100, capacity=None):
    """labels from label() -> (rows int32 [n,capacity,11], count int32 [n]): label, area, flags, coarse corners of the components
    of at least min_area pixels in ascending label order"""
    n, H, W = (int(s) for s in labels.shape)
    capacity = H * W // MIN_AREA_FLOOR + 1 if capacity is None else int(capacity)
    rows = torch.zeros((n, capacity, _lib.MARKER_CAND_INTS), dtype=torch.int32, device=labels.device)
    count = torch.zeros((n,), dtype=torch.int32, device=labels.device)
    if n:
        ws = _workspace(n, H, W, labels.device)
        _lib.check(_lib.lib().swnerf_marker_candidates(_lib.ptr(labels.contiguous()), n, H, W, int(min_area), _lib.ptr(ws), capacity,
                                                       _lib.ptr(rows), _lib.ptr(count), _lib.stream_of(labels)), "marker_candidates")
    return rows, count


def detect_raw(frames, radii=(11, 41), C=7, min_area=100, max_per_frame=64, out=None, workspace=None):
    """One swnerf_marker_detect call.  -> (quads float32 [n,K,4,2], payload int32 [n,K], count int32 [n]) on the device; count is
    the true number per frame, only the first K = max_per_frame are stored.  out = (quads, payload, count) and workspace may be
    given (tests put guard elements after them)."""
    frames = _frames(frames)
    n, H, W, c = (int(s) for s in frames.shape)
    K = int(max_per_frame)
    radii = [int(r) for r in radii]
    if not 1 <= len(radii) <= MAX_RADII or any(b <= a for a, b in zip(radii, radii[1:])):
        raise ValueError(f"swnerf.markers: 1..{MAX_RADII} ascending radii, got {radii}")
    if out is None:
        out = (torch.zeros((n, K, 4, 2), dtype=torch.float32, device=frames.device),
               torch.full((n, K), -1, dtype=torch.int32, device=frames.device), torch.zeros((n,), dtype=torch.int32, device=frames.device))
    quads, payload, count = out
    if n:
        ws = _workspace(n, H, W, frames.device, workspace)
        arr = (ctypes.c_int * len(radii))(*radii)
        _lib.check(_lib.lib().swnerf_marker_detect(_lib.ptr(frames), n, H, W, c, arr, len(radii), int(C), int(min_area), K, _lib.ptr(ws),
                                                   _lib.ptr(quads), _lib.ptr(payload), _lib.ptr(count), _lib.stream_of(frames)),
                   "marker_detect")
    return quads, payload, count


# ---- payloads ----------------------------------------------------------------------------------------------------------
def payload_bits(payload):
    """16-bit payload -> [4,4] bits, row-major from corner 0, the first cell in bit 15"""
    return np.array([(int(payload) >> (15 - k)) & 1 for k in range(16)], np.int64).reshape(4, 4)


def bits_payload(bits):
    return int(sum(int(b) << (15 - k) for k, b in enumerate(np.asarray(bits).reshape(-1))))


def payload_rotations(payload):
    """the four payloads read from corners 0, 1, 2, 3 of a marker whose payload from corner 0 is `payload`"""
    b = payload_bits(payload)
    return [bits_payload(np.rot90(b, k)) for k in range(4)]


def canonical_payload(payload):
    """-> (id, k): the smallest of the four rotations and the corner it starts from; (None, None) when two rotations tie for it
    (the marker is rotationally symmetric: its corners cannot be told apart)"""
    rots = payload_rotations(payload)
    m = min(rots)
    if rots.count(m) > 1:
        return None, None
    return m, rots.index(m)


def dictionary_table(dictionary):
    """[N,4,4] bits or [N] uint16 -> {payload: index}"""
    d = np.asarray(dictionary)
    if d.ndim == 3 and d.shape[1:] == (4, 4):
        vals = [bits_payload(b) for b in d]
    elif d.ndim == 1:
        vals = [int(v) for v in d]
    else:
        raise ValueError(f"swnerf.markers: a dictionary is [N,4,4] bits or [N] uint16 payloads, got shape {d.shape}")
    table = {}
    for i, v in enumerate(vals):
        table.setdefault(v, i)
    return table


def match_dictionary(payload, table):
    """-> (index, k) of the entry some rotation of the payload equals exactly (k: the corner that is the entry's top-left), or
    (None, None)"""
    for k, v in enumerate(payload_rotations(payload)):
        if v in table:
            return table[v], k
    return None, None


def detect_markers(frames, radii=(11, 41), C=7, min_area=100, max_per_frame=64, dictionary=None, stats=None):
    """frames: device uint8 [n,H,W,c], c in (1, 3, 4) -> one list per frame of (corners float32 [4,2], id).  Corners are in the
    detector's coordinates (module docstring), clockwise with y down, starting from the corner the id is read from.
    Without a dictionary the id is the canonical payload (canonical_payload); a rotationally symmetric marker is skipped.  With
    one, the id is the index of the matching entry and corner 0 its top-left (OpenCV's order); unmatched candidates are dropped.
    stats (a dict, optional) receives the numbers of skipped 'symmetric', 'unmatched' and 'truncated' (beyond max_per_frame)
    markers."""
    quads, payload, count = detect_raw(frames, radii, C, min_area, max_per_frame)
    quads, payload, count = quads.cpu().numpy(), payload.cpu().numpy(), count.cpu().numpy()
    table = None if dictionary is None else dictionary_table(dictionary)
    skipped = {"symmetric": 0, "unmatched": 0, "truncated": 0}
    out = []
    for f in range(len(count)):
        stored = min(int(count[f]), int(max_per_frame))
        skipped["truncated"] += int(count[f]) - stored
        found = []
        for s in range(stored):
            if table is None:
                ident, k = canonical_payload(payload[f, s])
                if ident is None:
                    skipped["symmetric"] += 1
                    continue
            else:
                ident, k = match_dictionary(payload[f, s], table)
                if ident is None:
                    skipped["unmatched"] += 1
                    continue
            found.append((np.roll(quads[f, s], -k, axis=0).astype(np.float32), int(ident)))
        out.append(found)
    if stats is not None:
        stats.update(skipped)
    return out


# ---- geometry (host, float64) --------------------------------------------------------------------------------------------
def undistort_points(points, k1, k2, p1, p2):
    """transform_mesh.py's undistort_points as written: the FORWARD Brown model applied to normalised points [m,2]"""
    p = np.asarray(points, np.float64)
    x, y = p[:, 0], p[:, 1]
    r2 = x * x + y * y
    radial = 1 + k1 * r2 + k2 * r2 * r2
    return np.stack([x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y], 1)


def ray_directions(corners, pose, intrinsics, convention="nerf"):
    """corners [m,2] in cv2 / get_rays coordinates (pixel centres at integers), pose [4,4] -> unit rays [m,3] in the world.
    "reference": transform_mesh.py's get_ray_direction, R [x, y, +1] after undistort_points.  "nerf": get_rays' R [(u - cx) / fx,
    -(v - cy) / fy, -1], no distortion."""
    c = np.asarray(corners, np.float64).reshape(-1, 2)
    T = np.asarray(pose, np.float64)
    x, y = (c[:, 0] - intrinsics["cx"]) / intrinsics["fl_x"], (c[:, 1] - intrinsics["cy"]) / intrinsics["fl_y"]
    if convention == "reference":
        u = undistort_points(np.stack([x, y], 1), *(float(intrinsics.get(k, 0.)) for k in ("k1", "k2", "p1", "p2")))
        d = np.stack([u[:, 0], u[:, 1], np.ones(len(u))], 1)
    elif convention == "nerf":
        d = np.stack([x, -y, -np.ones(len(x))], 1)
    else:
        raise ValueError(f"swnerf.markers: convention must be 'nerf' or 'reference', got {convention!r}")
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return d @ T[:3, :3].T


def camera_centre(pose, convention="nerf"):
    """"nerf": T[:3,3] (a camera-to-world matrix).  "reference": -R^T t, as calculate_3d_corners writes it (the centre of a
    world-to-camera matrix, though its rays use R as camera-to-world: the two conventions are not equivalent)."""
    T = np.asarray(pose, np.float64)
    if convention == "reference":
        return -T[:3, :3].T @ T[:3, 3]
    if convention == "nerf":
        return T[:3, 3].copy()
    raise ValueError(f"swnerf.markers: convention must be 'nerf' or 'reference', got {convention!r}")


def triangulate_point(rays, centres):
    """the point minimising sum |(I - d d^T)(p - c)|^2 over unit rays d [m,3] from centres c [m,3]: one 3x3 solve"""
    d = np.asarray(rays, np.float64)
    c = np.asarray(centres, np.float64)
    P = np.eye(3)[None] - d[:, :, None] * d[:, None, :]
    return np.linalg.solve(P.sum(0), np.einsum("mij,mj->i", P, c))


def triangulate_corners(corners_per_frame, poses, intrinsics, convention="nerf"):
    """corners_per_frame [m,4,2] (cv2 / get_rays coordinates), poses [m,4,4] from transforms.json, intrinsics: a dict with fl_x,
    fl_y, cx, cy (and k1, k2, p1, p2 for "reference") -> the four corners in the world [4,3].  The closed form of
    transform_mesh.py's triangulate_point, which runs least_squares on the same point-to-ray distances."""
    corners = np.asarray(corners_per_frame, np.float64).reshape(-1, 4, 2)
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    if len(corners) != len(poses) or len(poses) < 2:
        raise ValueError(f"swnerf.markers.triangulate_corners: {len(corners)} corner sets and {len(poses)} poses; at least 2 views are needed")
    rays = np.stack([ray_directions(c, T, intrinsics, convention) for c, T in zip(corners, poses)])     # [m,4,3]
    centres = np.stack([camera_centre(T, convention) for T in poses])
    return np.stack([triangulate_point(rays[:, i], centres) for i in range(4)])


def calculate_transform_matrix(corner_positions):
    """[4,4] rotation taking the marker's normal n = (c1 - c0) x (c2 - c0), normalised, to +z: Rodrigues' I + K + K^2 (1 - c) / s^2
    with v = n x z, c = n . z, s = |v|, K = [v]_x, as transform_mesh.py writes it.  Where s = 0 the reference divides by zero:
    here n = +z gives the identity and n = -z the half turn about x, diag(1, -1, -1)."""
    p = np.asarray(corner_positions, np.float64)
    n = np.cross(p[1] - p[0], p[2] - p[0])
    n = n / np.linalg.norm(n)
    v = np.cross(n, [0., 0., 1.])
    c, s = float(n[2]), float(np.linalg.norm(v))
    M = np.eye(4)
    if s < 1e-12:
        if c < 0:
            M[1, 1] = M[2, 2] = -1.
        return M
    K = np.array([[0., -v[2], v[1]], [v[2], 0., -v[0]], [-v[1], v[0], 0.]])
    M[:3, :3] = np.eye(3) + K + K @ K * ((1 - c) / (s * s))
    return M


def mean_edge_length(corner_positions):
    p = np.asarray(corner_positions, np.float64)
    return float(np.mean([np.linalg.norm(p[i] - p[(i + 1) % 4]) for i in range(4)]))


# ---- the flow ----------------------------------------------------------------------------------------------------------
def _intrinsics(meta, H, W):
    out = {k: float(meta[k]) for k in ("fl_x", "fl_y", "cx", "cy", "k1", "k2", "p1", "p2") if k in meta}
    if "fl_x" not in out:
        if "camera_angle_x" not in meta:
            raise ValueError("swnerf.markers.cal_scale: transforms.json holds neither fl_x nor camera_angle_x")
        out["fl_x"] = 0.5 * W / np.tan(0.5 * float(meta["camera_angle_x"]))
    out.setdefault("fl_y", out["fl_x"])
    out.setdefault("cx", 0.5 * W)
    out.setdefault("cy", 0.5 * H)
    return out


def _photo(datadir, file_path):
    p = os.path.join(datadir, file_path.replace("images/", "images_ori/"))
    for cand in (p, p + ".png", p + ".jpg", p + ".JPG"):
        if os.path.isfile(cand):
            return cand
    return None


def cal_scale(datadir, actual_size, convention="nerf", radii=(11, 41), C=7, min_area=100, max_per_frame=64, dictionary=None,
              device=None, budget_bytes=2 << 30, verbose=True):
    """transform_mesh.py's cal_scale: read datadir/transforms.json, take each frame's photo from images_ori/ instead of images/,
    detect markers on the device (the photos are loaded and searched in chunks of at most budget_bytes of frames + workspace),
    keep the most common id, triangulate its corners, -> (actual_size / mean edge length, calculate_transform_matrix(corners)).
    No window is opened.  convention: see triangulate_corners; "nerf" is the frame extract_mesh's mesh lives in."""
    from . import images
    with open(os.path.join(datadir, "transforms.json")) as fh:
        meta = json.load(fh)
    frames, paths = [], []
    for fr in meta["frames"]:
        p = _photo(datadir, fr["file_path"])
        if p is None:
            if verbose:
                print(f"Failed to load image for {fr['file_path']}")
            continue
        frames.append(fr)
        paths.append(p)
    if not paths:
        raise FileNotFoundError(f"swnerf.markers.cal_scale: none of the {len(meta['frames'])} photos exists under {datadir}")
    H, W = images.image_size(paths[0])[:2]
    per = max(1, int(budget_bytes // (workspace_bytes(1, H, W) + H * W * 4)))
    info = []
    for i in range(0, len(paths), per):
        batch = images.load_pngs(paths[i:i + per], device=device)
        for fr, found in zip(frames[i:i + per], detect_markers(batch, radii, C, min_area, max_per_frame, dictionary)):
            info += [(fr, ident, corners) for corners, ident in found]
        del batch
    if not info:
        raise RuntimeError(f"swnerf.markers.cal_scale: no marker found in {len(paths)} photos")
    best = Counter(ident for _, ident, _ in info).most_common(1)[0][0]
    keep = [(fr, c) for fr, ident, c in info if ident == best]
    if verbose:
        print(f"find ID: {best}, in total {len(keep)} frames")
    corners = np.stack([c.astype(np.float64) - 0.5 for _, c in keep])                  # detector -> cv2 / get_rays coordinates
    poses = np.stack([np.asarray(fr["transform_matrix"], np.float64) for fr, _ in keep])
    world = triangulate_corners(corners, poses, _intrinsics(meta, H, W), convention)
    return float(actual_size) / mean_edge_length(world), calculate_transform_matrix(world)


def transform_mesh(input_obj, output_obj, scale, transform_matrix):
    """transform_mesh.py's transform_mesh on swnerf.mesh: input_obj is an OBJ path or a Mesh; vertices become (v * scale) . M^T (with
    the translation of M), normals are turned by M[:3,:3], faces and colours are kept.  Writes output_obj (unless None) and
    returns the Mesh."""
    if isinstance(input_obj, Mesh):
        v, f, vn, col = input_obj.vertices, input_obj.faces, input_obj.vertex_normals, input_obj.vertex_colors
    else:
        v, f, vn, col = load_obj(input_obj)
    M = np.asarray(transform_matrix, np.float64).reshape(4, 4)
    v = np.asarray(v, np.float64).reshape(-1, 3) * float(scale)
    v = (np.concatenate([v, np.ones((len(v), 1))], 1) @ M.T)[:, :3]
    vn = np.asarray(vn, np.float64).reshape(-1, 3) @ M[:3, :3].T
    out = Mesh(v.astype(np.float32), f, vn.astype(np.float32), col)
    if output_obj is not None:
        out.export(output_obj)
    return out
