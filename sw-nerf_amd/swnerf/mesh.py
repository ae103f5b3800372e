"""Dense-grid network query for mesh extraction: the GPU side of
nerf/extract_mesh.py (`generate_viewdirs` :7-24, `sample_grid` :27-90) and of the 2-D form of
`network_query_fn` it uses (nerf/load_model.py:56-74), and the second half of that tool (`generate_mesh`, `nerf_to_mesh`
:92-145):
`marching_cubes` / `generate_mesh` / `nerf_to_mesh` (:92-145): the iso-surface on the GPU (swnerf_mc_count / swnerf_mc_emit) and
an OBJ writer, in place of skimage.measure.marching_cubes and trimesh.

`swnerf_query_points` evaluates the positional encodings in registers and - for V view
directions shared by every grid point - the 8-layer trunk and the density ONCE per point and
only the view branch V times: 8832 + 640 V MFMAs per 32 points instead of 9472 V.
`swnerf_query_points_time` does the same for the two time-conditioned nets at one frame time (`frame_time=`):
DirectTemporalNeRF (deformation net, gamma(x + dx), canonical trunk once per point; d_nerf/run_dnerf.py:46-83) and TNeRF
(t_nerf/run_tnerf.py:48-87); `mesh_sequence` meshes a list of times.

Clean-up and measurement of the extracted mesh (connected components, Taubin smoothing, normals, area / volume / extents) are in
swnerf.meshops and re-exported here: `components`, `keep_components`, `vertex_faces`, `smooth`, `vertex_normals`, `measure`,
`clean`, and the `clean=` keyword of `generate_mesh` / `nerf_to_mesh`; so are welding and decimation by vertex clustering:
`cluster`, `weld`, `decimate`, `decimation_cell` (and the `weld` / `decimate` keys of `clean`), and hole filling: `boundary_loops`,
`fill_holes` (and the `fill_holes` key of `clean`).  Rendering a mesh from the project's cameras and checking it against reference
silhouettes and depth maps are in swnerf.meshrender and re-exported here: `render_views`, `render_views_arrays`, `compare_views`."""
import ctypes

import numpy as np
import torch

from . import _lib


def generate_viewdirs(num_views=100):
    """extract_mesh.py:7-24: golden-angle spiral on the unit sphere, float64 [num_views, 3]."""
    k = np.arange(0, num_views, dtype=float) + 0.5
    phi = np.arccos(1 - 2 * k / num_views)
    theta = np.pi * (1 + 5 ** 0.5) * k
    return np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], axis=1)


def _single_time(frame_time):
    """frame_time as the kernels read it (one float32 value): a Python number, or a tensor whose values are all equal - the
    reference's "Only accepts all points from same time" (d_nerf/run_dnerf.py:53, t_nerf/run_tnerf.py:52)."""
    if isinstance(frame_time, torch.Tensor):
        if frame_time.numel() == 0:
            raise ValueError("swnerf.mesh.query_points: frame_time is an empty tensor")
        lo, hi = torch.aminmax(frame_time.detach().float())
        lo, hi = float(lo), float(hi)
        if lo != hi:
            raise ValueError("swnerf.mesh.query_points: Only accepts all points from same time "
                             f"(frame_time spans [{lo}, {hi}]; per-point times are not built)")
        return lo
    return float(np.float32(frame_time))


def _query_tnerf_rows(net, pts, dirs, t):
    """T-NeRF with one direction per point: the op path (embedders, then TNeRF.forward) - the fused stream has no per-row
    direction columns."""
    from .embedder import get_embedder
    bands = net.fused_bands()
    if bands is None:
        net.packed()                                       # raises, naming the shapes that are built
    Lp, Ld, Lt = bands
    tt = torch.full((pts.shape[0], 1), t, dtype=torch.float32, device=pts.device)
    ex, ed, et = get_embedder(Lp, 3)[0](pts), get_embedder(Ld, 3)[0](dirs), get_embedder(Lt, 1)[0](tt)
    return net(torch.cat([ex, ed], -1), ed, et).reshape(-1, 4)


def query_points(net, pts, viewdirs, shared_dirs=None, frame_time=None, return_dx=False):
    """pts [M,3]; viewdirs [M,3] (one per point -> raw [M,4], what network_query_fn(positions, viewdirs, fn)
    returns) or [V,3] shared (-> [M,4] = [mean_v raw rgb, sigma]).  `shared_dirs` defaults to
    `viewdirs.shape[0] != M`.
    A time-conditioned net (DirectTemporalNeRF, TNeRF) is queried at ONE `frame_time`: a Python float, or a tensor whose values
    are all equal (swnerf_query_points_time; for TNeRF rgb is what `color` returns, after its ReLU).  return_dx=True
    (DirectTemporalNeRF only) -> (out [M,4], position_delta [M,3])."""
    from .model import TNeRF
    tnerf = isinstance(net, TNeRF)
    kind = _lib.NET_TNERF if tnerf else net._pack_params()[0]          # refusals first: they need neither the GPU nor a packed blob
    timed = kind in (_lib.NET_DNERF, _lib.NET_TNERF)
    if kind != _lib.NET_CANON and not timed:
        raise NotImplementedError("swnerf.mesh.query_points: nets with view directions only (8x256 static, DirectTemporalNeRF, TNeRF)")
    if not timed and frame_time is not None:
        raise ValueError("swnerf.mesh.query_points: a static net takes no frame_time")
    if timed and frame_time is None:
        raise NotImplementedError("swnerf.mesh.query_points: a time-conditioned net is queried at one frame time - pass frame_time")
    if return_dx and kind != _lib.NET_DNERF:
        raise ValueError("swnerf.mesh.query_points: return_dx is the position_delta of a DirectTemporalNeRF")
    t = _single_time(frame_time) if timed else None
    pts = _lib.dev_f32(pts, "pts", 3).reshape(-1, 3)
    dirs = _lib.dev_f32(viewdirs, "viewdirs", 3).reshape(-1, 3)
    M = pts.shape[0]
    if shared_dirs is None:
        shared_dirs = dirs.shape[0] != M
    out = torch.empty((M, 4), dtype=torch.float32, device=pts.device)
    if tnerf and not shared_dirs:
        if dirs.shape[0] != M:
            raise RuntimeError(f"swnerf.mesh.query_points: need one direction per point, got {dirs.shape[0]} for {M} points")
        return _query_tnerf_rows(net, pts, dirs, t) if M else out
    kind, packed, Lp, Ld, Lt = net.packed()
    if not timed:
        _lib.check(_lib.lib().swnerf_query_points(_lib.ptr(packed), _lib.ptr(pts), M, _lib.ptr(dirs), dirs.shape[0],
                                                  int(bool(shared_dirs)), Lp, Ld, _lib.ptr(out), _lib.stream_of(pts)),
                   "query_points")
        return out
    run_deform = 0 if tnerf else int(not (t == 0. and net.zero_canonical))
    dx = torch.empty((M, 3), dtype=torch.float32, device=pts.device) if return_dx else None
    _lib.check(_lib.lib().swnerf_query_points_time(kind, _lib.ptr(packed), _lib.ptr(pts), M, _lib.ptr(dirs), dirs.shape[0],
                                                   int(bool(shared_dirs)), t, run_deform, Lp, Ld, Lt, _lib.ptr(out), _lib.ptr(dx),
                                                   _lib.stream_of(pts)), "query_points_time")
    return (out, dx) if return_dx else out


def sample_grid(bounds, resolution, net, num_views=100, batch_size=1 << 20, sharded=None, group=None, query=None, on_device=False,
                frame_time=None, points_device=None):
    """extract_mesh.py:27-90 with the network in place of `nerf_function`:
    -> (density_field [R,R,R], color_field [R,R,R,3], (X, Y, Z)), float64 numpy like the reference.
    `color` is the view-average of the RAW rgb and `density` of the raw sigma (batch_query_fn :155-175
    applies no sigmoid / relu).
    Multi-GPU ("shards over 8 GPUs the same way"): with torch.distributed initialised (`sharded`
    defaults to that) every rank queries its contiguous shard of the R^3 points and ONE all-gather of the [n,4] results
    returns the whole field to every rank - points are independent, exactly like rays (swnerf.parallel).
    `query(points [n,3] tensor, dirs [V,3] tensor) -> [n,4]` defaults to the fused HIP query of `net`.
    on_device=True returns the [R,R,R,4] float32 device tensor [rgb, sigma] instead (no host copy), for marching_cubes.
    frame_time: the one time a time-conditioned net (DirectTemporalNeRF, TNeRF) is queried at (query_points); an injected
    `query` keeps its two-argument form and never sees it.  points_device: the [R^3,3] float32 grid points already on the
    net's device (mesh_sequence uploads them once for all its times)."""
    import torch.distributed as dist
    from .parallel import gather_pixels
    from .synth import shard_range
    x = np.linspace(bounds[0][0], bounds[0][1], resolution)
    y = np.linspace(bounds[1][0], bounds[1][1], resolution)
    z = np.linspace(bounds[2][0], bounds[2][1], resolution)
    X, Y, Z = np.meshgrid(x, y, z, indexing='ij')
    points = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=-1)
    dev = next(net.parameters()).device if net is not None else torch.device("cpu")
    dirs = torch.tensor(generate_viewdirs(num_views), dtype=torch.float32, device=dev)
    if query is None:
        query = lambda p, d: query_points(net, p, d, shared_dirs=True, frame_time=frame_time)
    on = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    if sharded is None:
        sharded = on
    world, rank = (dist.get_world_size(group), dist.get_rank(group)) if (sharded and on) else (1, 0)
    ranges = [shard_range(len(points), world, r) for r in range(world)]
    lo, hi = ranges[rank]
    outs = []
    with torch.no_grad():
        for s in range(lo, hi, batch_size):
            e = min(hi, s + batch_size)
            p = points_device[s:e] if points_device is not None else torch.tensor(points[s:e], dtype=torch.float32, device=dev)
            outs.append(query(p, dirs))
    local = torch.cat(outs, 0) if outs else torch.empty((0, 4), dtype=torch.float32, device=dev)
    out = gather_pixels(local, [b - a for a, b in ranges], group) if world > 1 else local
    if on_device:
        return out.reshape(resolution, resolution, resolution, 4)
    out = out.cpu().numpy().astype(np.float64)
    return (out[:, 3].reshape(resolution, resolution, resolution),
            out[:, :3].reshape(resolution, resolution, resolution, 3), (X, Y, Z))


def _field_ld(t, name, trailing):
    """(tensor, ld): a float32 cuda tensor whose point strides are a uniform multiple ld of C order (and whose `trailing`
    channels are contiguous), or a contiguous copy with ld = `trailing` or 1."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"swnerf.mesh.marching_cubes: {name} must be a CUDA tensor (there is no CPU implementation)")
    if t.dtype != torch.float32:
        t = t.float()
    nx, ny, nz = t.shape[:3]
    st = t.stride()
    ld = st[2]
    if trailing and (t.shape[3] != 3 or st[3] != 1):
        ld = -1
    if not (ld >= (3 if trailing else 1) and st[1] == nz * ld and st[0] == ny * nz * ld):
        t = t.contiguous()
        ld = 3 if trailing else 1
    return t, ld


def marching_cubes(density, level, spacing=(1., 1., 1.), origin=(0., 0., 0.), colors=None):
    """Iso-surface {density = level} of a CUDA float32 field [nx,ny,nz] (strides a uniform multiple ld of C order, e.g.
    q[..., 3] of a [R,R,R,4] query output, read in place; other layouts are copied) on the GPU.  A point is inside iff
    density > level.  -> (verts [V,3] f32, faces [F,3] int32, normals [V,3] f32, vertex_colors [V,3] f32 or None), on the
    field's device.  Vertex coordinate = index * spacing + origin; normals point toward lower density; faces wind outward
    from the dense side.  colors [nx,ny,nz,3] (e.g. q[..., :3]): each vertex takes the colour of its nearer edge end point."""
    if density.dim() != 3:
        raise ValueError(f"swnerf.mesh.marching_cubes: density must be [nx,ny,nz], got {tuple(density.shape)}")
    nx, ny, nz = density.shape
    if min(nx, ny, nz) < 2:
        raise ValueError(f"swnerf.mesh.marching_cubes: every grid dimension must be >= 2, got {tuple(density.shape)}")
    f, ld = _field_ld(density, "density", 0)
    c, cld = (None, 0)
    if colors is not None:
        if tuple(colors.shape) != (nx, ny, nz, 3):
            raise ValueError(f"swnerf.mesh.marching_cubes: colors must be [{nx},{ny},{nz},3], got {tuple(colors.shape)}")
        c, cld = _field_ld(colors.to(f.device), "colors", 3)
    L = _lib.lib()
    dev, st = f.device, _lib.stream_of(f)
    ws = torch.empty(L.swnerf_mc_workspace_bytes(nx, ny, nz), dtype=torch.uint8, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    lv = float(np.float32(level))
    _lib.check(L.swnerf_mc_count(_lib.ptr(f), nx, ny, nz, ld, lv, _lib.ptr(ws), _lib.ptr(totals), st), "marching_cubes")
    V, F = (int(x) for x in totals.cpu())                          # the one host synchronisation: sizes the outputs
    verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((V, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
    vcol = torch.empty((V, 3), dtype=torch.float32, device=dev) if c is not None else None
    fl3 = lambda v: (ctypes.c_float * 3)(*(float(np.float32(x)) for x in v))
    _lib.check(L.swnerf_mc_emit(_lib.ptr(f), _lib.ptr(c), nx, ny, nz, ld, cld, lv, fl3(spacing), fl3(origin), _lib.ptr(ws),
                                V, F, _lib.ptr(verts), _lib.ptr(faces), _lib.ptr(normals), _lib.ptr(vcol), st), "marching_cubes")
    return verts, faces, normals, vcol


class Mesh:
    """What generate_mesh returns in place of a trimesh.Trimesh: numpy vertices [V,3], faces [F,3] (0-based int32),
    vertex_normals [V,3], vertex_colors [V,3] or None, and export(path) -> OBJ."""

    def __init__(self, vertices, faces, vertex_normals, vertex_colors=None):
        self.vertices, self.faces, self.vertex_normals, self.vertex_colors = vertices, faces, vertex_normals, vertex_colors

    def export(self, path):
        """Wavefront OBJ: `v x y z [r g b]` (colours clipped to [0,1]), `vn`, `f a//a b//b c//c` (1-based); %.9g keeps every
        float32 exact.  Formatted one block per record type (no per-vertex Python loop)."""
        v = np.asarray(self.vertices, np.float32).reshape(-1, 3)
        if self.vertex_colors is not None:
            v = np.concatenate([v, np.clip(np.asarray(self.vertex_colors, np.float32).reshape(-1, 3), 0, 1)], 1)
        vn = np.asarray(self.vertex_normals, np.float32).reshape(-1, 3)
        f = np.asarray(self.faces, np.int64).reshape(-1, 3) + 1
        with open(path, "w") as fh:
            fh.write(f"# swnerf marching cubes: {len(v)} vertices, {len(f)} faces\n")
            fh.write(_rows("v", v, "%.9g"))
            fh.write(_rows("vn", vn, "%.9g"))
            fh.write(_rows("f", np.repeat(f, 2, axis=1), "%d//%d", per=2))
        return path

    def measure(self):
        """area, volume, centroid, extents, edge statistics of this mesh, computed on the GPU (swnerf.meshops.measure)"""
        from . import meshops
        return meshops.measure(self)


def _rows(tag, a, fmt, per=1):
    """`tag` + one line per row of a 2-D array, `per` values per field (a//a)"""
    if a.shape[0] == 0:
        return ""
    field = " " + fmt
    line = tag + field * (a.shape[1] // per) + "\n"
    vals = a.astype(np.float64).ravel().tolist() if a.dtype.kind == "f" else a.ravel().tolist()
    return (line * a.shape[0]) % tuple(vals)


def load_obj(path):
    """The arrays Mesh.export wrote: (vertices [V,3], faces [F,3] 0-based, normals [V,3], colours [V,3] or None)."""
    v, vn, f = [], [], []
    with open(path) as fh:
        for ln in fh:
            t = ln.split()
            if not t or t[0].startswith("#"):
                continue
            if t[0] == "v":
                v.append([float(x) for x in t[1:]])
            elif t[0] == "vn":
                vn.append([float(x) for x in t[1:]])
            elif t[0] == "f":
                f.append([int(x.split("//")[0]) - 1 for x in t[1:]])
    v = np.array(v, np.float32).reshape(len(v), -1) if v else np.zeros((0, 3), np.float32)
    cols = v[:, 3:6] if v.shape[1] == 6 else None
    return (v[:, :3].reshape(-1, 3), np.array(f, np.int32).reshape(-1, 3), np.array(vn, np.float32).reshape(-1, 3), cols)


def _grid_geometry(xyz_coords):
    """generate_mesh's spacing and origin (extract_mesh.py:101-113): X[1,0,0] - X[0,0,0], ... and X[0,0,0], ..."""
    X, Y, Z = xyz_coords
    spacing = (X[1, 0, 0] - X[0, 0, 0], Y[0, 1, 0] - Y[0, 0, 0], Z[0, 0, 1] - Z[0, 0, 0])
    origin = (X[0, 0, 0], Y[0, 0, 0], Z[0, 0, 0])
    return tuple(float(x) for x in spacing), tuple(float(x) for x in origin)


def _check_clean(clean):
    """refuse a bad `clean=` before any GPU work"""
    from . import meshops
    meshops.clean_options(clean)


def _to_mesh(out, clean=None):
    """device arrays -> Mesh; `clean` (None, True or a dict of meshops.clean's keywords) is applied on the device first"""
    from . import meshops
    opts = meshops.clean_options(clean)
    if opts is not None:
        out = meshops.clean_arrays(*out, **opts)
    verts, faces, normals, vcol = out
    return Mesh(verts.cpu().numpy(), faces.cpu().numpy(), normals.cpu().numpy(), None if vcol is None else vcol.cpu().numpy())


def generate_mesh(density_field, color_field, xyz_coords, density_threshold=0.5, device=None, clean=None):
    """extract_mesh.py:92-131 on the GPU: marching cubes of density_field at density_threshold with the reference's spacing /
    origin derivation, each vertex coloured by its nearest sample -> Mesh.  clean: None (the surface as extracted), True or a dict
    of `clean`'s keywords (floaters removed, optionally smoothed, on the device before the host copy).  The fields are the float64
    numpy arrays of sample_grid (computed in float32 here) or CUDA tensors; color_field may be None.  Differences from skimage +
    trimesh: DESIGN.md 6b."""
    _check_clean(clean)
    spacing, origin = _grid_geometry(xyz_coords)
    if device is None:
        device = density_field.device if isinstance(density_field, torch.Tensor) and density_field.is_cuda else torch.device("cuda")
    as_dev = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a, np.float32))).to(device, torch.float32)
    d = as_dev(density_field)
    c = as_dev(color_field) if color_field is not None else None
    return _to_mesh(marching_cubes(d, density_threshold, spacing, origin, c), clean)


def _grid_spacing_origin(bounds, resolution):
    axes = [np.linspace(b[0], b[1], resolution) for b in bounds]
    return tuple(float(a[1] - a[0]) for a in axes), tuple(float(a[0]) for a in axes)


def nerf_to_mesh(net, bounds, resolution=64, density_threshold=8, num_views=100, batch_size=1 << 20, frame_time=None, clean=None):
    """extract_mesh.py:133-145 with the network in place of `nerf_function`: grid query and marching cubes on the net's
    device, no host round trip of the field (the [R,R,R,4] query output is read in place) -> Mesh.  frame_time: the time a
    time-conditioned net is meshed at (sample_grid).  clean: as in generate_mesh."""
    _check_clean(clean)
    q = sample_grid(bounds, resolution, net, num_views=num_views, batch_size=batch_size, on_device=True, sharded=False,
                    frame_time=frame_time)
    spacing, origin = _grid_spacing_origin(bounds, resolution)
    return _to_mesh(marching_cubes(q[..., 3], density_threshold, spacing, origin, q[..., :3]), clean)


def mesh_sequence(net, bounds, times, resolution=64, density_threshold=8, num_views=100, out_dir=None, basename="mesh_{:03d}.obj"):
    """The surface of a time-conditioned net (DirectTemporalNeRF, TNeRF) at every time of `times` -> [Mesh, ...]: one grid
    query and one marching-cubes pass per time on the net's device, the R^3 grid points uploaded once.  With `out_dir` mesh i is
    also written to out_dir/basename.format(i) (Wavefront OBJ, Mesh.export).  The meshes are as extracted: `clean(m)` removes the
    floaters of each (the signature is pinned by tests/test_query_time_host.py, so there is no `clean=` keyword here)."""
    import os
    axes = [np.linspace(b[0], b[1], resolution) for b in bounds]
    X, Y, Z = np.meshgrid(*axes, indexing='ij')
    dev = next(net.parameters()).device
    pts = torch.tensor(np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=-1), dtype=torch.float32, device=dev)
    spacing, origin = _grid_spacing_origin(bounds, resolution)
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
    meshes = []
    for i, t in enumerate(times):
        q = sample_grid(bounds, resolution, net, num_views=num_views, on_device=True, sharded=False, frame_time=float(t),
                        points_device=pts)
        m = _to_mesh(marching_cubes(q[..., 3], density_threshold, spacing, origin, q[..., :3]))
        if out_dir is not None:
            m.export(os.path.join(out_dir, basename.format(i)))
        meshes.append(m)
    return meshes


from .meshops import (components, select_components, keep_components, vertex_faces, smooth_step, smooth, vertex_normals,  # noqa: E402,F401
                      measure, measure_raw, clean, Measurement, cluster, collapse_counts, weld, decimate, decimation_cell,
                      simplify_arrays, weld_arrays, decimate_arrays, boundary_loops, fill_holes, fill_holes_arrays)
from .meshrender import render_views, render_views_arrays, compare_views  # noqa: E402,F401
