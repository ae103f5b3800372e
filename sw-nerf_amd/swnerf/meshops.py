"""Mesh clean-up and measurement on the device (DESIGN.md 6b "Clean-up and measurement"): what a trimesh user does after
nerf/extract_mesh.py and nerf/transform_mesh.py - `split()` / keep the object, `smoothed()`, then read extents, area and volume.
All of it runs on the [V,3] float32 / [F,3] int32 arrays `mesh.marching_cubes` leaves on the GPU (swnerf_mesh_* of
include/swnerf.h; csrc/meshops_kernels.hip, meshops_math.h); `swnerf.mesh` re-exports every name here.

  components(faces, n_vertices)       vertex labels (the smallest vertex index of the component) and the (label, faces, vertices) table
  keep_components(verts, faces, ...)  the `keep` largest components of at least `min_faces` faces, compacted
  vertex_faces(faces, n_vertices)     CSR of the corners 3 f + k at each vertex, ascending
  smooth(verts, faces, ...)           Taubin smoothing: iterations x (umbrella step lam, umbrella step mu), bit-reproducible
  vertex_normals(verts, faces)        area-weighted normals
  measure(verts, faces)               area, volume, centroid, bounding box, edge statistics, Euler characteristic, closedness
  clean(mesh, ...)                    components -> selection -> compaction -> optional smoothing (+ normals) -> Mesh

A mesh argument is a `Mesh`, the 4-tuple of `marching_cubes`, an OBJ path, or verts and faces (tensors or arrays); host data is
uploaded.  A face index outside 0..V-1 raises ValueError naming how many there are; it is never dereferenced."""
import numpy as np
import torch

from . import _lib

VALUE_SLOTS, COUNT_SLOTS = 16, 8


def _device(device=None):
    return torch.device("cuda") if device is None else torch.device(device)


def _faces(faces, device=None):
    """-> contiguous int32 [F,3] on the GPU"""
    if isinstance(faces, torch.Tensor):
        if faces.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"swnerf.mesh: faces must be int32 (or int64) indices, got {faces.dtype}")
        t = faces
    else:
        a = np.asarray(faces)
        if a.dtype.kind not in "iu":
            raise TypeError(f"swnerf.mesh: faces must be integer indices, got {a.dtype}")
        t = torch.from_numpy(np.ascontiguousarray(a.astype(np.int64)))
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"swnerf.mesh: faces must be [F,3], got {tuple(t.shape)}")
    if not t.is_cuda:
        t = t.to(_device(device))
    return t.to(torch.int32).contiguous()


def _rows3(a, name, device=None, like=None):
    """-> contiguous float32 [V,3] on the GPU (like.device when `like` is given)"""
    if not isinstance(a, torch.Tensor):
        a = np.asarray(a)
        if a.dtype.kind not in "fiu":
            raise TypeError(f"swnerf.mesh: {name} must be floating point, got {a.dtype}")
        a = torch.from_numpy(np.ascontiguousarray(a, np.float32))
    elif not a.dtype.is_floating_point:
        raise TypeError(f"swnerf.mesh: {name} must be floating point, got {a.dtype}")
    if a.dim() != 2 or a.shape[1] != 3:
        raise ValueError(f"swnerf.mesh: {name} must be [V,3], got {tuple(a.shape)}")
    if like is not None:
        if a.shape[0] != like.shape[0]:
            raise ValueError(f"swnerf.mesh: {name} has {a.shape[0]} rows for {like.shape[0]} vertices")
        a = a.to(like.device)
    elif not a.is_cuda:
        a = a.to(_device(device))
    return a.to(torch.float32).contiguous()


def _sizes(V, F):
    if V >= 2 ** 31 or 3 * F >= 2 ** 31:
        raise ValueError(f"swnerf.mesh: {V} vertices / {F} faces: corner ids 3 f + k are int32 (V < 2^31, 3 F < 2^31)")


def _workspace(V, F, device):
    _sizes(V, F)
    return torch.empty(int(_lib.lib().swnerf_mesh_workspace_bytes(V, F)), dtype=torch.uint8, device=device)


def _bad(n):
    if n:
        raise ValueError(f"swnerf.mesh: {n} face indices are outside 0..V-1")


def as_arrays(m, faces=None, device=None):
    """A Mesh, the tuple of marching_cubes, an OBJ path, or (verts, faces) -> (verts, faces, normals or None, colors or None) as
    device tensors."""
    from . import mesh as _mesh
    if faces is None:
        if isinstance(m, str):
            m = _mesh.load_obj(m)
        if isinstance(m, _mesh.Mesh):
            m = (m.vertices, m.faces, m.vertex_normals, m.vertex_colors)
        if not (isinstance(m, (tuple, list)) and len(m) in (2, 4)):
            raise TypeError("swnerf.mesh: expected a Mesh, (verts, faces, normals, colors), an OBJ path, or verts and faces")
        v, f = m[0], m[1]
        n, c = (m[2], m[3]) if len(m) == 4 else (None, None)
    else:
        v, f, n, c = m, faces, None, None
    v = _rows3(v, "verts", device)
    f = _faces(f, v.device).to(v.device)
    n = None if n is None or len(n) != len(v) else _rows3(n, "normals", like=v)
    c = None if c is None else _rows3(c, "colors", like=v)
    return v, f, n, c


# ---------------------------------------------------------------------------------------------------------------- components
def components(faces, n_vertices):
    """-> (vlabel int32 [V] device tensor, table int64 numpy [C,3]): every vertex's component label (the smallest vertex index in
    it) and one row (label, faces, vertices) per component in ascending label order.  A face belongs to the label of its first
    vertex; an unreferenced vertex is a component of 0 faces.  Reading the counts and the table is the host synchronisation."""
    V = int(n_vertices)
    if V < 0:
        raise ValueError(f"swnerf.mesh.components: n_vertices must be >= 0, got {V}")
    f = _faces(faces)
    F = f.shape[0]
    dev = f.device
    ws = _workspace(V, F, dev)
    vlabel = torch.empty(V, dtype=torch.int32, device=dev)
    table = torch.empty((V, 3), dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().swnerf_mesh_components(_lib.ptr(f), V, F, _lib.ptr(ws), _lib.ptr(vlabel), _lib.ptr(table), _lib.ptr(counts),
                                                 _lib.stream_of(f)), "mesh_components")
    C, bad = (int(x) for x in counts.cpu())
    _bad(bad)
    return vlabel, table[:C].cpu().numpy().astype(np.int64)


def _check_selection(keep, min_faces):
    if not (keep == "all" or (isinstance(keep, (int, np.integer)) and not isinstance(keep, bool) and keep >= 1)):
        raise ValueError(f"swnerf.mesh: keep must be a positive integer or 'all', got {keep!r}")
    if not (isinstance(min_faces, (int, np.integer)) and min_faces >= 0):
        raise ValueError(f"swnerf.mesh: min_faces must be a non-negative integer, got {min_faces!r}")


def select_components(table, keep=1, min_faces=1):
    """Rows of the component table to keep, in ascending label order: at least min_faces faces, then the `keep` largest by face
    count (a tie goes to the smaller label); keep='all' keeps every row that passes min_faces."""
    _check_selection(keep, min_faces)
    t = np.asarray(table, np.int64).reshape(-1, 3)
    t = t[t[:, 1] >= min_faces]
    if keep != "all":
        order = np.lexsort((t[:, 0], -t[:, 1]))[:int(keep)]
        t = t[np.sort(order)]
    return t


def keep_components(verts, faces, normals=None, colors=None, keep=1, min_faces=1):
    """-> (verts', faces', normals' or None, colors' or None, kept labels numpy): the selected components (select_components),
    exactly verts[mask] and remap[faces[fmask]] - kept vertices and faces stay in their original order."""
    _check_selection(keep, min_faces)
    v = _rows3(verts, "verts")
    f = _faces(faces, v.device).to(v.device)
    n = None if normals is None else _rows3(normals, "normals", like=v)
    c = None if colors is None else _rows3(colors, "colors", like=v)
    vlabel, table = components(f, v.shape[0])
    return _compact(v, f, n, c, vlabel, select_components(table, keep, min_faces))


def _compact(v, f, n, c, vlabel, rows):
    V, F, dev = v.shape[0], f.shape[0], v.device
    Vo, Fo = int(rows[:, 2].sum()), int(rows[:, 1].sum())
    kept = torch.from_numpy(np.ascontiguousarray(rows[:, 0], np.int32)).to(dev)
    vo = torch.empty((Vo, 3), dtype=torch.float32, device=dev)
    fo = torch.empty((Fo, 3), dtype=torch.int32, device=dev)
    no = torch.empty_like(vo) if n is not None else None
    co = torch.empty_like(vo) if c is not None else None
    ws = _workspace(V, F, dev)
    _lib.check(_lib.lib().swnerf_mesh_compact(_lib.ptr(v), _lib.ptr(f), _lib.ptr(n), _lib.ptr(c), _lib.ptr(vlabel), V, F, _lib.ptr(kept),
                                              len(rows), _lib.ptr(ws), Vo, Fo, _lib.ptr(vo), _lib.ptr(fo), _lib.ptr(no), _lib.ptr(co),
                                              _lib.stream_of(v)), "mesh_compact")
    return vo, fo, no, co, rows[:, 0].copy()


# ----------------------------------------------------------------------------------------------------------------- incidence
def vertex_faces(faces, n_vertices):
    """-> (offsets int32 [V+1], items int32 [3F]) device tensors: vertex v's slice items[offsets[v]:offsets[v+1]] lists the corner
    ids 3 f + k with faces[f][k] == v in ascending order (any valence; a face may repeat an index)."""
    V = int(n_vertices)
    if V < 0:
        raise ValueError(f"swnerf.mesh.vertex_faces: n_vertices must be >= 0, got {V}")
    f = _faces(faces)
    F, dev = f.shape[0], f.device
    ws = _workspace(V, F, dev)
    offsets = torch.empty(V + 1, dtype=torch.int32, device=dev)
    items = torch.empty(3 * F, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().swnerf_mesh_incidence(_lib.ptr(f), V, F, _lib.ptr(ws), _lib.ptr(offsets), _lib.ptr(items), _lib.ptr(status),
                                                _lib.stream_of(f)), "mesh_incidence")
    _bad(int(status.cpu()))
    return offsets, items


def _incidence(incidence, f, V):
    if incidence is None:
        return vertex_faces(f, V)
    offsets, items = incidence
    if tuple(offsets.shape) != (V + 1,) or tuple(items.shape) != (3 * f.shape[0],) or offsets.dtype != torch.int32 or items.dtype != torch.int32:
        raise ValueError("swnerf.mesh: incidence must be the (offsets [V+1], items [3F]) int32 pair of vertex_faces for this mesh")
    return offsets.to(f.device).contiguous(), items.to(f.device).contiguous()


def smooth_step(verts, faces, s, incidence=None):
    """One umbrella step with factor s (float32): out = p + s (mean of the slice's neighbours - p), in fp64 in slice order."""
    v = _rows3(verts, "verts")
    f = _faces(faces, v.device).to(v.device)
    offsets, items = _incidence(incidence, f, v.shape[0])
    out = torch.empty_like(v)
    _lib.check(_lib.lib().swnerf_mesh_smooth_step(_lib.ptr(v), _lib.ptr(f), _lib.ptr(offsets), _lib.ptr(items), v.shape[0], f.shape[0],
                                                  float(np.float32(s)), _lib.ptr(out), _lib.stream_of(v)), "mesh_smooth_step")
    return out


def _check_smoothing(iterations, lam, mu):
    if not (isinstance(iterations, (int, np.integer)) and not isinstance(iterations, bool) and iterations >= 0):
        raise ValueError(f"swnerf.mesh.smooth: iterations must be a non-negative integer, got {iterations!r}")
    if not (np.isfinite(lam) and np.isfinite(mu)):
        raise ValueError(f"swnerf.mesh.smooth: lam and mu must be finite, got {lam!r}, {mu!r}")


def smooth(verts, faces, iterations=10, lam=0.5, mu=-0.53, incidence=None):
    """Taubin smoothing: `iterations` x (a step with lam, a step with mu) between two buffers -> new verts [V,3] (the input is
    never written).  The incidence is built once (or passed in).  Bit-identical from run to run and to the numpy replay."""
    _check_smoothing(iterations, lam, mu)
    v = _rows3(verts, "verts")
    f = _faces(faces, v.device).to(v.device)
    V, F = v.shape[0], f.shape[0]
    if iterations == 0 or V == 0:
        return v.clone()
    offsets, items = _incidence(incidence, f, V)
    L, st = _lib.lib(), _lib.stream_of(v)
    a, b = v, torch.empty_like(v)
    spare = torch.empty_like(v)
    for _ in range(int(iterations)):
        for s in (lam, mu):
            _lib.check(L.swnerf_mesh_smooth_step(_lib.ptr(a), _lib.ptr(f), _lib.ptr(offsets), _lib.ptr(items), V, F, float(np.float32(s)),
                                                 _lib.ptr(b), st), "mesh_smooth_step")
            a, b = b, (spare if a is v else a)
    return a


def vertex_normals(verts, faces, incidence=None):
    """Area-weighted normals [V,3]: the fp64 sum of cross(p1 - p0, p2 - p0) over the incident faces, normalised; (0,0,0) where the
    sum is zero.  With faces wound outward from the dense side they point toward lower density, like marching_cubes' own."""
    v = _rows3(verts, "verts")
    f = _faces(faces, v.device).to(v.device)
    offsets, items = _incidence(incidence, f, v.shape[0])
    out = torch.empty_like(v)
    _lib.check(_lib.lib().swnerf_mesh_vertex_normals(_lib.ptr(v), _lib.ptr(f), _lib.ptr(offsets), _lib.ptr(items), v.shape[0], f.shape[0],
                                                     _lib.ptr(out), _lib.stream_of(v)), "mesh_vertex_normals")
    return out


# ------------------------------------------------------------------------------------------------------------------- measure
class Measurement(dict):
    """The result of measure(): a dict whose keys also read as attributes."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


def measure_raw(verts, faces, incidence=None):
    """-> (values float64 [16], counts int64 [8]) numpy, as swnerf_mesh_measure writes them (include/swnerf.h)."""
    v = _rows3(verts, "verts")
    f = _faces(faces, v.device).to(v.device)
    V, F, dev = v.shape[0], f.shape[0], v.device
    offsets, items = _incidence(incidence, f, V)
    ws = _workspace(V, F, dev)
    values = torch.empty(VALUE_SLOTS, dtype=torch.float64, device=dev)
    counts = torch.empty(COUNT_SLOTS, dtype=torch.int64, device=dev)
    _lib.check(_lib.lib().swnerf_mesh_measure(_lib.ptr(v), _lib.ptr(f), _lib.ptr(offsets), _lib.ptr(items), V, F, _lib.ptr(ws),
                                              _lib.ptr(values), _lib.ptr(counts), _lib.stream_of(v)), "mesh_measure")
    values, counts = values.cpu().numpy(), counts.cpu().numpy()
    _bad(int(counts[7]))
    return values, counts


def measure(m, faces=None, incidence=None):
    """Area, signed volume (positive for faces wound outward), centroid (None for zero volume), bounding box of the referenced
    vertices (None when there is none) and its extents, component count, boundary / non-manifold edge counts, Euler
    characteristic and the closed flag -> Measurement.  `moments` are the raw first moments (centroid x volume)."""
    v, f, _, _ = as_arrays(m, faces)
    values, counts = measure_raw(v, f, incidence)
    vol = float(values[1])
    has_box = counts[0] > 0
    lo, hi = values[5:8].copy(), values[8:11].copy()
    return Measurement(area=float(values[0]), volume=vol, moments=values[2:5].copy(), centroid=values[2:5] / vol if vol != 0 else None,
                       bbox_min=lo if has_box else None, bbox_max=hi if has_box else None, extents=hi - lo if has_box else None,
                       n_vertices=int(v.shape[0]), n_faces=int(f.shape[0]), referenced_vertices=int(counts[0]), edges=int(counts[1]),
                       boundary_edges=int(counts[2]), nonmanifold_edges=int(counts[3]), n_components=int(counts[4]),
                       euler=int(counts[5]), closed=bool(counts[6]))


# --------------------------------------------------------------------------------------------------------------------- clean
def clean_arrays(verts, faces, normals=None, colors=None, keep=1, min_faces=1, smooth_iterations=0, lam=0.5, mu=-0.53):
    """clean() on device tensors -> (verts, faces, normals, colors) device tensors; the normals are recomputed iff smoothing ran
    (and when none came in)."""
    _check_smoothing(smooth_iterations, lam, mu)
    v, f, n, c, _ = keep_components(verts, faces, normals, colors, keep, min_faces)
    if smooth_iterations > 0 or n is None:
        inc = vertex_faces(f, v.shape[0])
        if smooth_iterations > 0:
            v = smooth(v, f, smooth_iterations, lam, mu, incidence=inc)
        n = vertex_normals(v, f, incidence=inc)
    return v, f, n, c


def clean_options(clean):
    """The `clean=` keyword of generate_mesh / nerf_to_mesh / mesh_sequence: None -> None, True -> the defaults, a dict of clean()'s
    keywords -> itself (checked)."""
    if clean is None or clean is False:
        return None
    if clean is True:
        return {}
    if not isinstance(clean, dict):
        raise TypeError(f"swnerf.mesh: clean must be None, True or a dict of clean()'s keywords, got {type(clean).__name__}")
    extra = set(clean) - {"keep", "min_faces", "smooth_iterations", "lam", "mu"}
    if extra:
        raise TypeError(f"swnerf.mesh: unknown clean option(s) {sorted(extra)}")
    return dict(clean)


def clean(m, keep=1, min_faces=1, smooth_iterations=0, lam=0.5, mu=-0.53):
    """Remove floaters and (optionally) the marching-cubes staircase: components -> the `keep` largest of at least `min_faces`
    faces -> compaction -> `smooth_iterations` of Taubin smoothing -> Mesh.  Vertex normals are recomputed iff smoothing ran."""
    from . import mesh as _mesh
    _check_selection(keep, min_faces)
    _check_smoothing(smooth_iterations, lam, mu)
    v, f, n, c = as_arrays(m)
    return _mesh._to_mesh(clean_arrays(v, f, n, c, keep, min_faces, smooth_iterations, lam, mu))
