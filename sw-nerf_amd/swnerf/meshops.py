"""Mesh clean-up and measurement on the device (DESIGN.md 6b "Clean-up and measurement"): what a trimesh user does after
nerf/extract_mesh.py and nerf/transform_mesh.py - `split()` / keep the object, `smoothed()`, then read extents, area and volume.
All of it runs on the [V,3] float32 / [F,3] int32 arrays `mesh.marching_cubes` leaves on the GPU (swnerf_mesh_* of
include/swnerf.h; csrc/meshops_kernels.hip, meshsimp_kernels.hip, meshfill_kernels.hip, meshops_math.h); `swnerf.mesh` re-exports every name here.

  components(faces, n_vertices)       vertex labels (the smallest vertex index of the component) and the (label, faces, vertices) table
  keep_components(verts, faces, ...)  the `keep` largest components of at least `min_faces` faces, compacted
  vertex_faces(faces, n_vertices)     CSR of the corners 3 f + k at each vertex, ascending
  smooth(verts, faces, ...)           Taubin smoothing: iterations x (umbrella step lam, umbrella step mu), bit-reproducible
  vertex_normals(verts, faces)        area-weighted normals
  measure(verts, faces)               area, volume, centroid, bounding box, edge statistics, Euler characteristic, closedness
  clean(mesh, ...)                    components -> selection -> compaction -> optional smoothing (+ normals) -> Mesh
  cluster(verts, cell)                vertex labels of a uniform grid (the smallest vertex index of each cell)
  weld(mesh, tolerance)               merge the vertices of one cell (trimesh's process=True); degenerate / duplicate faces go
  decimate(mesh, cell | target_faces) vertex clustering with a quadric (volume-keeping), mean or weld representative per cell
  decimation_cell(mesh, target_faces) the cell size that leaves at most target_faces faces (bisection of log2 cell)
  boundary_loops(faces, n_vertices)   the boundary as loops: (leader half-edge, length) table and the loop-ordered vertex lists
  fill_holes(mesh, max_edges)         close every boundary loop with a face or a fan around its mean (trimesh's fill_holes)

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


# ---------------------------------------------------------------------------------------------------- welding and decimation
PLACEMENTS = {"weld": 0, "mean": 1, "quadric": 2}                  # SWNERF_MESH_WELD, _MEAN, _QUADRIC
CELL_LIMIT = 2 ** 21                                               # cells an axis (the 21-bit index of the 64-bit cell key)


def _check_cell(cell, what="cell"):
    """-> the cell size as the float32 value the kernels use"""
    try:
        c = float(np.float32(cell))
    except (TypeError, ValueError):
        raise ValueError(f"swnerf.mesh: {what} must be a finite positive number, got {cell!r}") from None
    if not (np.isfinite(c) and c > 0):
        raise ValueError(f"swnerf.mesh: {what} must be a finite positive number, got {cell!r}")
    return c


def _check_placement(placement, eps):
    if placement not in PLACEMENTS:
        raise ValueError(f"swnerf.mesh: unknown placement {placement!r} (one of {sorted(PLACEMENTS)})")
    if not (np.isfinite(eps) and eps >= 0):
        raise ValueError(f"swnerf.mesh: eps must be finite and >= 0, got {eps!r}")


def _check_decimate(cell, target_faces, placement, eps):
    if (cell is None) == (target_faces is None):
        raise ValueError("swnerf.mesh.decimate: give exactly one of cell and target_faces")
    _check_placement(placement, eps)
    if cell is not None:
        return _check_cell(cell), None
    if not (isinstance(target_faces, (int, np.integer)) and not isinstance(target_faces, bool) and target_faces >= 1):
        raise ValueError(f"swnerf.mesh.decimate: target_faces must be an integer >= 1, got {target_faces!r}")
    return None, int(target_faces)


def _raw(m, faces=None):
    """The mesh argument with an OBJ path loaded and a Mesh opened, so that its vertices can be looked at before any upload"""
    from . import mesh as _mesh
    if faces is None:
        if isinstance(m, str):
            m = _mesh.load_obj(m)
        if isinstance(m, _mesh.Mesh):
            m = (m.vertices, m.faces, m.vertex_normals, m.vertex_colors)
    return m


def _extent(verts):
    """The largest bounding-box extent over the finite coordinates (0.0 when there is none): numpy for host data, so a refusal that
    depends on it needs no GPU."""
    try:
        if isinstance(verts, torch.Tensor):
            v = verts.detach().reshape(-1, 3).to(torch.float32)
            if v.shape[0] == 0:
                return 0.0
            fin = torch.isfinite(v)
            lo = torch.where(fin, v, torch.full_like(v, float("inf"))).amin(0).cpu().numpy().astype(np.float64)
            hi = torch.where(fin, v, torch.full_like(v, float("-inf"))).amax(0).cpu().numpy().astype(np.float64)
        else:
            v = np.asarray(verts, np.float32).reshape(-1, 3)
            if v.shape[0] == 0:
                return 0.0
            fin = np.isfinite(v)
            lo = np.where(fin, v, np.inf).min(0).astype(np.float64)
            hi = np.where(fin, v, -np.inf).max(0).astype(np.float64)
    except (TypeError, ValueError, RuntimeError):
        return 0.0                                                 # not [V,3] numbers: the conversion that follows says so
    ext = np.where(hi >= lo, hi - lo, 0.0)
    return float(ext.max())


def _check_grid(extent, cell):
    if extent / cell >= CELL_LIMIT:
        raise ValueError(f"swnerf.mesh: a cell of {cell:g} over an extent of {extent:g} needs {extent / cell:.3g} cells an axis; "
                         f"the cell index has 21 bits (fewer than {CELL_LIMIT})")


def default_tolerance(extent):
    """weld()'s default cell: the largest extent x 2^-20, the finest grid the 21-bit cell index allows with a factor 2 to spare
    (1.0 for a mesh without extent: every vertex is in one cell then, whatever its size)."""
    t = float(np.float32(extent * 2.0 ** -20))
    return t if np.isfinite(t) and t > 0 else 1.0


def _simplify_workspace(V, F, device):
    _sizes(V, F)
    return torch.empty(int(_lib.lib().swnerf_mesh_simplify_workspace_bytes(V, F)), dtype=torch.uint8, device=device)


def _cluster(v, cell, origin=None, ws=None):
    """-> (vlabel int32 [V], clusters, origin float32 [3]) on v's device; reading the counts is the host synchronisation"""
    V, dev = v.shape[0], v.device
    if origin is not None:
        origin = torch.as_tensor(np.asarray(origin, np.float32).reshape(3)).to(dev) if not isinstance(origin, torch.Tensor) \
            else origin.to(dev, torch.float32).reshape(3).contiguous()
    vlabel = torch.empty(V, dtype=torch.int32, device=dev)
    used = torch.zeros(3, dtype=torch.float32, device=dev)
    counts = torch.empty(3, dtype=torch.int32, device=dev)
    ws = _simplify_workspace(V, 0, dev) if ws is None else ws
    _lib.check(_lib.lib().swnerf_mesh_cluster(_lib.ptr(v), V, _lib.ptr(origin), cell, _lib.ptr(ws), _lib.ptr(vlabel), _lib.ptr(used),
                                              _lib.ptr(counts), _lib.stream_of(v)), "mesh_cluster")
    n, invalid, full = (int(x) for x in counts.cpu())
    if invalid:
        raise ValueError(f"swnerf.mesh: {invalid} vertices have no cell: a coordinate is not finite, or lies below the origin or "
                         f"2^21 cells of {cell:g} or more above it")
    if full:
        raise RuntimeError("swnerf.mesh: the cell table overflowed (it holds at least 2 V slots: this is a bug)")
    return vlabel, n, used


def _collapse(f, vlabel, V, ws=None):
    """-> (vmap int32 [V+1], fpos int32 [F+1], (V', F', degenerate, duplicate)); reading the counts is the host synchronisation"""
    F, dev = f.shape[0], f.device
    vmap = torch.empty(V + 1, dtype=torch.int32, device=dev)
    fpos = torch.empty(F + 1, dtype=torch.int32, device=dev)
    counts = torch.empty(5, dtype=torch.int32, device=dev)
    ws = _simplify_workspace(V, F, dev) if ws is None else ws
    _lib.check(_lib.lib().swnerf_mesh_collapse(_lib.ptr(f), _lib.ptr(vlabel), V, F, _lib.ptr(ws), _lib.ptr(vmap), _lib.ptr(fpos),
                                               _lib.ptr(counts), _lib.stream_of(f)), "mesh_collapse")
    c = [int(x) for x in counts.cpu()]
    _bad(c[4])
    return vmap, fpos, tuple(c[:4])


def cluster(verts, cell, origin=None):
    """-> (vlabel int32 [V] device tensor, number of clusters): vlabel[v] is the smallest vertex index in v's cell of the uniform
    grid of size `cell` at `origin` (default: the per-axis minimum of the vertices, found on the device).  In fp64 the cell index is
    floor((p - origin) / cell) per axis; a vertex whose index is not in [0, 2^21) on every axis - a NaN among them - raises
    ValueError naming how many there are."""
    c = _check_cell(cell)
    _check_grid(_extent(verts), c)
    v = _rows3(verts, "verts")
    vlabel, n, _ = _cluster(v, c, origin)
    return vlabel, n


def collapse_counts(verts, faces, cell, origin=None):
    """-> dict(vertices, faces, degenerate, duplicate, clusters): what simplify_arrays would leave at this cell size, from the
    cluster and collapse phases alone (nothing is emitted)."""
    c = _check_cell(cell)
    _check_grid(_extent(verts), c)
    v = _rows3(verts, "verts")
    f = _faces(faces, v.device).to(v.device)
    ws = _simplify_workspace(v.shape[0], f.shape[0], v.device)
    vlabel, n, _ = _cluster(v, c, origin, ws)
    _, _, (Vo, Fo, ndeg, ndup) = _collapse(f, vlabel, v.shape[0], ws)
    return dict(vertices=Vo, faces=Fo, degenerate=ndeg, duplicate=ndup, clusters=n)


def simplify_arrays(verts, faces, normals=None, colors=None, cell=1., placement="quadric", eps=1e-3, origin=None):
    """Vertex clustering on device tensors -> (verts', faces', normals' or None, colors' or None): cluster on the grid of size
    `cell`, send every face through the clustering (degenerate faces and duplicates go; the survivors keep their order and their
    corner order), and place one vertex per remaining cluster ('weld': the cluster's smallest vertex, bit for bit; 'mean'; 'quadric':
    Lindstrom's volume-keeping point inside the cell).  Normals are copied by 'weld' and recomputed (area-weighted) by the other
    two when normals came in."""
    c = _check_cell(cell)
    _check_placement(placement, eps)
    _check_grid(_extent(verts), c)
    v = _rows3(verts, "verts")
    f = _faces(faces, v.device).to(v.device)
    n = None if normals is None else _rows3(normals, "normals", like=v)
    col = None if colors is None else _rows3(colors, "colors", like=v)
    V, F, dev = v.shape[0], f.shape[0], v.device
    ws = _simplify_workspace(V, F, dev)
    vlabel, _, used = _cluster(v, c, origin, ws)
    vmap, fpos, (Vo, Fo, _, _) = _collapse(f, vlabel, V, ws)
    vo = torch.empty((Vo, 3), dtype=torch.float32, device=dev)
    fo = torch.empty((Fo, 3), dtype=torch.int32, device=dev)
    copy_normals = n is not None and placement == "weld"
    no = torch.empty_like(vo) if copy_normals else None
    co = torch.empty_like(vo) if col is not None else None
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().swnerf_mesh_collapse_emit(_lib.ptr(v), _lib.ptr(f), _lib.ptr(n) if copy_normals else None, _lib.ptr(col),
                                                    _lib.ptr(vlabel), _lib.ptr(vmap), _lib.ptr(fpos), _lib.ptr(used), c, V, F,
                                                    PLACEMENTS[placement], float(eps), _lib.ptr(ws), Vo, Fo, _lib.ptr(vo), _lib.ptr(fo),
                                                    _lib.ptr(no), _lib.ptr(co), _lib.ptr(status), _lib.stream_of(v)), "mesh_collapse_emit")
    _bad(int(status.cpu()))
    if n is not None and not copy_normals:
        no = vertex_normals(vo, fo)
    return vo, fo, no, co


def weld_arrays(verts, faces, normals=None, colors=None, tolerance=None):
    """weld() on device tensors -> (verts, faces, normals, colors)"""
    tol = default_tolerance(_extent(verts)) if tolerance is None else _check_cell(tolerance, "tolerance")
    return simplify_arrays(verts, faces, normals, colors, tol, "weld")


def weld(m, tolerance=None, faces=None):
    """Merge coincident vertices (trimesh's process=True): the vertices of one cell of a grid of size `tolerance` become the
    smallest-indexed of them, faces that collapse or repeat go, unreferenced vertices go -> Mesh.  The default tolerance is the
    largest bounding-box extent x 2^-20.  Like trimesh's rounding merge this is a grid merge, not a distance merge: two vertices
    closer than the tolerance that straddle a cell boundary stay apart."""
    from . import mesh as _mesh
    tol = None if tolerance is None else _check_cell(tolerance, "tolerance")
    raw = _raw(m, faces)
    ext = _extent(raw if faces is not None else raw[0])
    tol = default_tolerance(ext) if tol is None else tol
    _check_grid(ext, tol)
    return _mesh._to_mesh(_filled(weld_arrays(*as_arrays(raw, faces), tolerance=tol)))


def _filled(out):
    """Mesh wants normals: area-weighted ones when none came in"""
    v, f, n, c = out
    return v, f, vertex_normals(v, f) if n is None else n, c


def _decimation_cell(v, f, N, extent):
    if not extent > 0:
        return 1.0                                                 # one cell whatever its size: no face survives
    ws = _simplify_workspace(v.shape[0], f.shape[0], v.device)

    def faces_at(x):
        h = _check_cell(2.0 ** x)
        vlabel, _, _ = _cluster(v, h, None, ws)
        return _collapse(f, vlabel, v.shape[0], ws)[2][1]

    hi = float(np.log2(extent))
    lo = hi - 20.0
    if faces_at(hi) > N:
        raise ValueError(f"swnerf.mesh.decimate: even one cell of the mesh's extent leaves more than target_faces = {N} faces")
    if faces_at(lo) <= N:
        return _check_cell(2.0 ** lo)
    for _ in range(24):
        mid = 0.5 * (lo + hi)
        if faces_at(mid) <= N:
            hi = mid
        else:
            lo = mid
    return _check_cell(2.0 ** hi)


def decimation_cell(m, target_faces, faces=None):
    """The cell size decimate(m, target_faces=N) uses: log2 of the cell is bisected in 24 steps between the largest bounding-box
    extent x 2^-20 and the extent itself, keeping faces(hi) <= N < faces(lo), and the upper end is returned (the lower end when
    even the finest grid leaves at most N faces).  Each probe runs the cluster and collapse phases only.  ValueError when a single
    cell of the extent still leaves more than N faces."""
    _, N = _check_decimate(None, target_faces, "quadric", 1e-3)
    raw = _raw(m, faces)
    ext = _extent(raw if faces is not None else raw[0])
    v, f, _, _ = as_arrays(raw, faces)
    return _decimation_cell(v, f, N, ext)


def decimate_arrays(verts, faces, normals=None, colors=None, cell=None, target_faces=None, placement="quadric", eps=1e-3):
    """decimate() on device tensors -> (verts, faces, normals, colors); with target_faces >= F the input tensors themselves"""
    cell, N = _check_decimate(cell, target_faces, placement, eps)
    if N is not None:
        if len(faces) <= N:
            return verts, faces, normals, colors
        v = _rows3(verts, "verts")
        cell = _decimation_cell(v, _faces(faces, v.device).to(v.device), N, _extent(verts))
    return simplify_arrays(verts, faces, normals, colors, cell, placement, eps)


def decimate(m, cell=None, target_faces=None, placement="quadric", eps=1e-3, faces=None):
    """Decimate by vertex clustering -> Mesh: one vertex per occupied cell of a grid of size `cell` (or of decimation_cell(m,
    target_faces), which leaves at most target_faces faces; a mesh that already has no more is returned unchanged).  placement:
    'quadric' (the default: the point that keeps the cluster's faces' planes, and with them the volume), 'mean' or 'weld'; eps is
    the quadric's regularisation toward the mean.  Fully parallel and bit-reproducible; exactly one of cell and target_faces."""
    from . import mesh as _mesh
    cell, N = _check_decimate(cell, target_faces, placement, eps)
    raw = _raw(m, faces)
    if cell is not None:
        _check_grid(_extent(raw if faces is not None else raw[0]), cell)
    v, f, n, c = as_arrays(raw, faces)
    if N is not None and f.shape[0] <= N:
        return _mesh._to_mesh(_filled((v, f, n, c)))
    return _mesh._to_mesh(_filled(decimate_arrays(v, f, n, c, cell, N, placement, eps)))


# -------------------------------------------------------------------------------------------------------------- hole filling
INFO_KEYS = ("boundary_edges", "loops", "filled_loops", "filled_edges", "skipped_loops", "unfillable_edges", "new_vertices", "new_faces")


def _check_max_edges(max_edges, what="max_edges"):
    """-> max_edges as the kernels take it (0: no limit); no GPU"""
    if max_edges is None:
        return 0
    if not (isinstance(max_edges, (int, np.integer)) and not isinstance(max_edges, bool) and 3 <= max_edges < 2 ** 31):
        raise ValueError(f"swnerf.mesh: {what} must be None or an integer >= 3 (a loop has at least 3 edges), got {max_edges!r}")
    return int(max_edges)


def _check_fill(fill_holes):
    """clean()'s fill_holes: None / False -> None, True -> 0 (no limit), an integer >= 3 -> itself; no GPU"""
    if fill_holes is None or fill_holes is False:
        return None
    return 0 if fill_holes is True else _check_max_edges(fill_holes, "fill_holes")


def _fill_workspace(V, F, device):
    _sizes(V, F)
    return torch.empty(int(_lib.lib().swnerf_mesh_fill_workspace_bytes(V, F)), dtype=torch.uint8, device=device)


def _loops(f, V, max_edges, ws):
    """boundary and loops phases -> (table, loop_offsets, loop_vertices, loop_vnew, loop_fnew, info); the device tensors are cut to
    the L loops found.  Reading the counts after each phase is the host synchronisation."""
    F, dev = f.shape[0], f.device
    L_, st = _lib.lib(), _lib.stream_of(f)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    nb = 0
    if V > 0 and F > 0:
        bhe, bnext, counts = i32(3 * F), i32(3 * F), i32(2)
        _lib.check(L_.swnerf_mesh_boundary(_lib.ptr(f), V, F, _lib.ptr(ws), _lib.ptr(bhe), _lib.ptr(bnext), _lib.ptr(counts), st), "mesh_boundary")
        nb, bad = (int(x) for x in counts.cpu())
        _bad(bad)
    cap = nb // 3
    table, loop_offsets, loop_vertices, vnew, fnew, counts = i32(cap, 2), i32(cap + 1), i32(nb), i32(cap + 1), i32(cap + 1), i32(8)
    if nb > 0:
        _lib.check(L_.swnerf_mesh_boundary_loops(_lib.ptr(f), _lib.ptr(bhe), _lib.ptr(bnext), V, F, nb, max_edges, _lib.ptr(ws), _lib.ptr(table),
                                                 _lib.ptr(loop_offsets), _lib.ptr(loop_vertices), _lib.ptr(vnew), _lib.ptr(fnew),
                                                 _lib.ptr(counts), st), "mesh_boundary_loops")
        L, M, nfill, efill, Vn, Fn = (int(x) for x in counts[:6].cpu())
    else:
        L = M = nfill = efill = Vn = Fn = 0
        for t in (loop_offsets, vnew, fnew):
            t.zero_()
    info = dict(boundary_edges=nb, loops=L, filled_loops=nfill, filled_edges=efill, skipped_loops=L - nfill, unfillable_edges=nb - M,
                new_vertices=Vn, new_faces=Fn)
    return table[:L], loop_offsets[:L + 1], loop_vertices[:M], vnew[:L + 1], fnew[:L + 1], info


def boundary_loops(faces, n_vertices):
    """The boundary of a mesh as loops -> (table int64 numpy [L,2], loop_offsets int32 [L+1], loop_vertices int32 device tensors, info).
    Half-edge c = 3 f + k runs faces[f][k] -> faces[f][(k+1)%3]; it is a boundary half-edge when its edge occurs once over all faces.
    A loop is a cycle of boundary half-edges through vertices with exactly one entering and one leaving; table row i is (its
    smallest half-edge id, its length), rows ascending, and loop_vertices[loop_offsets[i]:loop_offsets[i+1]] are its vertices in
    order from that half-edge's tail (index them into verts for perimeters).  info: boundary_edges, loops, unfillable_edges
    (boundary half-edges on no loop: a bow-tie, a chain through a pinched vertex) and the fill counts without a length limit."""
    V = int(n_vertices)
    if V < 0:
        raise ValueError(f"swnerf.mesh.boundary_loops: n_vertices must be >= 0, got {V}")
    f = _faces(faces)
    table, loop_offsets, loop_vertices, _, _, info = _loops(f, V, 0, _fill_workspace(V, f.shape[0], f.device))
    return table.cpu().numpy().astype(np.int64), loop_offsets, loop_vertices, info


def fill_holes_arrays(verts, faces, normals=None, colors=None, max_edges=None):
    """fill_holes() on device tensors -> (verts, faces, normals or None, colors or None, info).  The input rows come first, bit for
    bit; new vertices and faces follow in ascending leader order.  Normals are recomputed (area-weighted) when normals came in and
    anything was added; when nothing was added the input tensors themselves are returned."""
    me = _check_max_edges(max_edges)
    v = _rows3(verts, "verts")
    f = _faces(faces, v.device).to(v.device)
    n = None if normals is None else _rows3(normals, "normals", like=v)
    c = None if colors is None else _rows3(colors, "colors", like=v)
    V, F, dev = v.shape[0], f.shape[0], v.device
    ws = _fill_workspace(V, F, dev)
    _, loop_offsets, loop_vertices, vnew, fnew, info = _loops(f, V, me, ws)
    if info["new_faces"] == 0:
        return v, f, n, c, info
    Vo, Fo = V + info["new_vertices"], F + info["new_faces"]
    _sizes(Vo, Fo)
    vo = torch.empty((Vo, 3), dtype=torch.float32, device=dev)
    fo = torch.empty((Fo, 3), dtype=torch.int32, device=dev)
    co = torch.empty_like(vo) if c is not None else None
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().swnerf_mesh_fill_emit(_lib.ptr(v), _lib.ptr(f), _lib.ptr(c), V, F, _lib.ptr(loop_offsets), _lib.ptr(loop_vertices),
                                                _lib.ptr(vnew), _lib.ptr(fnew), info["loops"], loop_vertices.shape[0], _lib.ptr(ws), Vo, Fo,
                                                _lib.ptr(vo), _lib.ptr(fo), _lib.ptr(co), _lib.ptr(status), _lib.stream_of(v)), "mesh_fill_emit")
    _bad(int(status.cpu()))
    return vo, fo, None if n is None else vertex_normals(vo, fo), co, info


def fill_holes(m, max_edges=None, faces=None):
    """Close the holes of a mesh (trimesh's fill_holes) -> Mesh with the counts as `.fill_info`: every boundary loop of at most
    max_edges edges (None: any length) gets one face when it is a triangle, else one new vertex at the mean of its vertices and a
    fan of faces wound like the surface around it, so that measure() sees a closed surface and its volume.  For a planar loop the
    fan gives the exact cap volume even when the loop is not convex (the triangles may then overlap).  Boundary edges through a
    vertex with more than one entering or leaving boundary edge are left alone (fill_info['unfillable_edges'])."""
    from . import mesh as _mesh
    _check_max_edges(max_edges)
    *out, info = fill_holes_arrays(*as_arrays(m, faces), max_edges=max_edges)
    r = _mesh._to_mesh(_filled(out))
    r.fill_info = info
    return r


_DECIMATE_KEYS = {"cell", "target_faces", "placement", "eps"}


def _check_clean_extras(weld, decimate, fill_holes=None):
    """-> (weld tolerance or None when weld is True, decimate keywords), both checked, and fill_holes checked; no GPU"""
    _check_fill(fill_holes)
    if not (weld is None or weld is False or weld is True):
        weld = _check_cell(weld, "weld")
    if decimate is not None:
        if not isinstance(decimate, dict) or set(decimate) - _DECIMATE_KEYS:
            raise TypeError(f"swnerf.mesh: decimate must be None or a dict of decimate()'s keywords {sorted(_DECIMATE_KEYS)}, got {decimate!r}")
        _check_decimate(decimate.get("cell"), decimate.get("target_faces"), decimate.get("placement", "quadric"), decimate.get("eps", 1e-3))
    return weld, decimate


# --------------------------------------------------------------------------------------------------------------------- clean
def clean_arrays(verts, faces, normals=None, colors=None, keep=1, min_faces=1, smooth_iterations=0, lam=0.5, mu=-0.53, weld=None,
                 decimate=None, fill_holes=None):
    """clean() on device tensors -> (verts, faces, normals, colors) device tensors; the normals are recomputed iff smoothing ran
    (and when none came in).  weld (None, True or a tolerance) is applied first, decimate (None or a dict of decimate()'s
    keywords) after the component selection, then fill_holes (None, True or a max_edges), both before the smoothing."""
    _check_smoothing(smooth_iterations, lam, mu)
    weld, decimate = _check_clean_extras(weld, decimate, fill_holes)
    fill = _check_fill(fill_holes)
    if weld is not None and weld is not False:
        verts, faces, normals, colors = weld_arrays(verts, faces, normals, colors, None if weld is True else weld)
    v, f, n, c, _ = keep_components(verts, faces, normals, colors, keep, min_faces)
    if decimate is not None:
        v, f, n, c = decimate_arrays(v, f, n, c, **decimate)
    if fill is not None:
        v, f, n, c, _ = fill_holes_arrays(v, f, n, c, fill or None)
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
    extra = set(clean) - {"keep", "min_faces", "smooth_iterations", "lam", "mu", "weld", "decimate", "fill_holes"}
    if extra:
        raise TypeError(f"swnerf.mesh: unknown clean option(s) {sorted(extra)}")
    _check_clean_extras(clean.get("weld"), clean.get("decimate"), clean.get("fill_holes"))
    return dict(clean)


def clean(m, keep=1, min_faces=1, smooth_iterations=0, lam=0.5, mu=-0.53, weld=None, decimate=None, fill_holes=None):
    """Remove floaters and (optionally) the marching-cubes staircase: [weld ->] components -> the `keep` largest of at least
    `min_faces` faces -> compaction [-> decimate] [-> fill_holes] -> `smooth_iterations` of Taubin smoothing -> Mesh.  weld: None,
    True (the default tolerance of weld()) or a tolerance; decimate: None or a dict of decimate()'s keywords; fill_holes: None, True
    or the longest loop to fill (fill_holes()'s max_edges) - the caps are smoothed with the rest.  Vertex normals are recomputed
    iff smoothing, a 'mean' / 'quadric' decimation or a fill ran."""
    from . import mesh as _mesh
    _check_selection(keep, min_faces)
    _check_smoothing(smooth_iterations, lam, mu)
    _check_clean_extras(weld, decimate, fill_holes)
    v, f, n, c = as_arrays(m)
    return _mesh._to_mesh(clean_arrays(v, f, n, c, keep, min_faces, smooth_iterations, lam, mu, weld, decimate, fill_holes))
