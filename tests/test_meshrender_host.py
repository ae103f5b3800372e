"""Mesh rendering without a GPU: the header-derived exports, the z-buffer size, every Python refusal, the numpy replay of
tests/meshrender_ref.py checked against independent facts (an analytic depth, front / back balance and cull symmetry on closed
surfaces), and csrc/meshrender_math.h on the host - tests/meshrender_host_main.cpp, a stand-alone program that renders through the
header's functions, pixel boxes included, over exact-size heap buffers, is built with g++ under AddressSanitizer and UBSan (without
them when the sanitizer runtime cannot be linked, as tests/test_meshops_host.py does) and must equal the replay, which tests every
pixel against every face, bit for bit: the device kernels call the same functions."""
import os
import subprocess

import numpy as np
import pytest

import meshops_ref as R
import meshrender_ref as M

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "sw-nerf_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
NAMES = ["swnerf_mesh_render_workspace_bytes", "swnerf_mesh_render_raster", "swnerf_mesh_render_resolve", "swnerf_mesh_view_compare"]
H, W, FOCAL = 40, 48, 60.0
CASES = M.cases()


def test_exports_come_from_the_header():
    from swnerf import _lib, mesh
    for n in NAMES:
        assert n in _lib.EXPORTS, n
    L = _lib.lib()
    assert all(hasattr(L, n) for n in NAMES)
    assert _lib.DEFINES["VERSION"] == 112
    assert (_lib.DEFINES["MESH_CULL_BACK"], _lib.DEFINES["MESH_CULL_FRONT"], _lib.DEFINES["MESH_SHADE_HEADLIGHT"]) == (1, 2, 2)
    for n in ("render_views", "render_views_arrays", "compare_views"):
        assert callable(getattr(mesh, n))
    from swnerf import runner
    assert callable(runner.render_path_mesh) and callable(runner.evaluate_mesh)


def test_workspace_bytes():
    from swnerf import _lib
    ws = _lib.lib().swnerf_mesh_render_workspace_bytes
    for N, h, w in ((-1, 4, 4), (1, -4, 4), (1, 4, -4), (1, 0, 4), (1, 4, 0), (1, 2 ** 16, 2 ** 15), (2, 2 ** 15, 2 ** 15), (2 ** 31, 1, 1),
                    (2 ** 40, 2 ** 40, 2 ** 40), (1, 2 ** 31, 1)):
        assert ws(N, h, w) == 0, (N, h, w)
    sizes = [0, 1, 2, 3, 31, 32, 33, 40, 48, 800]
    for h in sizes[1:]:
        for w in sizes[1:]:
            prev = 0
            for N in sizes:
                b = ws(N, h, w)
                assert b > 0 and b % 256 == 0 and b >= 8 * N * h * w and b >= prev, (N, h, w)
                prev = b
    assert [ws(3, h, 48) for h in sizes[1:]] == sorted(ws(3, h, 48) for h in sizes[1:])
    assert [ws(3, 40, w) for w in sizes[1:]] == sorted(ws(3, 40, w) for w in sizes[1:])
    assert ws(1, 2 ** 15, 2 ** 16 - 1) >= 8 * 2 ** 15 * (2 ** 16 - 1)


def test_python_refusals_need_no_gpu():
    from swnerf import mesh, runner
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    f = np.array([[0, 1, 2], [1, 2, 3]], np.int32)
    col = np.zeros_like(v)
    m, bare = mesh.Mesh(v, f, np.zeros_like(v), col), mesh.Mesh(v, f, np.zeros_like(v))
    poses = np.zeros((2, 3, 4), np.float32)
    for call in (lambda **kw: mesh.render_views(m, **kw), lambda **kw: mesh.render_views_arrays(v, f, colors=col, **kw)):
        good = dict(H=8, W=8, K=None, focal=10.0, poses=poses)
        for name in ("flat", "", None, 0, "color"):
            with pytest.raises(ValueError, match="shading"):
                call(**good, shading=name)
        for name in ("both", "", 1, True):
            with pytest.raises(ValueError, match="cull"):
                call(**good, cull=name)
        for near in (-1e-3, -1, float("nan")):
            with pytest.raises(ValueError, match="near"):
                call(**good, near=near)
        for near, far in ((1., 1.), (2., 1.), (0., 0.), (0., float("nan")), (0., -1.)):
            with pytest.raises(ValueError, match="far"):
                call(**good, near=near, far=far)
        for h, w in ((0, 8), (8, 0), (-1, 8), (8, -3), (2.5, 8), (8, None), (True, 8)):
            with pytest.raises(ValueError, match="positive integer"):
                call(**dict(good, H=h, W=w))
        for p in (np.zeros((3, 4)), np.zeros((2, 3, 3)), np.zeros((2, 4, 3)), np.zeros((2, 2, 3, 4)), np.zeros(12)):
            with pytest.raises(ValueError, match="poses"):
                call(**dict(good, poses=p))
        for K, focal in ((None, None), (np.eye(4), None), (np.zeros(3), None), (None, -1.0), (None, float("inf")), ("x", None)):
            with pytest.raises(ValueError, match="focal|K must"):
                call(**dict(good, K=K, focal=focal))
        with pytest.raises(ValueError, match="output"):
            call(**good, outputs=("rgb", "normal"))
        with pytest.raises(ValueError, match="background"):
            call(**good, background=(1, 2))
        with pytest.raises(ValueError, match="2\\^31"):
            call(**dict(good, H=2 ** 15, W=2 ** 15))
    with pytest.raises(ValueError, match="colours"):
        mesh.render_views(bare, 8, 8, None, poses, focal=10.0)
    with pytest.raises(ValueError, match="colours"):
        mesh.render_views_arrays(v, f, 8, 8, 10.0, poses, shading="colors")
    with pytest.raises(ValueError, match="colours"):
        mesh.render_views(v, 8, 8, 10.0, poses, faces=f)
    acc = np.zeros((2, 8, 8), np.float32)
    out = dict(acc=acc, depth=acc)
    with pytest.raises(ValueError, match="alpha or a reference depth"):
        mesh.compare_views(out)
    with pytest.raises(ValueError, match="acc"):
        mesh.compare_views({}, alpha=acc)
    for a in (np.zeros((2, 8, 9), np.float32), np.zeros((1, 8, 8), np.float32), np.zeros((2, 8, 8, 4, 1), np.uint8), np.zeros((8, 8), np.float32)):
        with pytest.raises(ValueError, match="alpha"):
            mesh.compare_views(out, alpha=a)
        with pytest.raises(ValueError, match="depth"):
            mesh.compare_views(out, depth=a)
    with pytest.raises(ValueError, match="alpha_channel"):
        mesh.compare_views(out, alpha=np.zeros((2, 8, 8, 4), np.uint8), alpha_channel=4)
    with pytest.raises(ValueError, match="shading"):
        runner.render_path_mesh(m, poses, [8, 8, 10.0], None, shading="flat")
    with pytest.raises(ValueError, match="split"):
        runner.evaluate_mesh(m, dict(images=None, poses=poses, hwf=[8, 8, 10.0], i_split=[[0], [1], []], K=None), split="all")


# ----------------------------------------------------------------------------------------- the replay against independent facts
def test_the_square_has_the_analytic_depth():
    """identity rotation, camera at z = 2, the square in z = 0: d_z = -1 exactly, so t = o_z up to its one float32 rounding"""
    v, f, cam = M.square()
    o = M.render(v, f, H, W, M.intrinsics(H, W, focal=FOCAL), cam)
    hit = o["acc"][0] > 0
    assert 300 < hit.sum() < H * W and o["ties"] == 0
    oz = np.float32(2.0)
    assert (np.abs(o["depth"][0][hit] - oz) <= np.spacing(oz)).all()
    assert (o["depth"][0][~hit] == 0).all() and (o["face"][0][~hit] == -1).all()
    px, py = np.arange(H * W) % W, np.arange(H * W) // W                  # the covered pixels are those whose ray meets the rectangle
    x = 0.1 + 2.0 * (px - W * 0.5) / FOCAL
    y = -0.2 - 2.0 * (py - H * 0.5) / FOCAL
    inside = (x > -0.4 + 1e-6) & (x < 0.5 - 1e-6) & (y > -0.3 + 1e-6) & (y < 0.45 - 1e-6)
    outside = (x < -0.4 - 1e-6) | (x > 0.5 + 1e-6) | (y < -0.3 - 1e-6) | (y > 0.45 + 1e-6)
    assert hit[inside].all() and not hit[outside].any()
    b = o["bary"][0][hit].astype(np.float64)
    assert (np.abs(b.sum(1) - 1) <= 3 * 2.0 ** -24).all() and (b >= 0).all()


@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres"])
def test_closed_fixtures_from_the_standard_views(name):
    """a closed surface is entered as often as it is left along every ray, there is no hit exactly on an edge from these views (a
    condition on the inputs), and culling either side leaves the same silhouette"""
    v, f, poses = CASES[name]
    intr = M.intrinsics(H, W, focal=FOCAL)
    o = M.render(v, f, H, W, intr, poses[:2])
    assert R.measure(v, f)["closed"]
    assert o["ties"] == 0
    assert np.array_equal(o["front"], o["back"]) and o["front"].sum() > 200
    back, front = (M.render(v, f, H, W, intr, poses[:2], cull=c, want_counts=False) for c in (1, 2))
    assert np.array_equal(back["acc"], o["acc"]) and np.array_equal(front["acc"], o["acc"])
    assert np.array_equal(back["face"], o["face"])                       # the nearest hit of a closed surface faces the camera
    hit = o["acc"] > 0
    assert (front["depth"][hit] > back["depth"][hit]).all()


def test_the_tie_view_sends_rays_through_edges():
    v, f, poses = CASES["sphere"]
    intr = M.intrinsics(48, 48, focal=FOCAL)
    d = M.ray_dirs(48, 48, intr, poses[2])
    U, V_, W_, det, _, tf = M.hit_terms([v[f[:, k]][None] for k in range(3)], poses[2][:, 3], d[:, None, :])
    ok = M.hit_mask(U, V_, W_, det, tf, 0., np.inf, 0)
    assert int((ok & ((U == 0) | (V_ == 0) | (W_ == 0))).sum()) == 40
    o = M.render(v, f, 48, 48, intr, poses[2:])
    assert o["ties"] == 40 and ((o["front"] + o["back"] > 0) == (o["acc"] > 0)).all()


def test_the_counters_of_the_single_faces():
    intr = M.intrinsics(H, W, focal=FOCAL)
    o = M.render(*CASES["whole_image"][:2], H, W, intr, CASES["whole_image"][2])
    assert o["acc"][0].all() and o["counts"].tolist()[:3] == [0, 0, 3]
    o = M.render(*CASES["behind"][:2], H, W, intr, CASES["behind"][2][:1])
    assert o["counts"].tolist() == [0, 1, 0, 0] and not o["acc"].any()
    v, f, p = CASES["straddles"]
    cls, npx, _ = M.boxes(v, f, p[0], intr, H, W)
    assert cls.tolist() == [2] and npx.tolist() == [H * W]
    assert 0 < M.render(v, f, H, W, intr, p[:1])["acc"].sum() < H * W
    for name, bad in (("repeated_index", 1), ("index_equal_V", 2), ("nan_vertex", 2)):
        assert M.render(*CASES[name][:2], H, W, intr, CASES[name][2][:1], want_counts=False)["counts"][0] == bad


def test_the_ordered_sum_is_the_sum():
    import math
    rng = np.random.default_rng(1)
    for n in (1, 1023, 1024, 1025, 1920, 5000):
        x = rng.standard_normal(n) ** 2
        assert abs(M.ordered_sum(x) - math.fsum(x.tolist())) <= 2.0 ** -45 * math.fsum(x.tolist())


# ---------------------------------------------------------------------------------------- the header's functions on the host
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("meshrender_host") / "meshrender_host_main")
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "meshrender_host_main.cpp"), "-o", exe]
    r = subprocess.run(base + SAN, capture_output=True, text=True)
    if r.returncode != 0:
        assert "sanitize" in r.stderr or "asan" in r.stderr or "ubsan" in r.stderr, r.stderr      # only a failed sanitizer link falls back
        subprocess.run(base, check=True)
    return exe


def run_program(program, tmp_path, v, f, poses, h, w, intr, near=0., far=np.inf, cull=0, shading=0, colors=None, normals=None, bg=(0., 0., 0.)):
    V, F, N = len(v), len(f), len(poses)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([V, F, N, h, w, cull, shading, colors is not None, normals is not None, 0], np.int32).tobytes())
        fh.write(np.array(list(intr) + [near, far] + list(bg), np.float32).tobytes())
        fh.write(np.ascontiguousarray(v, np.float32).tobytes() + np.ascontiguousarray(f, np.int32).tobytes())
        for a in (colors, normals):
            if a is not None:
                fh.write(np.ascontiguousarray(a, np.float32).tobytes())
        fh.write(np.ascontiguousarray(poses, np.float32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, r.stderr[-3000:]
    raw = open(tmp_path / "out.bin", "rb").read()
    P = N * h * w
    out, at = dict(counts=np.frombuffer(raw, np.int64, 4, 0)), 32
    for name, dtype, k in (("face", np.int32, 1), ("depth", np.float32, 1), ("disp", np.float32, 1), ("acc", np.float32, 1), ("bary", np.float32, 3),
                           ("rgb", np.float32, 3)):
        out[name] = np.frombuffer(raw, dtype, k * P, at).reshape((N, h * w) + ((3,) if k == 3 else ()))
        at += 4 * k * P
    assert at == len(raw)
    return out


def same(got, want, rgb=True):
    assert got["counts"].tolist() == want["counts"].tolist()
    assert np.array_equal(got["face"], want["face"])
    for k in ("depth", "disp", "acc", "bary") + (("rgb",) if rgb else ()):
        assert got[k].tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("name", sorted(CASES))
def test_header_functions_equal_the_replay_bit_for_bit(program, tmp_path, name):
    v, f, poses = CASES[name]
    intr = M.intrinsics(H, W, focal=FOCAL)
    col = M.vertex_colors(v)
    kw = dict(colors=col, bg=(0.25, 0.5, 1.0))
    same(run_program(program, tmp_path, v, f, poses, H, W, intr, **kw), M.render(v, f, H, W, intr, poses, colors=col, background=(0.25, 0.5, 1.0)))


@pytest.mark.parametrize("shading", [1, 2])
@pytest.mark.parametrize("name", ["sphere", "cut_sphere", "straddles"])
def test_header_shading_modes(program, tmp_path, name, shading):
    v, f, poses = CASES[name]
    intr = M.intrinsics(H, W, focal=FOCAL)
    nor = R.vertex_normals(v, f).astype(np.float32)
    col = M.vertex_colors(v) if name != "cut_sphere" else None
    same(run_program(program, tmp_path, v, f, poses, H, W, intr, shading=shading, colors=col, normals=nor),
         M.render(v, f, H, W, intr, poses, shading=shading, colors=col, normals=nor))


@pytest.mark.parametrize("kw", [dict(cull=1), dict(cull=2), dict(near=2.0, far=2.3), dict(near=0.0, far=2.1), dict(near=2.2)])
def test_header_windows_and_culling(program, tmp_path, kw):
    v, f, poses = CASES["sphere"]
    intr = M.intrinsics(H, W, focal=FOCAL)
    col = M.vertex_colors(v)
    want = M.render(v, f, H, W, intr, poses, colors=col, **kw)
    same(run_program(program, tmp_path, v, f, poses, H, W, intr, colors=col, **kw), want)
    full = M.render(v, f, H, W, intr, poses, colors=col, want_counts=False)
    assert 0 < want["acc"].sum() and 0 < want["counts"][3] < full["counts"][3]         # the window or the culling drops hits
    assert np.array_equal(want["face"], full["face"]) == (kw == dict(cull=1))


def test_header_with_a_pinhole_matrix_and_an_odd_image(program, tmp_path):
    """K with its own centre and two focal lengths, an image that is no multiple of anything, a camera inside the torus' hole"""
    v, f, _ = CASES["torus"]
    h, w = 37, 53
    intr = M.intrinsics(h, w, K=[[70.5, 0, 20.25], [0, 64.0, 21.5], [0, 0, 1]])
    poses = np.stack([M.pose(0.9, 0.2, 0.05, M.box_centre(v)), M.pose(-1.1, 1.3, 1.4, M.box_centre(v))])
    col = M.vertex_colors(v)
    want = M.render(v, f, h, w, intr, poses, colors=col)
    assert want["counts"][2] > 0 and 0 < want["acc"].sum()
    same(run_program(program, tmp_path, v, f, poses, h, w, intr, colors=col), want)


def test_header_whole_image_boxes_for_a_rotation_that_is_not_orthonormal(program, tmp_path):
    v, f, poses = CASES["sphere"]
    intr = M.intrinsics(H, W, focal=FOCAL)
    p = poses[:1].copy()
    p[0, :3, :3] *= np.float32(1.05)
    p[0, 0, 1] += np.float32(0.1)
    assert not M.view_boxes(p[0, :3, :3], intr[0], intr[1], H, W) and M.view_boxes(poses[0, :3, :3], intr[0], intr[1], H, W)
    col = M.vertex_colors(v)
    want = M.render(v, f, H, W, intr, p, colors=col)
    assert want["counts"][2] == len(f) and want["acc"].sum() > 100
    same(run_program(program, tmp_path, v, f, p, H, W, intr, colors=col), want)
