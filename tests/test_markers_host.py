"""swnerf.markers on the host: the geometry against recordings of the reference (tests/golden/g21_markers.npz), payload
matching, transform_mesh, and the numpy replay of the detector on the fixture set (the condition that the set is sound)."""
import os

import numpy as np
import pytest

import marker_ref as R
from swnerf import markers, mesh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_markers.npz")
KEYS = ("fl_x", "fl_y", "cx", "cy", "k1", "k2", "p1", "p2")


@pytest.fixture(scope="module")
def g21():
    return dict(np.load(GOLDEN, allow_pickle=False))


def test_reference_convention_matches_recordings(g21):
    intr = dict(zip(KEYS, g21["intrinsics"]))
    np.testing.assert_allclose(markers.undistort_points(g21["undistort_in"], *g21["intrinsics"][4:]), g21["undistort_out"], rtol=0, atol=1e-15)
    for c, T, rays in zip(g21["corners"], g21["poses"], g21["rays"]):
        np.testing.assert_allclose(markers.ray_directions(c[0], T, intr, "reference"), rays, rtol=0, atol=1e-14)
    world = markers.triangulate_corners(g21["corners"][:, 0], g21["poses"], intr, convention="reference")
    dist = np.linalg.norm(world - g21["least_squares_world"], axis=1)
    print("closed form vs least_squares:", dist, "stored:", g21["closed_form_distance"])
    assert g21["closed_form_distance"].max() < 1e-5 * float(g21["edge"])
    assert np.all(dist <= 10 * g21["closed_form_distance"].max())
    for c, M in zip(g21["transform_in"], g21["transform_out"]):
        np.testing.assert_allclose(markers.calculate_transform_matrix(c), M, rtol=0, atol=1e-13)


def test_conventions_differ(g21):
    intr = dict(zip(KEYS, g21["intrinsics"]))
    a = markers.triangulate_corners(g21["corners"][:, 0], g21["poses"], intr, convention="reference")
    b = markers.triangulate_corners(g21["corners"][:, 0], g21["poses"], intr, convention="nerf")
    assert np.abs(a - b).max() > float(g21["edge"])


def test_nerf_convention_recovers_exact_projections():
    s = R.make_scene(noise=0.)
    intr = dict(fl_x=s["fx"], fl_y=s["fy"], cx=s["cx"], cy=s["cy"])
    world = markers.triangulate_corners(s["uv"], s["poses"], intr, convention="nerf")
    err = np.abs(world - s["corners3d"]).max()
    print("nerf triangulation error / edge:", err / s["edge"])
    assert err < 1e-9 * s["edge"]
    assert abs(markers.mean_edge_length(world) - s["edge"]) < 1e-9 * s["edge"]


@pytest.mark.parametrize("normal", [(0, 0, 1), (0, 0, -1), (0, 1e-9, -1), (1, 2, 3), (-1, 0.5, -2)])
def test_transform_matrix_takes_normal_to_z(normal):
    n = np.asarray(normal, np.float64)
    n /= np.linalg.norm(n)
    a = np.cross(n, [1., 0.3, 0.2])
    a /= np.linalg.norm(a)
    b = np.cross(n, a)                                                       # a x b = n
    corners = np.array([0 * a, a, a + b, b]) * 0.08 + 0.3
    assert np.allclose(np.cross(corners[1] - corners[0], corners[2] - corners[0]) / 0.08 ** 2, n)
    M = markers.calculate_transform_matrix(corners)
    assert np.all(np.isfinite(M))
    np.testing.assert_allclose(M[:3, :3] @ n, [0, 0, 1], atol=1e-8)
    np.testing.assert_allclose(M[:3, :3] @ M[:3, :3].T, np.eye(3), atol=1e-8)
    assert np.linalg.det(M[:3, :3]) > 0 and np.array_equal(M[3], [0, 0, 0, 1]) and np.array_equal(M[:3, 3], [0, 0, 0])


def test_transform_mesh_obj_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    v = rng.normal(size=(12, 3)).astype(np.float32)
    vn = rng.normal(size=(12, 3)).astype(np.float32)
    vn /= np.linalg.norm(vn, axis=1, keepdims=True)
    col = rng.uniform(0, 1, (12, 3)).astype(np.float32)
    f = rng.integers(0, 12, (7, 3)).astype(np.int32)
    src, dst = str(tmp_path / "mesh.obj"), str(tmp_path / "transformed_mesh.obj")
    mesh.Mesh(v, f, vn, col).export(src)
    M = markers.calculate_transform_matrix(np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0.5], [0, 1, 0.5]], np.float64))
    M[:3, 3] = [0.1, -0.2, 0.3]
    markers.transform_mesh(src, dst, 3.7, M)
    v2, f2, vn2, col2 = mesh.load_obj(dst)
    want = (v.astype(np.float64) * 3.7) @ M[:3, :3].T + M[:3, 3]             # scale first, then the rigid motion
    np.testing.assert_allclose(v2, want, rtol=0, atol=4e-7 * np.abs(want).max())
    np.testing.assert_allclose(vn2, vn.astype(np.float64) @ M[:3, :3].T, rtol=0, atol=3e-7)
    np.testing.assert_allclose(np.linalg.norm(vn2, axis=1), 1, atol=1e-6)
    assert np.array_equal(f2, f) and np.array_equal(col2, mesh.load_obj(src)[3])


def test_payload_rotations_canonical_and_dictionary():
    rng = np.random.default_rng(5)
    entries = [R.payload_of(R.random_bits(rng)) for _ in range(6)]
    table = markers.dictionary_table(np.array(entries, np.uint16))
    assert markers.dictionary_table(np.stack([markers.payload_bits(e) for e in entries])) == table
    for i, e in enumerate(entries):
        ident0, k0 = markers.canonical_payload(e)
        for k in range(4):
            seen = R.rotate_payload(e, k)                                    # what the detector reads when its corner 0 is corner k
            assert markers.payload_rotations(e)[k] == seen
            ident, kc = markers.canonical_payload(seen)
            assert ident == ident0 and (k + kc) % 4 == k0                    # the same physical corner whatever the start
            idx, kd = markers.match_dictionary(seen, table)
            assert idx == i and (k + kd) % 4 == 0                            # the entry's top-left
    assert markers.match_dictionary(0x1000, {0x8000: 0}) == (0, 1)            # the white cell sits at corner 1
    assert markers.match_dictionary(0x0001, {0x8000: 0}) == (0, 2)
    assert markers.match_dictionary(0x0001, {0x1234: 0}) == (None, None)
    half_turn = np.array([[1, 0, 0, 1], [0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 1]])
    assert np.array_equal(np.rot90(half_turn, 2), half_turn)
    assert markers.canonical_payload(markers.bits_payload(half_turn)) == (None, None)
    assert markers.canonical_payload(0xFFFF) == (None, None)


@pytest.fixture(scope="module")
def fixture_set():
    return R.fixture_frames()


def test_replay_on_fixture_set(fixture_set):
    frames, quads, payloads = fixture_set
    assert frames.shape == (80, 240, 320)
    errs = []
    for k in range(len(frames)):
        side = np.linalg.norm(quads[k] - np.roll(quads[k], -1, axis=0), axis=1)
        assert 12 <= quads[k].min() and quads[k][:, 0].max() <= 320 - 12 and quads[k][:, 1].max() <= 240 - 12
        assert 20 * 0.7 <= side.min() and side.max() <= 84 * 1.3
        found = R.detect(frames[k])
        assert len(found) == 1, f"frame {k}: {len(found)} markers"
        q, p = found[0]
        rot = R.match_rotation(q, quads[k])
        assert p == R.rotate_payload(payloads[k], rot), f"frame {k}: payload"
        errs.append(np.linalg.norm(q - np.roll(quads[k], -rot, axis=0), axis=1).max())
    print(f"replay: worst corner error {max(errs):.4f} px, mean {np.mean(errs):.4f} px")
    assert max(errs) <= 0.5


def test_replay_labels_are_component_minima():
    rng = np.random.default_rng(11)
    mask = (rng.uniform(size=(37, 53)) < 0.45).astype(np.uint8)
    lab = R.label(mask)
    assert np.array_equal(lab < 0, mask == 0)
    seen = {}
    for i in range(37):                                                     # flood fill as the independent definition
        for j in range(53):
            if mask[i, j] and (i, j) not in seen:
                stack, comp = [(i, j)], []
                seen[(i, j)] = True
                while stack:
                    y, x = stack.pop()
                    comp.append(y * 53 + x)
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            yy, xx = y + dy, x + dx
                            if 0 <= yy < 37 and 0 <= xx < 53 and mask[yy, xx] and (yy, xx) not in seen:
                                seen[(yy, xx)] = True
                                stack.append((yy, xx))
                assert all(lab.reshape(-1)[p] == min(comp) for p in comp)
