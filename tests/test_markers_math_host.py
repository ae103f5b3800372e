"""csrc/marker_math.h on the host: tests/marker_host_main.cpp - a stand-alone program that loops the header's functions over
exact-size heap buffers - is built here with g++ under AddressSanitizer and UBSan (without them when the sanitizer runtime cannot
be linked) and compared with the numpy replay of tests/marker_ref.py: the threshold bit for bit, refinement in double to round-off
and in float within the gate of tests/test_gpu_markers.py (the device runs the same float code)."""
import os
import subprocess

import numpy as np
import pytest

import marker_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "sw-nerf_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
FLOAT_GATE = 4 * 4.612e-5                 # test_gpu_markers.REFINE_GATE: fp32 bilinear and line-fit round-off, measured on the device
DOUBLE_GATE = 1e-9                        # the same formulae in float64 on coordinates below 320: round-off through a line fit


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("marker_host") / "marker_host_main")
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "marker_host_main.cpp"), "-o", exe]
    r = subprocess.run(base + SAN, capture_output=True, text=True)
    if r.returncode != 0:
        assert "sanitize" in r.stderr or "asan" in r.stderr or "ubsan" in r.stderr, r.stderr      # only a failed sanitizer link falls back
        subprocess.run(base, check=True)
    return exe


def _run(program, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program, *args], capture_output=True, text=True, timeout=120, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("r", [11, 41])
def test_threshold_functions_equal_the_replay(program, tmp_path, r):
    rng = np.random.default_rng(r)
    q = np.array([[12., 9.], [50., 14.], [46., 52.], [8., 47.]])
    g = R.render_marker(37, 61, [q], [R.random_bits(rng)], noise=6., seed=r)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array(g.shape, np.int32).tobytes() + g.tobytes())
    _run(program, "mask", str(tmp_path / "in.bin"), str(r), "7", str(tmp_path / "out.bin"))
    got = np.fromfile(tmp_path / "out.bin", np.uint8).reshape(g.shape)
    assert 0 < got.sum() < got.size and np.array_equal(got, R.dark_mask(g, r, 7))


def test_refinement_in_double_and_float_against_the_replay(program, tmp_path):
    frames, quads, payloads = R.fixture_frames(count=12)                    # sides 20 .. 84 px
    worst = {"d": 0., "f": 0.}
    for k, g in enumerate(frames):
        cand = R.detect_radius(g, 11)[2]
        corners = np.ascontiguousarray(cand[:, 3:], np.int32)               # flagged ones too: they must end in a status, not a fault
        edge = np.array([[0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 319, 0, 319, 239, 0, 239], [5, 5, 5, 5, 5, 5, 5, 5]], np.int32)
        corners = np.concatenate([corners, edge])
        with open(tmp_path / "in.bin", "wb") as f:
            f.write(np.array(g.shape + (len(corners),), np.int32).tobytes() + g.tobytes() + corners.tobytes())
        lines = _run(program, "refine", str(tmp_path / "in.bin")).split("\n")
        found = 0
        for i, c in enumerate(corners):
            want = R.refine(g, c.reshape(4, 2).astype(np.float64) + 0.5)
            for line in lines[2 * i:2 * i + 2]:
                t = line.split()
                payload, q = int(t[1]), np.array([float(v) for v in t[2:]]).reshape(4, 2)
                assert (payload < 0) == (want is None), f"frame {k}, candidate {i}, {t[0]}"
                if want is not None:
                    assert payload == want[1]
                    worst[t[0]] = max(worst[t[0]], np.abs(q - want[0]).max())
            found += want is not None
        assert found >= 1, f"frame {k}"
    print(f"marker_math.h against the replay: double {worst['d']:.3e} px, float {worst['f']:.3e} px")
    assert worst["d"] <= DOUBLE_GATE and worst["f"] <= FLOAT_GATE
