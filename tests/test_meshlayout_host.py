"""The workspaces of the three mesh units without a GPU: the byte counts that swnerf_mesh_workspace_bytes,
swnerf_mesh_simplify_workspace_bytes and swnerf_mesh_fill_workspace_bytes report, as literals, and the layouts of
csrc/meshops_layout.h on the host - tests/meshlayout_host_main.cpp, a stand-alone program that carves every layout from a heap block
of exactly the reported size and writes the ends of every array, is built with g++ under AddressSanitizer and UBSan (without them
when the sanitizer runtime cannot be linked, as tests/test_meshops_host.py does)."""
import os
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "sw-nerf_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

# (V, F): mesh, simplify, fill - the values of the formulas these functions had before the layouts were written once
BYTES = {
    (0, 0): (12032, 3584, 2560),
    (257, 85): (15360, 22016, 9728),
    (360, 716): (18688, 41216, 61696),
    (369654, 674416): (7155200, 38871552, 56684032),
    (3699905, 6709002): (71351552, 362620672, 563871744),
    (2 ** 31 - 1, (2 ** 31 - 1) // 3): (28666680576, 114566016256, 60163097344),
}


def test_workspace_bytes_are_the_literal_values():
    from swnerf import _lib
    L = _lib.lib()
    for (V, F), want in BYTES.items():
        got = (L.swnerf_mesh_workspace_bytes(V, F), L.swnerf_mesh_simplify_workspace_bytes(V, F), L.swnerf_mesh_fill_workspace_bytes(V, F))
        assert got == want, (V, F)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("meshlayout_host") / "meshlayout_host_main")
    base = ["g++", "-O1", "-g", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tests", "meshlayout_host_main.cpp"), "-o", exe]
    r = subprocess.run(base + SAN, capture_output=True, text=True)
    if r.returncode != 0:
        assert "sanitize" in r.stderr or "asan" in r.stderr or "ubsan" in r.stderr, r.stderr      # only a failed sanitizer link falls back
        subprocess.run(base, check=True)
    return exe


def test_every_layout_fits_the_size_it_reports(program):
    from swnerf import _lib
    L = _lib.lib()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([program], capture_output=True, text=True, timeout=120, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [(name, int(V), int(F), int(b)) for name, V, F, b in (line.split() for line in r.stdout.splitlines())]
    sizes = [(1, 1), (3, 1), (257, 85), (360, 716)]
    assert [(n, V, F) for n, V, F, _ in rows] == [(n, V, F) for V, F in sizes for n in ("mesh", "simplify", "fill_boundary", "fill_loops")] + [("simplify", 360, 0)]
    for name, V, F, b in rows:                                       # the library reports what the header's carving gives
        if name == "mesh":
            assert b == L.swnerf_mesh_workspace_bytes(V, F)
        elif name == "simplify":
            assert b == L.swnerf_mesh_simplify_workspace_bytes(V, F)
        else:                                                        # the fill workspace: its largest phase and 512 bytes
            assert b + 512 <= L.swnerf_mesh_fill_workspace_bytes(V, F)
