"""Out-of-bounds guard for the mesh hole-filling entry points: tools/tight_buffer_check_meshfill.py runs swnerf_mesh_boundary,
_boundary_loops and _fill_emit at (V, F) = (3, 1), an open tetrahedron (4, 3) and the 360 / 358 open sphere with operands, outputs
and workspace that end where their allocation ends, so an access wider than an element at the last row, or an index one past V, F,
3 F or the number of boundary half-edges, faults.  A fresh child process, started before this pytest process has initialised the
GPU (this module sorts in front of test_00_bench_launcher.py, whose last test initialises the GPU in-process)."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOL = os.path.join(ROOT, "tools", "tight_buffer_check_meshfill.py")
CASES = [f"{c}-{s}" for c in ("boundary", "loops", "emit") for s in ("v3f1", "tet_open", "open_sphere")]


def test_every_meshfill_case_is_run():
    from swnerf import meshops  # noqa: F401  (the cases are the entry points of swnerf.meshops)
    cases = subprocess.run([sys.executable, TOOL, "list"], capture_output=True, text=True, timeout=60).stdout.split()
    assert sorted(cases) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_meshfill_entry_points_on_tight_allocations():
    from swnerf import meshops  # noqa: F401
    if torch.cuda.is_initialized():
        pytest.skip("the GPU is already initialised in this process: starting programs from it is not allowed on this pool")
    r = subprocess.run([sys.executable, TOOL] + CASES, capture_output=True, text=True, timeout=500)
    out = r.stdout + r.stderr
    assert "Memory access fault" not in out and "HSA_STATUS_ERROR" not in out, out[-3000:]
    assert r.returncode == 0, out[-3000:]
    for c in CASES:
        assert f"{c}: ok" in r.stdout, (c, out[-2000:])
