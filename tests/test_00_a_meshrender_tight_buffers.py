"""Out-of-bounds guard for the mesh-rendering entry points: tools/tight_buffer_check_meshrender.py runs swnerf_mesh_render_raster,
_render_resolve and swnerf_mesh_view_compare on one triangle over a 5 x 3 image, on the 360 / 716 sphere from three views at 48 x 40
and on that sphere with a last face that straddles the camera plane, with operands, outputs and z-buffer that end where their
allocation ends, so a pixel one past the image or an index one past V or F faults.  A fresh child process, started before this pytest
process has initialised the GPU (this module sorts in front of test_00_bench_launcher.py, whose last test initialises the GPU
in-process)."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOL = os.path.join(ROOT, "tools", "tight_buffer_check_meshrender.py")
CASES = [f"{c}-{s}" for c in ("raster", "resolve", "compare") for s in ("tri_5x3", "sphere_3views", "straddle_last")]


def test_every_meshrender_case_is_run():
    from swnerf import meshrender  # noqa: F401  (the cases are the entry points of swnerf.meshrender)
    cases = subprocess.run([sys.executable, TOOL, "list"], capture_output=True, text=True, timeout=60).stdout.split()
    assert sorted(cases) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_meshrender_entry_points_on_tight_allocations():
    from swnerf import meshrender  # noqa: F401
    if torch.cuda.is_initialized():
        pytest.skip("the GPU is already initialised in this process: starting programs from it is not allowed on this pool")
    r = subprocess.run([sys.executable, TOOL] + CASES, capture_output=True, text=True, timeout=500)
    out = r.stdout + r.stderr
    assert "Memory access fault" not in out and "HSA_STATUS_ERROR" not in out, out[-3000:]
    assert r.returncode == 0, out[-3000:]
    for c in CASES:
        assert f"{c}: ok" in r.stdout, (c, out[-2000:])
