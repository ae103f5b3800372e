"""Out-of-bounds guard for the Laplacian-pyramid entry points: tools/tight_buffer_check_pyramid.py runs swnerf_pyramid_down
(k = 3, 5), swnerf_pyramid_up_axpy (with and without a base, and at equal sizes) and swnerf_pyramid_up_adjoint on ragged odd
sizes (17 x 31, 9 x 13, 37 x 53) with operands and outputs that end where their allocation ends, so a blur tap, a `+1`
neighbour or a 4-float run past the last element faults.  A fresh child process, started before this pytest process has
initialised the GPU (this module sorts in front of test_00_bench_launcher.py, whose last test initialises the GPU
in-process)."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOL = os.path.join(ROOT, "tools", "tight_buffer_check_pyramid.py")
CASES = ["down_k3", "down_k5", "up_axpy_base", "up_axpy_nobase", "up_axpy_same_size", "up_adjoint"]


def test_every_pyramid_case_is_run():
    from swnerf import pyramid  # noqa: F401  (the cases are the entry points of swnerf.pyramid)
    cases = subprocess.run([sys.executable, TOOL, "list"], capture_output=True, text=True, timeout=60).stdout.split()
    assert sorted(cases) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_pyramid_entry_points_on_tight_allocations():
    from swnerf import pyramid  # noqa: F401
    if torch.cuda.is_initialized():
        pytest.skip("the GPU is already initialised in this process: starting programs from it is not allowed on this pool")
    r = subprocess.run([sys.executable, TOOL] + CASES, capture_output=True, text=True, timeout=500)
    out = r.stdout + r.stderr
    assert "Memory access fault" not in out and "HSA_STATUS_ERROR" not in out, out[-3000:]
    assert r.returncode == 0, out[-3000:]
    for c in CASES:
        assert f"{c}: ok" in r.stdout, (c, out[-2000:])
