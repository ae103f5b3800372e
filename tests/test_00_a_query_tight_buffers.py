"""Out-of-bounds guard for the grid query of the time-conditioned nets: tools/tight_buffer_check_query.py runs
swnerf_query_points_time (D-NeRF with and without the deformation pass, T-NeRF) on a packed blob, points, directions and outputs
that end where their allocation ends, so a read or write past the last element faults.  A fresh child process, started before
this pytest process has initialised the GPU (this module sorts in front of test_00_bench_launcher.py, whose last test
initialises the GPU in-process)."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOL = os.path.join(ROOT, "tools", "tight_buffer_check_query.py")
CASES = ["query_dnerf", "query_dnerf_t0", "query_tnerf"]


def test_every_query_case_is_run():
    cases = subprocess.run([sys.executable, TOOL, "list"], capture_output=True, text=True, timeout=60).stdout.split()
    assert sorted(cases) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_query_entry_point_on_tight_allocations():
    if torch.cuda.is_initialized():
        pytest.skip("the GPU is already initialised in this process: starting programs from it is not allowed on this pool")
    r = subprocess.run([sys.executable, TOOL] + CASES, capture_output=True, text=True, timeout=500)
    out = r.stdout + r.stderr
    assert "Memory access fault" not in out and "HSA_STATUS_ERROR" not in out, out[-3000:]
    assert r.returncode == 0, out[-3000:]
    for c in CASES:
        assert f"{c}: ok" in r.stdout, (c, out[-2000:])
