"""Out-of-bounds guard for the T-NeRF entry points: tools/tight_buffer_check_tnerf.py runs swnerf_pack_net (kind 3), the fused
T-NeRF pass with every optional input and output set (stratified and given depths), swnerf_linear_act with ELU and
swnerf_elu_grad on operands and outputs that end where their allocation ends, so a read or write past the last element
faults.  A fresh child process, started before this pytest process has initialised the GPU (this module sorts in front of
test_00_bench_launcher.py, whose last test initialises the GPU in-process)."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOL = os.path.join(ROOT, "tools", "tight_buffer_check_tnerf.py")
CASES = ["pack", "pass_coarse", "pass_zvals", "elu_gemm"]


def test_every_tnerf_case_is_run():
    cases = subprocess.run([sys.executable, TOOL, "list"], capture_output=True, text=True, timeout=60).stdout.split()
    assert sorted(cases) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_tnerf_entry_points_on_tight_allocations():
    if torch.cuda.is_initialized():
        pytest.skip("the GPU is already initialised in this process: starting programs from it is not allowed on this pool")
    r = subprocess.run([sys.executable, TOOL] + CASES, capture_output=True, text=True, timeout=500)
    out = r.stdout + r.stderr
    assert "Memory access fault" not in out and "HSA_STATUS_ERROR" not in out, out[-3000:]
    assert r.returncode == 0, out[-3000:]
    for c in CASES:
        assert f"{c}: ok" in r.stdout, (c, out[-2000:])
