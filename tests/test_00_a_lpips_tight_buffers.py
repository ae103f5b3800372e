"""Out-of-bounds guard for the LPIPS entry points: tools/tight_buffer_check_lpips.py runs swnerf_conv2d_pack,
swnerf_conv2d_nhwc (16-byte and 4-byte gathers, both column tiles, ragged pixel / channel / K counts, windows over every
border), swnerf_maxpool2d_nhwc and swnerf_lpips_layer on operands, workspace and outputs that end where their allocation ends,
so a read or write past the last element faults.  A fresh child process, started before this pytest process has initialised
the GPU (this module sorts in front of test_00_bench_launcher.py, whose last test initialises the GPU in-process)."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOL = os.path.join(ROOT, "tools", "tight_buffer_check_lpips.py")
CASES = ["pack", "conv_vec", "conv_scalar", "pool", "layer"]


def test_every_lpips_case_is_run():
    cases = subprocess.run([sys.executable, TOOL, "list"], capture_output=True, text=True, timeout=60).stdout.split()
    assert sorted(cases) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_lpips_entry_points_on_tight_allocations():
    if torch.cuda.is_initialized():
        pytest.skip("the GPU is already initialised in this process: starting programs from it is not allowed on this pool")
    r = subprocess.run([sys.executable, TOOL] + CASES, capture_output=True, text=True, timeout=500)
    out = r.stdout + r.stderr
    assert "Memory access fault" not in out and "HSA_STATUS_ERROR" not in out, out[-3000:]
    assert r.returncode == 0, out[-3000:]
    for c in CASES:
        assert f"{c}: ok" in r.stdout, (c, out[-2000:])
