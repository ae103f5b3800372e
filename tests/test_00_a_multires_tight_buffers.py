"""Out-of-bounds guard for the MultiRes training entry points: tools/tight_buffer_check_multires.py runs swnerf_patch_batch (40 x 56
with 8 / 4 / 2 / 1 patches that end at the last pixel of every level, 36 x 52 with a corner that clips levels 2 and 3, 12 x 20 with
2 levels that are their own patches; the first and the last frame) and swnerf_multires_loss with and without rgb0 and the global
term (patch sizes 8/4/2/1, 32/16/7x7/3x3, 12x20/6x10 and one level of 5x3), with operands and outputs that end where their
allocation ends.  A fresh child process with a time limit of its own, started before this pytest process has initialised the GPU
(this module sorts in front of test_00_bench_launcher.py, whose last test initialises the GPU in-process)."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOL = os.path.join(ROOT, "tools", "tight_buffer_check_multires.py")
CASES = ["patch_batch", "loss", "loss_rgb0"]


def test_every_multires_case_is_run():
    from swnerf import batching
    assert hasattr(batching, "PatchBatcher") and hasattr(batching, "multires_loss")      # the cases are the entry points behind them
    cases = subprocess.run([sys.executable, TOOL, "list"], capture_output=True, text=True, timeout=60).stdout.split()
    assert sorted(cases) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_multires_entry_points_on_tight_allocations():
    from swnerf import batching  # noqa: F401
    if torch.cuda.is_initialized():
        pytest.skip("the GPU is already initialised in this process: starting programs from it is not allowed on this pool")
    r = subprocess.run([sys.executable, TOOL] + CASES, capture_output=True, text=True, timeout=240)
    out = r.stdout + r.stderr
    assert "Memory access fault" not in out and "HSA_STATUS_ERROR" not in out, out[-3000:]
    assert r.returncode == 0, out[-3000:]
    for c in CASES:
        assert f"{c}: ok" in r.stdout, (c, out[-2000:])
