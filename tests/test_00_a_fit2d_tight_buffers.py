"""Out-of-bounds guard for the 2-D fitting entry points: tools/tight_buffer_check_fit2d.py runs swnerf_encode2d (N = 1961), the
BatchNorm kernels at (33, 257) and (513, 96) - both sides of the one-launch threshold -, swnerf_fit2d_loss (M = 33),
swnerf_pack_fit2d, swnerf_fit2d_forward at M = 1 / 31 / 33 / 1961 with rows of 96 floats holding 82 columns, and
swnerf_fit2d_picture at 53 x 37 to floats, to bytes and to both, with operands and outputs that end where their allocation
ends.  A fresh child process, started before this pytest process has initialised the GPU (this module sorts in front of
test_00_bench_launcher.py, whose last test initialises the GPU in-process)."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOL = os.path.join(ROOT, "tools", "tight_buffer_check_fit2d.py")
CASES = ["encode", "bn_forward", "bn_backward", "bn_apply", "loss", "pack", "forward", "picture_f32", "picture_u8", "picture_both"]


def test_every_fit2d_case_is_run():
    from swnerf import fit2d  # noqa: F401  (the cases are the entry points behind swnerf.fit2d)
    cases = subprocess.run([sys.executable, TOOL, "list"], capture_output=True, text=True, timeout=60).stdout.split()
    assert sorted(cases) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_fit2d_entry_points_on_tight_allocations():
    from swnerf import fit2d  # noqa: F401
    if torch.cuda.is_initialized():
        pytest.skip("the GPU is already initialised in this process: starting programs from it is not allowed on this pool")
    r = subprocess.run([sys.executable, TOOL] + CASES, capture_output=True, text=True, timeout=500)
    out = r.stdout + r.stderr
    assert "Memory access fault" not in out and "HSA_STATUS_ERROR" not in out, out[-3000:]
    assert r.returncode == 0, out[-3000:]
    for c in CASES:
        assert f"{c}: ok" in r.stdout, (c, out[-2000:])
