"""Out-of-bounds guard for the fused optimizer step: tools/tight_buffer_check_optim.py runs swnerf_adam_step on tensors whose p, g,
m and v end where their allocation ends - the vector path on sizes that are multiples of 4, the vector path's masked tail in front
of a sentinel, the scalar path from unaligned starts (1, 3, 255, 256, 257, 4099 floats), and a list over the tensor cap in two
launches - and compares every result with the same call on ordinary allocations, bit for bit.  A fresh child process, started
before this pytest process has initialised the GPU (this module sorts in front of test_00_bench_launcher.py, whose last test
initialises the GPU in-process)."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOL = os.path.join(ROOT, "tools", "tight_buffer_check_optim.py")
CASES = ["vec", "vec_ragged", "scalar", "multi"]


def test_every_optim_case_is_run():
    from swnerf import optim  # noqa: F401  (the cases are the entry point behind swnerf.optim)
    cases = subprocess.run([sys.executable, TOOL, "list"], capture_output=True, text=True, timeout=60).stdout.split()
    assert sorted(cases) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_adam_step_on_tight_allocations():
    from swnerf import optim  # noqa: F401
    if torch.cuda.is_initialized():
        pytest.skip("the GPU is already initialised in this process: starting programs from it is not allowed on this pool")
    r = subprocess.run([sys.executable, TOOL] + CASES, capture_output=True, text=True, timeout=240)
    out = r.stdout + r.stderr
    assert "Memory access fault" not in out and "HSA_STATUS_ERROR" not in out, out[-3000:]
    assert r.returncode == 0, out[-3000:]
    for c in CASES:
        assert f"{c}: ok" in r.stdout, (c, out[-2000:])
