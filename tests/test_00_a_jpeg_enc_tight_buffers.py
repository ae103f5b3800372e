"""Out-of-bounds guard for swnerf_jpeg_encode: tools/tight_buffer_check_jpeg_enc.py runs it at 1 x 1, 17 x 23 and 257 x 9, 4:2:0 and
4:4:4, on uint8 and float32 frames of 3 and 4 channels, with frames, tables, scratch planes and coefficients that end where their
allocation ends, so a pixel read past the last frame, an 8-byte load past the last plane row or a 16-byte store past the last
block faults.  The same inputs pass through the stand-alone host program under AddressSanitizer first
(tests/test_jpeg_enc_host.py::test_host_program_on_the_sizes_of_the_tight_allocation_tool).  A fresh child process with a time limit,
started before this pytest process has initialised the GPU (this module sorts in front of test_00_bench_launcher.py, whose last
test initialises the GPU in-process)."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOL = os.path.join(ROOT, "tools", "tight_buffer_check_jpeg_enc.py")
CASES = [f"encode_{s}_{t}_c{c}" for s in ("420", "444") for t in ("u8", "f32") for c in (3, 4)]


def test_every_jpeg_encode_case_is_run():
    from swnerf import images  # noqa: F401  (the cases are the entry point behind swnerf.images.encode_jpegs)
    cases = subprocess.run([sys.executable, TOOL, "list"], capture_output=True, text=True, timeout=60).stdout.split()
    assert sorted(cases) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_jpeg_encode_on_tight_allocations():
    from swnerf import images  # noqa: F401
    if torch.cuda.is_initialized():
        pytest.skip("the GPU is already initialised in this process: starting programs from it is not allowed on this pool")
    r = subprocess.run([sys.executable, TOOL] + CASES, capture_output=True, text=True, timeout=500)
    out = r.stdout + r.stderr
    assert "Memory access fault" not in out and "HSA_STATUS_ERROR" not in out, out[-3000:]
    assert r.returncode == 0, out[-3000:]
    for c in CASES:
        assert f"{c}: ok" in r.stdout, (c, out[-2000:])
