"""Out-of-bounds guard for the dataset image entry points: tools/tight_buffer_check_images.py runs swnerf_png_unfilter (bpp 3
and 4 at 1 x 1, 17 x 31 and 257 x 9: rows of 1 + W * bpp bytes, nothing aligned, a second row band) and swnerf_area_resize
(uint8 and float32, 3 and 4 channels, a 2x and a fractional factor) with operands and outputs that end where their allocation
ends, so a load wider than a byte at the last pixel, or a footprint cell past the last row, faults.  A fresh child process,
started before this pytest process has initialised the GPU (this module sorts in front of test_00_bench_launcher.py, whose last
test initialises the GPU in-process)."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOL = os.path.join(ROOT, "tools", "tight_buffer_check_images.py")
CASES = ["unfilter_bpp3", "unfilter_bpp4"] + [f"resize_{t}_c{c}_{k}" for t in ("u8", "f32") for c in (3, 4) for k in ("2x", "frac")]


def test_every_images_case_is_run():
    from swnerf import images  # noqa: F401  (the cases are the entry points of swnerf.images)
    cases = subprocess.run([sys.executable, TOOL, "list"], capture_output=True, text=True, timeout=60).stdout.split()
    assert sorted(cases) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_image_entry_points_on_tight_allocations():
    from swnerf import images  # noqa: F401
    if torch.cuda.is_initialized():
        pytest.skip("the GPU is already initialised in this process: starting programs from it is not allowed on this pool")
    r = subprocess.run([sys.executable, TOOL] + CASES, capture_output=True, text=True, timeout=500)
    out = r.stdout + r.stderr
    assert "Memory access fault" not in out and "HSA_STATUS_ERROR" not in out, out[-3000:]
    assert r.returncode == 0, out[-3000:]
    for c in CASES:
        assert f"{c}: ok" in r.stdout, (c, out[-2000:])
