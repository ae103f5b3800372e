"""Out-of-bounds guard for the training-batch entry points: tools/tight_buffer_check_batching.py runs swnerf_perm_indices,
swnerf_train_batch in permutation and in ids mode on float32 RGB and uint8 RGBA images (3 x 37 x 53; 1, 255, 257 and 1000 rays;
rows of 8, 11 and 12 columns; the last pixel of the last image among the ids) and swnerf_photo_loss with and without rgb0
(N = 1 / 33 / 4096), with operands and outputs that end where their allocation ends.  A fresh child process, started before this
pytest process has initialised the GPU (this module sorts in front of test_00_bench_launcher.py, whose last test initialises
the GPU in-process).  examples/train_lego_like.py runs here too, at a reduced size, for the same reason: it is a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOL = os.path.join(ROOT, "tools", "tight_buffer_check_batching.py")
CASES = ["perm", "batch_perm_f32", "batch_perm_u8", "batch_ids_f32", "batch_ids_u8", "loss", "loss_rgb0"]


def test_every_batching_case_is_run():
    from swnerf import batching  # noqa: F401  (the cases are the entry points behind swnerf.batching)
    cases = subprocess.run([sys.executable, TOOL, "list"], capture_output=True, text=True, timeout=60).stdout.split()
    assert sorted(cases) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_batching_entry_points_on_tight_allocations():
    from swnerf import batching  # noqa: F401
    if torch.cuda.is_initialized():
        pytest.skip("the GPU is already initialised in this process: starting programs from it is not allowed on this pool")
    r = subprocess.run([sys.executable, TOOL] + CASES, capture_output=True, text=True, timeout=500)
    out = r.stdout + r.stderr
    assert "Memory access fault" not in out and "HSA_STATUS_ERROR" not in out, out[-3000:]
    assert r.returncode == 0, out[-3000:]
    for c in CASES:
        assert f"{c}: ok" in r.stdout, (c, out[-2000:])


@pytest.mark.gpu
@pytest.mark.timeout(400)
def test_train_example_in_a_child_process(tmp_path):
    """examples/train_lego_like.py: 3 teacher frames of 16 x 16, 20 steps of runner.train, the held-out PSNR printed."""
    if torch.cuda.is_initialized():
        pytest.skip("the GPU is already initialised in this process: starting programs from it is not allowed on this pool")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_lego_like.py"), str(tmp_path), "16", "3", "20"],
                       capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("held-out PSNR")]
    print(line)
    assert len(line) == 1 and np.isfinite(float(line[0].split()[-2])), out[-2000:]
    assert os.path.exists(os.path.join(str(tmp_path), "train_lego_like", "000020.tar"))
