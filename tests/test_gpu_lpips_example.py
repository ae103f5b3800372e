"""examples/score_render_dir.py run as written (in process): seeded weight files in both formats -> render_test with
lpips_weights (metrics.json gains "lpips") -> estim/ and gt/ PNGs -> evaluate_dir with lpips_weights (metrics.txt gains 'lpips')."""
import ast
import json
import math
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_score_render_dir_example(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import score_render_dir as ex
    m1, m2, scored = ex.main(str(tmp_path), H=48, n_poses=3)
    assert sorted(os.listdir(tmp_path / "lpips_weights")) == ["alex.pth", "alexnet-owt-7be5be79.pth", "vgg.pth", "vgg16-397923af.pth"]
    assert set(m1) == {"psnr", "ssim", "lpips"} and all(len(v) == 3 for v in m1.values())
    assert all(math.isfinite(v) and v > 0 for v in m1["lpips"]) and all(10 < v < 80 for v in m1["psnr"])
    assert json.loads(open(os.path.join(scored, "metrics.json")).read()) == m1
    assert set(m2) == {"mse", "psnr", "ssim", "lpips"} and math.isfinite(m2["lpips"]) and m2["lpips"] > 0
    assert ast.literal_eval(open(os.path.join(scored, "metrics.txt")).read()) == m2
    assert sorted(os.listdir(os.path.join(scored, "estim"))) == ["000.png", "001.png", "002.png", "003.png"]
