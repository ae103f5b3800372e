"""Static checks of the generated gfx950 code of the fused T-NeRF training pass (hipcc -S, no GPU needed): the segment plan of
the backward kernel and of the TRAIN forward, and zero scratch from the code object's metadata (csrc/tnerf_train_kernels.hip,
swnerf_common.h SW_TN_BWD_*).  Resource numbers only."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa_tn_train") / "tnerf_train.s"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-S", "--cuda-device-only",
                    "-o", str(out), os.path.join(ROOT, "sw-nerf_amd", "csrc", "tnerf_train_kernels.hip")], check=True, stderr=subprocess.DEVNULL)
    return out.read_text()


def _kernel(asm, key):
    import isa_audit
    found = [(n, b) for n, b in isa_audit.kernels(asm) if key in n]
    assert len(found) == 1, [n for n, _ in found]
    name, body = found[0]
    stats, bad = isa_audit.audit(body)
    assert not bad
    meta = re.search(rf"\.amdhsa_kernel {name}.*?\.end_amdhsa_kernel", asm, re.S).group(0)
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0
    return stats, len(re.findall(r"global_load_lds_dwordx4", body)), int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1))


def test_backward_kernel_plan(asm):
    stats, dma, vgprs = _kernel(asm, "tnerf_backward_kernel")
    # static segment sites per tile: W9f^T (4 x 2 = 32 steps) and the 4 x 4 loop body of layers.7 .. layers.1 (64 steps), once each
    steps = 32 + 64
    assert stats["mfma"] == 4 * steps and stats["scratch"] == 0, stats
    # + ring priming (8) + the activation fetch sites: the layer_9 hidden (a burst of 8), h7 (16, spread over the W9f^T segment),
    # the loop's h_{l-1} (16, spread over the 4 x 4 segment)
    assert dma == steps + 8 + 8 + 16 + 16
    assert vgprs <= 256                                   # 208 incl. 64 accumulation registers; one workgroup per CU by LDS


def test_train_forward_keeps_the_inference_plan(asm):
    stats, dma, vgprs = _kernel(asm, "tnerf_render_kernel")
    steps = 16 + 16 + 8 + 32 + 64 + 32 + 32               # tests/test_tnerf_isa.py: the same sites, once each
    assert stats["mfma"] == 4 * steps and stats["scratch"] == 0, stats
    assert dma == steps + 8 + 1
    assert vgprs <= 256                                   # two waves per SIMD, as the inference pass
