"""Static checks of the generated gfx950 code of the fused T-NeRF pass (hipcc -S, no GPU needed): no scratch, the MFMA
count of the segment plan, and one LDS-DMA step per weight-stream step (csrc/tnerf_kernels.hip, swnerf_common.h SW_TN_*)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa_tn") / "tnerf.s"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-S", "--cuda-device-only",
                    "-o", str(out), os.path.join(ROOT, "sw-nerf_amd", "csrc", "tnerf_kernels.hip")], check=True, stderr=subprocess.DEVNULL)
    return out.read_text()


def test_tnerf_pass_isa(asm):
    import isa_audit
    found = [(n, b) for n, b in isa_audit.kernels(asm) if "tnerf_render_kernel" in n]
    assert len(found) == 1
    name, body = found[0]
    stats, bad = isa_audit.audit(body)
    assert not bad
    # static segment sites: per-ray prefix T0 (16) T5 (16) DIR (8); per tile L0 (32), the 4x4 loop body (64), the skip's
    # gamma(x) columns (32), layer_9 (32) - every site once
    steps = 16 + 16 + 8 + 32 + 64 + 32 + 32
    assert stats["mfma"] == 4 * steps, stats
    dma = len(re.findall(r"global_load_lds_dwordx4", body))
    assert dma == steps + 8 + 1                     # + ring priming (8) + the L2 warm-up site (render_pass.h pass_startup)
    m = re.search(rf"\.amdhsa_kernel {name}.*?\.end_amdhsa_kernel", asm, re.S)
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(0)).group(1)) == 0
    assert "scratch_" not in body
