"""csrc/wgrad_x3_kernels.hip compiled to gfx950 assembly: every kernel of the unit holds no scratch and runs on
v_mfma_f32_32x32x16_bf16 (the bf16x3 weight-gradient GEMM; its fp32 sibling is audited in tests/test_isa_audit.py)."""
import os
import re
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_wgrad_x3_kernels_isa(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "wgrad_x3.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(ROOT, "sw-nerf_amd", "csrc", "wgrad_x3_kernels.hip")], check=True, stderr=subprocess.DEVNULL)
    asm = out.read_text()
    seen = []
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S):
        name = m.group(1)
        priv = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
        assert priv == 0, f"{name} spills {priv} bytes/lane"
        body = asm[asm.index("\n" + name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert "scratch_" not in body, name
        mfma = re.findall(r"^\s*(v_mfma\S*)", body, re.M)
        assert mfma and set(mfma) == {"v_mfma_f32_32x32x16_bf16"}, (name, sorted(set(mfma)))
        # two k-steps of 16 rows per 32-row slab x 4 tiles x 3 terms, the slab loop once
        assert len(mfma) == 2 * 4 * 3, (name, len(mfma))
        seen.append(name)
    assert len(seen) == 1 and "gemm_tn_x3_group_kernel" in seen[0], seen
