"""Static checks of the generated gfx950 code of the MFMA kernels (hipcc -S, no GPU needed).

The weight stream is hand-pinned inline asm (csrc/mlp_core.h); these are the properties the
design relies on and that a compiler change could silently break:
  * no scratch (spills) in the render kernels, exactly the expected MFMA count per kernel body,
  * every LDS-DMA step is an asm statement and there are as many as weight-stream steps,
  * no instruction touches a VGPR that an inline-asm load still has in flight
    (tools/isa_audit.py; vacuous for LDS-DMA, kept as a guard should a register ring come back)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    text = ""
    for src in ("render_kernels.hip", "train_kernels.hip"):      # inference (ring depth 8) and training (16) units
        out = d / (src + ".s")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-S", "--cuda-device-only",
                        "-o", str(out), os.path.join(ROOT, "sw-nerf_amd", "csrc", src)], check=True,
                       stderr=subprocess.DEVNULL)
        text += out.read_text()
    return text


def test_mfma_kernels_isa(asm):
    import isa_audit
    seen = {}
    for name, body in isa_audit.kernels(asm):
        if "sample_coarse_kernel" in name:          # the one non-MFMA kernel of these translation units
            assert "v_mfma" not in body and "scratch_" not in body
            continue
        stats, bad = isa_audit.audit(body)
        assert not bad, f"{name}: {len(bad)} uses of in-flight asm-load registers, e.g. {bad[0]}"
        dma = len(re.findall(r"global_load_lds_dwordx4", body))
        seen[name] = (stats, dma)
        # code is unrolled per segment type: L0(64) trunk(256) skip-emb(64) and the view layer - feature_linear is folded into
        # it at pack time (swnerf_common.h SW_CANON_STEPS), so NO 256-step feature body may be left.  The fused passes run the view
        # layer as DIR (16 steps, once per RAY: outside the tile loop) + VIEWSH (128 per tile): 8192 MFMAs per tile instead of
        # round 3's 9280; kernels with per-row directions run one 144-step [gamma(d) | h7] segment.  Same static count either way.
        # (+ the 96-step deformation layer 0 in the D-NeRF instantiations); +8 priming DMAs
        steps = 64 + 256 + 64 + 144 + (96 if "kernelILb1" in name else 0)
        if "query_points" in name:
            steps = 64 + 256 + 64 + 144
        if "render_pass_kernelILb0ELb0ELi0ELb0EE" in name or "render_pass_kernelILb0ELb1ELi0ELb0EE" in name or "mlp_forward_noview" in name:
            steps = 64 + 256 + 64                  # no view branch (inference, TRAIN): L0 (64), trunk body (256), skip-emb (64)
        if "mlp_backward_dx" in name:              # RGB^T (16) W_vf^T (128: view layer and feature_linear as one) + the L7..L1 loop body (256)
            steps = 16 + 128 + 256                # <true>: + the gamma(x) columns of pts_linears.5 and .0 (64 each)
            if "kernelILb1" in name:
                steps += 128
        if "deform_forward_train" in name:         # _time.0 (96) + trunk body (256) + skip-emb (64)
            steps = 96 + 256 + 64
        if "deform_backward_dx" in name:           # the _time.7 .. _time.1 loop body
            steps = 256
        if "render_pass_backward" in name:         # the fused backward: the same chain as mlp_backward_dx<false>, per tile
            steps = 16 + 128 + 256
            if "kernelILi1" in name:               # D-NeRF: + the gamma(x+dx) columns (2 x 64) + the deformation loop body
                steps += 128 + 256
            if "kernelILi2" in name:               # no view directions: the L7..L1 loop body alone (output_linear^T runs on the VALU)
                steps = 256
        # the backward chains also fetch the ReLU bit masks by LDS-DMA: one fetch before the ring is primed, one per
        # static use site after it (mlp_backward_dx: views hidden, h7, loop body; deformation: h7, loop body)
        masks = 3 if ("mlp_backward_dx" in name or "render_pass_backward" in name) else (2 if "deform_backward_dx" in name else 0)
        if "render_pass_backward_kernelILi1" in name:
            masks = 5                                # canonical (3 sites) + deformation (h7, loop body)
        if "render_pass_backward_kernelILi2" in name:
            masks = 2                                # h7, loop body
        assert stats["mfma"] == 4 * steps, (name, stats)
        # ring priming: 8 steps in the render unit, 16 in the training unit (train_kernels.hip)
        training = any(k in name for k in ("mlp_backward_dx", "deform_", "mlp_forward_kernelILb0ELb1E", "render_pass_backward",
                                           "render_pass_kernelILb0ELb1E", "render_pass_kernelILb1ELb1E"))
        # the fused pass pulls the weight stream into L2 at kernel start with one more static DMA site (render_pass.h pass_startup)
        warm = 1 if "render_pass_kernel" in name else 0
        # kernels whose view directions vary per row leave the main stream behind the trunk and prime the ring afresh on the views
        # loop (mlp_core.h ws_restart): one more set of priming DMAs
        restart = (16 if training else 8) if ("query_points" in name or "mlp_forward_kernel" in name) else 0
        assert dma == steps + (16 if training else 8) + masks + warm + restart, (name, dma)
    assert len(seen) == 18
    for name in seen:
        m = re.search(rf"\.amdhsa_kernel {name}.*?\.end_amdhsa_kernel", asm, re.S)
        assert m, name
        priv = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(0)).group(1))
        # No spills at all (since the bias tiles are read one at a time and the head sums are pinned, mlp_core.h).
        # A scratch access shares vmcnt with the weight DMA ring, so a reload inside a segment would drain the ring:
        # should spills ever come back, none may sit within 40 instructions of an MFMA.
        assert priv == 0, f"{name} spills {priv} bytes/lane to scratch"
        if "render_pass" in name or "query_points" in name or "mlp_backward_dx" in name:
            body = asm[asm.index("\n" + name + ":"):]
            body = body[:body.index("s_endpgm")]
            lines = [l for l in body.split("\n") if l.strip() and not l.strip().startswith(";")]
            mf = [k for k, l in enumerate(lines) if "v_mfma" in l]
            import bisect
            for k, l in enumerate(lines):
                if "scratch_" in l and mf[0] < k < mf[-1]:
                    p_ = bisect.bisect(mf, k)
                    assert k - mf[p_ - 1] >= 40 and mf[p_] - k >= 40, f"{name}: `{l.strip()}` sits inside the MFMA stream"


def test_weight_gradient_gemm_isa(tmp_path):
    """wgrad_kernels.hip: every weight-gradient GEMM kernel holds no scratch (round-1 VERDICT: the narrow GEMM spilled 56-176 B/lane
    through its staging registers; the first narrow5_kernel spilled 428 B/lane).  The kernels, 14 in all:
      4  gemm_tn_kernel<VA, VB>                   the operand-alignment variants of the narrow GEMM (slabs staged by LDS-DMA too)
      2  gemm_tn_dma_kernel<HB2>                  the 256x256 LDS-DMA GEMM, without and with the B2 rider
      1  gemm_tn_dma_group_kernel                 the grouped launch: both of those bodies
      5  gemm_tn_tiled_kernel<TO, TI, WO, WI>     the wave grids of the skinny double-buffered kernel
      1  narrow5_kernel, 1 narrow_plan_kernel     the fused narrow products (five roles / four tile shapes, the slab loop once per role)
    and the static MFMA counts of the two kernels that hold several bodies: a body that comes back (or goes missing) shows here."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "wgrad.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(ROOT, "sw-nerf_amd", "csrc", "wgrad_kernels.hip")], check=True, stderr=subprocess.DEVNULL)
    asm = out.read_text()
    seen, mfma = 0, {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S):
        name = m.group(1)
        if "gemm_tn" not in name and "narrow5" not in name and "narrow_plan" not in name:
            continue
        priv = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
        assert priv == 0, f"{name} spills {priv} bytes/lane"
        body = asm[asm.index("\n" + name + ":"):]
        body = body[:body.index(".Lfunc_end")]                # the whole kernel (these kernels have early exits: several s_endpgm)
        assert "scratch_" not in body, name
        mfma[name] = len(re.findall(r"^\s*v_mfma", body, re.M))
        seen += 1
    assert seen == 14
    count = lambda key: [n for k, n in mfma.items() if key in k]
    # four tile shapes x 8 k-pairs of a 16-row slab x 4 tiles
    assert count("narrow_plan_kernel") == [4 * 8 * 4]
    # two bodies, each the slab loop once per bias role: without the rider 16 k-pairs x 4 tiles, with it 4 unrolled k-pairs x 5 tiles
    assert count("gemm_tn_dma_group_kernel") == [2 * 16 * 4 + 2 * 4 * 5]


def test_x3_kernels_isa(tmp_path):
    """The bf16x3 / bf16 pass (csrc/mlp_core_x3.h): the properties its shared weight ring relies on.
      * no scratch at all (a scratch reload drains the DMA ring: scratch shares vmcnt),
      * static MFMA count = groups of the unrolled bodies x terms (the software-pipelined form: a two-layer loop body),
      * one bare s_barrier per chunk of 8 groups (+ the one that publishes chunk 0), each behind a counted vmcnt wait -
        never a `vmcnt(0)` between the first and the last MFMA (it would wait for the whole ring),
      * the refill of a chunk is 4 LDS-DMA instructions, issued one per group."""
    import isa_audit
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "x3.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-S", "--cuda-device-only",
                    "-o", str(out), os.path.join(ROOT, "sw-nerf_amd", "csrc", "x3_kernels.hip")], check=True, stderr=subprocess.DEVNULL)
    text = out.read_text()
    seen = 0
    for name, body in isa_audit.kernels(text):
        if "render_pass_kernel" not in name:
            continue
        seen += 1
        terms = 3 if "Li3E" in name else 1
        # static: L0 (32) + the two-layer loop body (256) + layer 5's gamma(x) part (32) + layer 7 behind the loop (128) + the view
        # layer (64 + 8) - feature_linear is folded into the view layer's weights (round 4): no 128-group body of its own any more
        groups = 32 + 256 + 32 + 128 + 64 + 8
        if "kernelILb1" in name:                    # D-NeRF: + the deformation layer 0 (48)
            groups += 48
        lines = body.split("\n")
        mf = [i for i, l in enumerate(lines) if "v_mfma_f32_32x32x16_bf16" in l]
        assert len(mf) == groups * terms, (name, len(mf))
        assert "v_mfma_f32_32x32x2_f32" not in body
        chunks = groups // 8
        assert len(re.findall(r"\bs_barrier\b", body)) == chunks + 1 + 1, name         # + chunk 0's + bias_to_lds's __syncthreads
        dma = len(re.findall(r"global_load_lds_dwordx4", body))
        assert dma == 4 * chunks + 4 * 4 + 3, (name, dma)                              # + priming: 4 chunks and 3 parts of the fifth
        hot = "\n".join(lines[mf[0]:mf[-1]])
        assert "vmcnt(0)" not in hot and "scratch_" not in body, name
        m = re.search(rf"\.amdhsa_kernel {name}.*?\.end_amdhsa_kernel", text, re.S)
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(0)).group(1)) == 0
    assert seen == 4


def test_embed_kernel_isa(tmp_path):
    """misc_kernels.hip embed_kernel: no scratch in either instantiation (the kernel is VALU-issue bound).  <true> (L > 10) holds
    the double-precision argument reduction of the bands k >= 10 (swnerf_common.h sw_sincos_pair_wide) inline; <false> (L <= 10:
    every embedder the reference builds, and what the fused path must agree with bit for bit) holds no double instruction."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "misc.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(ROOT, "sw-nerf_amd", "csrc", "misc_kernels.hip")], check=True, stderr=subprocess.DEVNULL)
    asm = out.read_text()
    found = {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S*embed_kernel\S*)(.*?)\.end_amdhsa_kernel", asm, re.S)}
    assert sorted("ILb1E" in n for n in found) == [False, True], list(found)
    for name, desc in found.items():
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)) == 0, name
        body = asm[asm.index("\n" + name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert "scratch_" not in body and "s_swappc" not in body, name
        assert ("v_rndne_f64" in body) == ("ILb1E" in name) and ("_f64" in body) == ("ILb1E" in name), name
