"""CPU-only checks of the 2-D fitting host side: Model's state_dict against the golden G16 (tests/golden/make_golden_fit2d.py: the
reference's 2d_pos_encoding/ on CPU), the checkpoint format, the float64 restatement tests/fit2d_ref.py against G16, the argument
refusals of every new C entry point (returned before anything touches the GPU), and the generated gfx950 code of
csrc/fit2d_kernels.hip: no scratch in any kernel, and the fused pass's MFMA count equals its static segment plan.  The second half
is the CPU side of the shape sweep (tests/test_gpu_fit2d_shapes.py): its yardstick, its gate, and the encoder's slot map
csrc/fit2d_cols.h printed by tests/fit2d_cols_host_main.cpp for every band count."""
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import cases_fit2d as C
import fit2d_ref as R
from swnerf import _lib, fit2d, runner

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g16_fit2d.npz")


@pytest.fixture(scope="module")
def g16():
    g = dict(np.load(GOLDEN, allow_pickle=False))
    assert np.array_equal(g["checksum"], C.inputs_checksum()), "cases_fit2d.py no longer generates the inputs G16 was made from"
    return g


def golden_encode(g, L):
    """the reference's encode(grid, L), rebuilt from the stored distinct x / y rows"""
    pos = C.grid().astype(int)
    e = np.zeros((pos.shape[0], 4 * L + 2), np.float32)
    cols = [0] + [4 * i + 2 + 2 * s for i in range(23) for s in (0, 1)]
    for j, c in enumerate(cols):
        if c < 4 * L + 2:
            e[:, c] = g["enc_x"][pos[:, 0], j]
            e[:, c + 1] = g["enc_y"][pos[:, 1], j]
    return e


def test_state_dict_matches_reference(g16):
    torch.manual_seed(0)
    sd = fit2d.Model(input_dimension=82, layer_num=10).state_dict()
    assert list(sd.keys()) == list(g16["init_names"])
    assert [(list(v.shape) + [0, 0])[:2] for v in sd.values()] == g16["init_shapes"].tolist()
    assert np.array_equal(np.array([float(v.double().sum()) for v in sd.values()]), g16["init_sums"])
    assert "model.2.running_mean" in sd and "model.2.num_batches_tracked" in sd and "model.30.weight" in sd


def _args(tmp_path, **over):
    a = dict(L=4, layer_num=2, regularization=0.1, picture_dir="pics/blob.jpg", checkpoint_save=str(tmp_path), checkpoint_load=None,
             output_dir=str(tmp_path), epochs=1, v=False)
    a.update(over)
    return types.SimpleNamespace(**a)


def test_checkpoint_round_trip(tmp_path):
    args = _args(tmp_path)
    torch.manual_seed(3)
    model, opt, sch, start, metrics = runner.create_fit2d(args, device="cpu")
    assert isinstance(model, fit2d.Model) and model.input_dimension == 18 and start == 0 and metrics == {"MSE": [], "PSNR": []}
    assert type(opt).__name__ == "AdamW" and type(sch).__name__ == "ExponentialLR" and opt.defaults["lr"] == 0.001 and sch.gamma == 0.95
    with torch.no_grad():
        model.model[2].running_mean.uniform_(0, 1)
    path = fit2d.save_checkpoint(model, opt, 4, {"MSE": [0.5], "PSNR": [torch.tensor(3.0)]}, args)
    assert path == os.path.join(str(tmp_path), "blob_4_2_0.1.pth")
    ck = torch.load(path, weights_only=False)
    assert set(ck) == {"cur_epoch", "model_state_dict", "optimizer_state_dict", "metrics"} and ck["cur_epoch"] == 5
    model2, _, _, start2, metrics2 = runner.create_fit2d(_args(tmp_path, checkpoint_load=path), device="cpu")
    assert start2 == 5 and metrics2["MSE"] == [0.5]
    for (k1, v1), (k2, v2) in zip(model.state_dict().items(), model2.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2)


def test_cpu_parameters_are_an_error():
    m = fit2d.Model(18, 2).eval()
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(4, 18))
    with pytest.raises(RuntimeError, match="GPU"):
        fit2d.encode(torch.zeros(4, 2), 4)


@pytest.mark.parametrize("L", C.ENCODE_LS)
def test_restatement_encode(g16, L):
    want = golden_encode(g16, L)
    got = R.encode(C.grid(), L)
    assert np.array_equal(got[:, :2].astype(np.float32), want[:, :2])          # the normalised coordinates: bit-equal
    assert np.abs(got - want).max() < 1.2e-7                                   # torch's fp32 sin / cos of the same fp32 argument


@pytest.mark.parametrize("name", sorted(C.EVAL))
def test_restatement_eval_and_fold(g16, name):
    n, L, hid, _ = C.EVAL[name]
    sd, x = C.weights(name), golden_encode(g16, L).astype(np.float64)
    want = g16[f"eval_{name}"]
    ref = R.forward_eval(sd, x)
    assert want.shape == (C.GRID_W * C.GRID_H, 3) and want.std() > 0.5
    assert np.abs(ref - want).max() < 2e-5                                     # the reference's own fp32 (measured: up to 8e-6)
    assert np.abs(R.forward_folded(R.fold(sd), x) - ref).max() < 2e-6          # the fold is exact up to one rounding per weight
    assert any((sd[f"model.{3 * i + 2}.weight"] < 0).any() for i in range(n))  # negative gamma: a fold THROUGH the ReLU would show


def test_restatement_train_step(g16):
    t = C.TRAIN
    idx, target = C.train_batch()
    x = golden_encode(g16, t["L"])[idx]
    loss, _, grads, bufs, pre = R.train_step(C.train_weights(), x, target, t["reg"], t["layer_num"], t["hidden_dim"])
    assert min(float(np.abs(p).min()) for p in pre) > 1e-5                     # no pre-activation near the ReLU's kink
    assert abs(loss - float(g16["train_loss"][0])) < 1e-6
    for k, g in grads.items():
        assert np.abs(g16[f"train_grad_{k}"] - g).max() <= 2e-6 * np.abs(g).max(), k
    for k, b in bufs.items():
        assert np.allclose(g16[f"train_buf_{k}"], b, rtol=0, atol=2e-6), k
    assert int(g16["train_buf_model.2.num_batches_tracked"]) == 8


def test_c_entry_points_validate_before_any_device_call():
    L = _lib.lib()
    err = lambda: L.swnerf_last_error().decode()
    one = 1 << 12                                                               # never dereferenced: rejected first
    assert L.swnerf_encode2d(one, 4, 1.0, 1.0, 24, one, None) == -1 and "L 24" in err()
    assert L.swnerf_encode2d(one, 4, 0.0, 1.0, 4, one, None) == -1 and "max_x" in err()
    assert L.swnerf_encode2d(one, 4, 1.0, 0.0, 4, one, None) == -1
    assert L.swnerf_encode2d(None, 4, 1.0, 1.0, 4, None, None) == -1 and "NULL" in err()
    assert L.swnerf_encode2d(None, 0, 1.0, 1.0, 4, None, None) == 0
    a7 = [one] * 7
    assert L.swnerf_bn_forward_train(one, 1, 8, 1, one, one, 1e-5, 0.1, *a7, None) == -1 and "M >= 2" in err()
    assert L.swnerf_bn_forward_train(one, 4, 0, 1, one, one, 1e-5, 0.1, *a7, None) == -1
    assert L.swnerf_bn_forward_train(None, 4, 8, 1, one, one, 1e-5, 0.1, *a7, None) == -1 and "NULL" in err()
    assert L.swnerf_bn_forward_train(one, 513, 8, 1, one, one, 1e-5, 0.1, one, one, one, one, one, None, None) == -1 and "workspace" in err()
    assert L.swnerf_bn_backward(one, one, 1, 8, 1, *([one] * 7), None) == -1 and "M >= 2" in err()
    assert L.swnerf_bn_backward(None, one, 4, 8, 1, *([one] * 7), None) == -1 and "NULL" in err()
    assert L.swnerf_bn_apply(None, 4, 8, 0, one, one, one, one, 1e-5, one, None) == -1 and "NULL" in err()
    assert L.swnerf_bn_apply(one, 4, 0, 0, one, one, one, one, 1e-5, one, None) == -1
    assert [L.swnerf_bn_workspace_bytes(m, 256) for m in (2, 512, 513, 1 << 20)] == [0, 0, 3 * 2 * 256 * 8, 1024 * 2 * 256 * 8]
    assert L.swnerf_fit2d_loss(None, one, 4, 0.1, one, one, None) == -1 and "NULL" in err()
    assert L.swnerf_fit2d_loss(one, one, 0, 0.1, one, one, None) == -1
    assert [L.swnerf_fit2d_packed_floats(n) for n in (0, 1, 10, 65)] == [0, (96 + 16) * 256 + 33 * 32, (96 + 9 * 256 + 16) * 256 + 105 * 32, 0]
    assert L.swnerf_pack_fit2d(None, 10, 20, 1e-5, one, None) == -1 and "NULL" in err()
    arr = (_lib.c_void_p * 62)(*([one] * 62))
    assert L.swnerf_pack_fit2d(arr, 0, 20, 1e-5, one, None) == -1 and "n_layers" in err()
    assert L.swnerf_pack_fit2d(arr, 10, 24, 1e-5, one, None) == -1 and "L 24" in err()
    assert L.swnerf_pack_fit2d(arr, 65, 20, 1e-5, one, None) == -2
    arr[5] = None
    assert L.swnerf_pack_fit2d(arr, 10, 20, 1e-5, one, None) == -1 and "params[5]" in err()
    assert L.swnerf_fit2d_forward(one, one, 4, 82, 24, 10, one, None) == -1 and "L 24" in err()
    assert L.swnerf_fit2d_forward(one, one, 4, 82, 20, 0, one, None) == -1 and "n_layers" in err()
    assert L.swnerf_fit2d_forward(one, one, 4, 81, 20, 10, one, None) == -1 and "82" in err()
    assert L.swnerf_fit2d_forward(None, one, 4, 82, 20, 10, one, None) == -1 and "NULL" in err()
    assert L.swnerf_fit2d_forward(one, one, 0, 82, 20, 10, one, None) == 0
    assert L.swnerf_fit2d_picture(one, 37, 53, 20, 10, None, None, None) == -1 and "both NULL" in err()
    assert L.swnerf_fit2d_picture(one, 37, 1, 20, 10, one, None, None) == -1 and "1-pixel" in err()
    assert L.swnerf_fit2d_picture(one, 37, 53, 24, 10, one, None, None) == -1
    assert L.swnerf_fit2d_picture(one, 37, 53, 20, 0, one, None, None) == -1
    assert L.swnerf_fit2d_picture(None, 37, 53, 20, 10, one, None, None) == -1 and "NULL" in err()


def test_python_refusals():
    bn = torch.nn.BatchNorm1d(8)
    with pytest.raises(RuntimeError, match="GPU"):
        fit2d.relu_batch_norm(torch.zeros(4, 8), bn)
    with pytest.raises(ValueError, match="L 24"):
        fit2d.encode(torch.zeros(4, 2), 24)
    assert fit2d.Model(82, 10).fused_L() == 20 and fit2d.Model(18, 3, hidden_dim=64).fused_L() is None
    assert fit2d.Model(98, 2).fused_L() is None and fit2d.Model(94, 2).fused_L() == 23 and fit2d.Model(2, 1).fused_L() == 0


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa_fit2d") / "fit2d.s"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-S", "--cuda-device-only",
                    "-o", str(out), os.path.join(ROOT, "sw-nerf_amd", "csrc", "fit2d_kernels.hip")], check=True, stderr=subprocess.DEVNULL)
    return out.read_text()


def test_fit2d_kernels_isa(asm):
    descs = re.findall(r"\.amdhsa_kernel (\w+)(.*?)\.end_amdhsa_kernel", asm, re.S)
    names = [n for n, _ in descs]
    for want in ("encode2d_kernel", "bn_one_kernel", "bn_partial_kernel", "bn_final_kernel", "bn_apply_saved_kernel", "bn_apply_kernel",
                 "fit2d_loss_kernel", "pack_fit2d_w_kernel", "pack_fit2d_b_kernel", "fit2d_kernel"):
        assert any(want in n for n in names), want
    for n, d in descs:
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", d).group(1)) == 0, n
    fused = [n for n in names if "fit2d_kernel" in n and "pack" not in n]
    assert len(fused) == 2                                                      # forward and picture: one template
    for n in fused:
        body = asm[asm.index(f"\n{n}:"):]
        body = body[:body.index("s_endpgm")]
        # static plan: layer 0 (8 x 3 tiles = 96 steps) and ONE 8 x 8 loop body (256 steps), 4 MFMAs per step
        assert len(re.findall(r"^\s*v_mfma", body, re.M)) == 4 * (96 + 256), n


# ---- the shape sweep (cases_fit2d.SHAPES; the GPU half is tests/test_gpu_fit2d_shapes.py) -------------------------------------
# Yardstick: ref64 = fit2d_ref.forward_eval in float64; e_ref = the distance of the same net in fp32 torch on the CPU from it.
# A kernel passes a case when max |got - ref64| <= max(GATE * e_ref, GATE fp32 ulps of max |ref64|): per case, never pooled.
# The checks here show that the yardstick is usable at every case (finite, O(1..1e3), not a dead net, e_ref > 0, the fold restated
# in float64 agrees with it) and that the gate has teeth: the fp32 CPU model with one defect of the kind a mispacked stream would
# have lies outside it.  The fourth defect (2e-4 on one folded bias of layer 1) is asserted below 33 layers only: from there on
# e_ref is 1e-3 and more, so 2e-4 on one of 256 channels falls under 4 e_ref by construction.
GATE = 4.0                                  # the standing margin for "the same fp32 sums in another order" (test_gpu_lpips.py, test_gpu_optim.py)
BIAS_DEFECT, BIAS_DEFECT_BELOW = 2e-4, 33
FUSED_CASES = sorted(C.SHAPES) + sorted(C.BN_EPS)


def fp32_model(sd, eps=1e-5):
    """the same net in fp32 torch on the CPU, eval mode"""
    n = R.layer_num(sd)
    net = R.module(sd["model.0.weight"].shape[1], n, sd["model.0.weight"].shape[0], sd[f"model.{3 * n}.weight"].shape[0], sd, dtype=torch.float32)
    for mod in net.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.eps = eps
    return net.eval()


def fp32_eval(sd, x32, eps=1e-5):
    with torch.no_grad():
        return fp32_model(sd, eps)(torch.from_numpy(np.ascontiguousarray(x32, np.float32))).numpy()


def yardstick(sd, x32, eps=1e-5):
    """(ref64, e_ref, gate) of one case on the fp32 rows x32"""
    ref64 = R.forward_eval(sd, np.asarray(x32, np.float64), eps)
    e_ref = float(np.abs(fp32_eval(sd, x32, eps) - ref64).max())
    return ref64, e_ref, max(GATE * e_ref, GATE * float(np.spacing(np.float32(np.abs(ref64).max()))))


def fused_case(name):
    """(state dict, eps, L, layer_num, grid indices of its rows)"""
    if name in C.BN_EPS:
        sd, eps = C.bn_weights(name)
        return sd, eps, C.BN_L, C.BN_LAYERS, C.shape_rows(C.BN_LAYERS, C.BN_SEED)
    _, L, n, seed = C.SHAPES[name]
    return C.shape_weights(name), 1e-5, L, n, C.shape_rows(n, seed)


_host_cache = {}


def _host_case(name):
    """the case on the restatement's own encoding rounded to fp32 (the GPU tests take the rows from the encode kernel)"""
    if name not in _host_cache:
        sd, eps, L, n, idx = fused_case(name)
        x32 = R.encode(C.grid(), L)[idx].astype(np.float32)
        _host_cache[name] = (sd, eps, L, n, x32) + yardstick(sd, x32, eps)
    return _host_cache[name]


@pytest.mark.parametrize("name", FUSED_CASES)
def test_shape_yardstick_is_sound(name):
    sd, eps, L, n, x32, ref64, e_ref, gate = _host_case(name)
    assert x32.shape == (1961 if n >= C.DEEP_FROM else 161, 4 * L + 2)
    assert np.isfinite(ref64).all() and np.abs(ref64).max() < 1e4
    assert ref64.std(axis=0).min() > 0.05                                       # a dead net would pin nothing
    assert e_ref > 0
    fold = R.forward_folded(R.fold(sd, eps), x32.astype(np.float64))
    e_fold = float(np.abs(fold - ref64).max())
    print(f"{name}: max |ref64| {np.abs(ref64).max():.3e}, std {ref64.std(axis=0).min():.3f}, e_ref {e_ref:.3e}, gate {gate:.3e}, fp32-rounded fold {e_fold:.3e}")
    # the fold restated in float64 WITHOUT the rounding of the folded weights: the restatement itself, to 1e-9 relative
    h = x32.astype(np.float64)
    for l in range(n + 1):
        W, b = sd[f"model.{3 * l}.weight"].astype(np.float64), sd[f"model.{3 * l}.bias"].astype(np.float64)
        if l > 0:
            p = f"model.{3 * (l - 1) + 2}."
            s = sd[p + "weight"].astype(np.float64) / np.sqrt(sd[p + "running_var"].astype(np.float64) + eps)
            t = sd[p + "bias"].astype(np.float64) - sd[p + "running_mean"].astype(np.float64) * s
            W, b = W * s, b + W @ t
        h = h @ W.T + b
        if l < n:
            h = np.maximum(h, 0)
    assert np.abs(h - ref64).max() <= 1e-9 * np.abs(ref64).max()
    # ... and with them rounded to fp32 once (what the pack kernel stores) it stays inside the gate
    assert e_fold <= gate


def _defect_error(sd, eps, x32, ref64):
    return float(np.abs(fp32_eval(sd, x32, eps) - ref64).max())


@pytest.mark.parametrize("name", FUSED_CASES)
def test_shape_gate_has_teeth(name):
    sd, eps, L, n, x32, ref64, e_ref, gate = _host_case(name)
    errs = {}
    x = x32.copy()
    x[:, 4 * L + 1] = 0.0                 # L >= 1: the last band's cosine of the y half; L = 0: the raw y coordinate
    errs["column"] = _defect_error(sd, eps, x, ref64)
    bad = {k: v.copy() for k, v in sd.items()}
    bad[f"model.{3 * n}.weight"][:, [5, 133]] = bad[f"model.{3 * n}.weight"][:, [133, 5]]      # the head reads two channels of layer n - 1 swapped
    errs["swap"] = _defect_error(bad, eps, x32, ref64)
    if n < BIAS_DEFECT_BELOW:
        bad = {k: v.copy() for k, v in sd.items()}
        if n == 1:
            c = 0                                                                # layer 1 is the head: any of its three biases
        else:
            # the most influential bias of layer 1: among the channels that at least half of the rows switch on, the one with the
            # largest folded weight |s_c| max_o |W2[o, c]| towards the next Linear (2e-4 on a dead or lightly weighted channel moves nothing)
            on = (R.forward_eval(sd, x32.astype(np.float64), eps, want_pre=True)[1][1] > 0).mean(axis=0) >= 0.5
            W2 = R.fold(sd, eps)[2][0]
            c = int(np.where(on, np.abs(W2).max(axis=0), 0.0).argmax())
        bad["model.3.bias"][c] += np.float32(BIAS_DEFECT)
        errs["bias"] = _defect_error(bad, eps, x32, ref64)
    print(f"{name}: gate {gate:.3e}, defects " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v > gate, k


@pytest.fixture(scope="module")
def col_map(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fit2d_cols") / "fit2d_cols_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-I", os.path.join(ROOT, "sw-nerf_amd", "csrc"),
                    os.path.join(ROOT, "tests", "fit2d_cols_host_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout
    rows = [[int(v) for v in line.split()] for line in out.splitlines()]
    assert len(rows) == 48 and all(len(r) == 50 for r in rows)
    return {(r[0], r[1]): r[2:] for r in rows}


@pytest.mark.parametrize("L", range(24))
def test_column_scatter_is_a_permutation(col_map, L):
    cols = [c for h in (0, 1) for c in col_map[(L, h)] if c >= 0]
    assert len(cols) == len(set(cols)) == 4 * L + 2                             # no column twice
    assert sorted(cols) == list(range(4 * L + 2))                               # ... and every one once
    for h in (0, 1):
        m = col_map[(L, h)]
        assert m[46] == h and m[47] == -1                                       # slot 46: the raw coordinate; 47: never used
        assert all(m[a] == -1 for a in range(2 * L, 46))                        # bands i >= L: no column (an exact zero operand)
        assert [m[a] for a in range(2 * L)] == [2 + 4 * (a >> 1) + 2 * (a & 1) + h for a in range(2 * L)]   # encoding.py:29-38
