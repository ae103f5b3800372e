"""GPU tests of 2-D image fitting (swnerf.fit2d, csrc/fit2d_kernels.hip) against the golden G16 (the reference's 2d_pos_encoding/
on CPU, tests/golden/make_golden_fit2d.py) and the float64 restatement tests/fit2d_ref.py.  DESIGN.md 6h has the gates.

  encode      2e-7 abs: the 1.2e-7 bound of sw_sincos_pair_wide plus torch's own fp32 sin / cos rounding (3e-8 in band 19)
  FWD_GATE    fused / layer-by-layer eval against G16: 3 x the maximum measured on the MI355X over the four cases
  BN_GATE     the BatchNorm kernels against float64 torch, relative to each tensor's max: 3 x the measured maximum
  gradients   2e-5 of each tensor's max, the project's gradient gate; loss and running buffers take the same relative gate
  AdamW       5 steps: the loss values within 1e-4 relative; the last layer within 5e-5 - an AdamW step is lr (1e-3) times a ratio
              m / (sqrt(v) + eps) in [-1, 1], and a gradient within 2e-5 of the tensor's max moves that ratio by at most 1e-2
              where |g| > 2e-3 max, i.e. 1e-5 per step
Every test prints the figure it measured before it asserts."""
import types

import numpy as np
import pytest
import torch

import cases_fit2d as C
import fit2d_ref as R
from test_fit2d_host import golden_encode, g16  # noqa: F401
from swnerf import fit2d

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_GATE = 3.0e-5          # measured 1.001e-5 (d10_L20, outputs in [-4.5, 2.8]; the reference's own fp32 is 8.0e-6 from float64 there)
BN_GATE = 4.0e-7           # measured 1.32e-7 (y at (33, 257), relu)
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make_model(sd, n, L, hid):
    m = fit2d.Model(4 * L + 2, n, hidden_dim=hid)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to(DEV)


@pytest.fixture(scope="module")
def models():
    return {name: make_model(C.weights(name), n, L, hid).eval() for name, (n, L, hid, _) in C.EVAL.items()}


@pytest.mark.parametrize("L", C.ENCODE_LS)
def test_encode_matches_reference(g16, L):
    want = golden_encode(g16, L)
    got = fit2d.encode(T(C.grid()), L).cpu().numpy()
    assert got.shape == want.shape
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"encode L={L}: max abs err {err:.3e}")
    assert np.array_equal(got[:, :2], want[:, :2])                     # the normalised coordinates: bit-equal
    assert err <= 2e-7


BN_SHAPES = [(2, 1), (48, 64), (512, 256), (513, 96), (33, 257)]


def _bn_case(M, Cc, relu, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, Cc, generator=g) * 1.2 + 0.3
    dy = torch.randn(M, Cc, generator=g)
    bn = torch.nn.BatchNorm1d(Cc)
    with torch.no_grad():
        bn.weight.copy_((torch.rand(Cc, generator=g) + 0.5) * torch.where(torch.rand(Cc, generator=g) < 0.1, -1.0, 1.0))
        bn.bias.copy_(torch.rand(Cc, generator=g) * 0.6 - 0.3)
        bn.running_mean.copy_(torch.rand(Cc, generator=g) * 0.6)
        bn.running_var.copy_(torch.rand(Cc, generator=g) * 1.7 + 0.3)
    return a, dy, bn


def _bn_run(a, dy, bn, relu):
    import copy
    bn = copy.deepcopy(bn).to(DEV).train()
    a_ = a.to(DEV).requires_grad_(True)
    y = fit2d.relu_batch_norm(a_, bn, relu=relu)
    y.backward(dy.to(DEV))
    return dict(y=y.detach(), dx=a_.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, rmean=bn.running_mean.clone(), rvar=bn.running_var.clone(),
                nbt=bn.num_batches_tracked.clone())


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("M,Cc", BN_SHAPES)
def test_bn_kernels_against_float64(M, Cc, relu):
    import copy
    a, dy, bn = _bn_case(M, Cc, relu, 100 * M + Cc)
    got = _bn_run(a, dy, bn, relu)
    ref = copy.deepcopy(bn).double().train()
    a64 = a.double().requires_grad_(True)
    y64 = ref(torch.relu(a64) if relu else a64)
    y64.backward(dy.double())
    want = dict(y=y64.detach(), dx=a64.grad, dgamma=ref.weight.grad, dbeta=ref.bias.grad, rmean=ref.running_mean, rvar=ref.running_var)
    worst = 0.0
    x64 = (torch.relu(a64) if relu else a64).detach()
    invstd = 1.0 / torch.sqrt(x64.var(0, unbiased=False) + bn.eps)
    for k, w in want.items():
        scale = max(float(w.abs().max()), 1e-30)
        if k == "dx":
            # dx = gamma invstd / M (M dy - dbeta - xhat dgamma) is a difference of terms of size |gamma| invstd |dy|; at M = 2 they
            # cancel down to the eps residue (1e-6 of them), so the error is measured against the terms, not against the residue
            scale = float((ref.weight.detach().abs() * invstd).max() * dy.abs().max())
        e = float((got[k].cpu().double() - w).abs().max()) / scale
        print(f"bn ({M},{Cc}) relu={relu} {k}: rel err {e:.3e} (max {scale:.3e})")
        worst = max(worst, e)
    assert int(got["nbt"]) == 1
    if relu:
        assert bool((got["dx"].cpu()[a <= 0] == 0).all())
    assert worst <= BN_GATE


@pytest.mark.parametrize("M,Cc", [(512, 256), (513, 96)])
def test_bn_is_deterministic(M, Cc):
    a, dy, bn = _bn_case(M, Cc, True, 7)
    r1, r2 = _bn_run(a, dy, bn, True), _bn_run(a, dy, bn, True)
    for k in r1:
        assert torch.equal(r1[k], r2[k]), k


def test_bn_single_row_raises():
    bn = torch.nn.BatchNorm1d(8).to(DEV).train()
    with pytest.raises(ValueError, match="more than 1 value"):
        fit2d.relu_batch_norm(torch.zeros(1, 8, device=DEV), bn)


@pytest.mark.parametrize("reg", [0.0, 0.1])
def test_loss_kernel_against_float64(reg):
    g = torch.Generator().manual_seed(5)
    M = 512
    out = (torch.rand(M, 3, generator=g) * 2 - 0.5)
    tgt = torch.rand(M, 3, generator=g)
    assert float(out.min()) < -0.4 and float(out.max()) > 1.4 and bool(((out != 0) & (out != 1)).all())
    o = out.to(DEV).requires_grad_(True)
    loss, sums = fit2d.fit_loss(o, tgt.to(DEV), reg)
    loss.backward()
    o64 = out.double().requires_grad_(True)
    l64 = R.loss(o64, tgt.double(), reg)
    l64.backward()
    g64 = float(R.gray_mse(out.double(), tgt.double()))
    e_l, e_g = abs(float(sums[0]) - float(l64.detach())) / float(l64.detach()), abs(float(sums[1]) - g64) / g64
    e_d = float((o.grad.cpu().double() - o64.grad).abs().max() / o64.grad.abs().max())
    print(f"loss reg={reg}: rel err loss {e_l:.3e}, grey {e_g:.3e}, grad {e_d:.3e}")
    # fp32 inputs, fp64 sums: the differences are rounded once in fp32 (6e-8 relative each, averaging out over 1536 terms)
    assert e_l < 1e-6 and e_g < 1e-6 and e_d < 1e-6
    assert abs(float(loss.detach()) - float(sums[0])) <= 1e-6 * float(sums[0])


@pytest.mark.parametrize("name", ["d10_L20", "d1_L20", "d3_L4"])
def test_fused_forward_matches_reference(g16, models, name):
    n, L, hid, _ = C.EVAL[name]
    m = models[name]
    assert m.fused_L() == L
    x = T(golden_encode(g16, L))
    want = g16[f"eval_{name}"]
    with torch.no_grad():
        got = m(x).cpu().numpy()
        err = float(np.abs(got - want).max())
        print(f"fused forward {name}: max abs err vs G16 {err:.3e}; vs float64 {np.abs(got - R.forward_eval(C.weights(name), x.cpu().numpy().astype(np.float64))).max():.3e}")
        assert err <= FWD_GATE
        for M in (1, 31, 33, 1000):                                   # ragged row counts: the same rows give the same bits
            assert np.array_equal(m(x[:M].contiguous()).cpu().numpy(), got[:M]), M


@pytest.mark.parametrize("name", sorted(C.EVAL))
def test_layerwise_eval_matches_reference_and_fused(g16, models, name):
    n, L, hid, _ = C.EVAL[name]
    m = models[name]
    x = T(golden_encode(g16, L))
    with torch.no_grad():
        lay = m.forward_layers(x).cpu().numpy()
        full = m(x).cpu().numpy()
    e1, e2 = float(np.abs(lay - g16[f"eval_{name}"]).max()), float(np.abs(lay - full).max())
    print(f"layer-by-layer eval {name}: vs G16 {e1:.3e}, vs model(x) {e2:.3e}")
    assert (m.fused_L() is None) == (name == "generic")
    assert e1 <= FWD_GATE and e2 <= FWD_GATE


@pytest.mark.parametrize("name", ["d10_L20", "d1_L20", "d3_L4"])
def test_picture_equals_forward_bit_for_bit(models, name):
    n, L, hid, _ = C.EVAL[name]
    m = models[name]
    args = types.SimpleNamespace(L=L)
    pic = fit2d.get_picture(C.GRID_W, C.GRID_H, m, args)
    with torch.no_grad():
        fwd = m(fit2d.encode(T(C.grid()), L)).cpu().numpy().reshape(C.GRID_H, C.GRID_W, 3)
    assert pic.shape == (C.GRID_H, C.GRID_W, 3) and pic.dtype == np.float32
    assert np.array_equal(pic, np.clip(fwd, 0, 1))
    assert 0.05 < float(((pic > 0) & (pic < 1)).mean())                # not all clipped away
    u8 = fit2d.get_picture_u8(C.GRID_W, C.GRID_H, m, args)
    assert u8.dtype == np.uint8 and np.array_equal(u8, (255 * np.clip(pic, 0, 1)).astype(np.uint8))
    f, u = fit2d._picture(C.GRID_W, C.GRID_H, m, L, want_f32=True, want_u8=True)
    assert np.array_equal(f.cpu().numpy(), pic) and np.array_equal(u.cpu().numpy(), u8)


def _train_model():
    t = C.TRAIN
    return make_model(C.train_weights(), t["layer_num"], t["L"], t["hidden_dim"]).train()


def test_training_step_matches_reference(g16):
    t = C.TRAIN
    idx, target = C.train_batch()
    x = golden_encode(g16, t["L"])[idx]
    _, _, _, _, pre = R.train_step(C.train_weights(), x, target, t["reg"], t["layer_num"], t["hidden_dim"])
    margin = min(float(np.abs(p).min()) for p in pre)
    print(f"ReLU margin {margin:.3e}")
    assert margin > 1e-5                                                # no pre-activation near the kink: the masks are well defined
    m = _train_model()
    loss, sums = fit2d.fit_loss(m(T(x)), T(target), t["reg"])
    loss.backward()
    e = abs(float(sums[0]) - float(g16["train_loss"][0])) / float(g16["train_loss"][0])
    print(f"train step: loss rel err {e:.3e}")
    assert e <= 2e-5
    for k, p in m.named_parameters():
        want = g16[f"train_grad_{k}"]
        e = float(np.abs(p.grad.cpu().numpy() - want).max() / np.abs(want).max())
        print(f"  grad {k}: err / max {e:.3e}")
        assert e <= 2e-5, k
    for k, b in m.named_buffers():
        want = g16[f"train_buf_{k}"]
        if k.endswith("num_batches_tracked"):
            assert int(b) == int(want)
            continue
        e = float(np.abs(b.cpu().numpy() - want).max() / np.abs(want).max())
        print(f"  buffer {k}: err / max {e:.3e}")
        assert e <= 2e-5, k


def test_adamw_sequence_matches_reference(g16):
    t = C.TRAIN
    idx, target = C.train_batch()
    x, tg = T(golden_encode(g16, t["L"])[idx]), T(target)
    m = _train_model()
    opt = torch.optim.AdamW(m.parameters(), lr=0.001)
    sch = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.95)
    losses = []
    for k in range(C.ADAMW_STEPS):
        opt.zero_grad()
        loss, sums = fit2d.fit_loss(m(x), tg, t["reg"])
        loss.backward()
        opt.step()
        losses.append(float(sums[0]))
        if k + 1 == C.ADAMW_SCHED_AFTER:
            sch.step()
    e_l = float(np.abs(np.array(losses) / g16["adamw_losses"] - 1).max())
    head = m.model[3 * t["layer_num"]]
    e_w = float(np.abs(head.weight.detach().cpu().numpy() - g16["adamw_last_weight"]).max())
    e_b = float(np.abs(head.bias.detach().cpu().numpy() - g16["adamw_last_bias"]).max())
    print(f"AdamW x5: loss rel err {e_l:.3e}, last weight abs err {e_w:.3e}, last bias {e_b:.3e}")
    assert e_l <= 1e-4 and e_w <= 5e-5 and e_b <= 5e-5


def test_learning_and_fresh_pack_after_training():
    """20 steps on one batch of 512 at the default shape (10 x 256, L = 20) make the loss fall; afterwards model.eval() and
    get_picture must show the TRAINED net: the kernels write the running buffers through raw pointers, which torch's version
    counters do not see, so a pack cached before the steps would give a stale picture."""
    torch.manual_seed(0)
    L, W, H = 20, C.GRID_W, C.GRID_H
    m = fit2d.Model(4 * L + 2, 10).to(DEV)
    args = types.SimpleNamespace(L=L)
    pos = T(C.grid())
    g = torch.Generator().manual_seed(11)
    idx = torch.randperm(W * H, generator=g)[:512].to(DEV)
    tgt = (0.5 + 0.5 * torch.sin(pos[idx] * torch.tensor([0.31, 0.17], device=DEV))).repeat(1, 2)[:, :3].contiguous()
    x = fit2d.encode(pos, L)[idx].contiguous()
    pic0 = fit2d.get_picture(W, H, m.eval(), args)                      # caches a pack of the untrained net
    opt = torch.optim.AdamW(m.parameters(), lr=0.001)
    m.train()
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss, sums = fit2d.fit_loss(m(x), tgt, 0.1)
        loss.backward()
        opt.step()
        losses.append(sums[0])
    losses = torch.stack(losses).tolist()
    print(f"learning: loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert losses[-1] < 0.5 * losses[0]
    assert int(m.model[2].num_batches_tracked) == 20
    m.eval()
    pic1 = fit2d.get_picture(W, H, m, args)
    with torch.no_grad():
        lay = m.forward_layers(fit2d.encode(pos, L)).clamp(0, 1).cpu().numpy().reshape(H, W, 3)
    e = float(np.abs(pic1 - lay).max())
    print(f"after training: |picture - layer-by-layer eval| {e:.3e}; |picture - picture before| {np.abs(pic1 - pic0).max():.3e}")
    assert e <= FWD_GATE
    assert float(np.abs(pic1 - pic0).max()) > 1e-2
