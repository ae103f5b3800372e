"""csrc/generic_kernels.hip unit by unit against float64: the six GEMM kernels behind generic_launch (64 x 64 tiles and the
double-buffered 128 x 128 tiles on 4-byte or 16-byte loads, each as X . W^T and as A . B), their epilogues, the two elementwise
backward kernels, and generic._Linear under autograd.  The GEMMs are called through the C ABI with explicit pointers and leading
dimensions - generic.linear makes its input contiguous, so nothing else in the suite shows these kernels a leading dimension
above the row length or a base off 16-byte alignment.

Case table, dispatch restatement, operand builders and the gate are tests/generic_units_ref.py (its docstring derives the gate:
|got - ref64| <= (K + 2) u (|A| . |op(B)| + |bias|) per entry, u = 2^-24, plus elu.h's pinned 1.2e-7 under ELU);
tests/test_generic_units_host.py checks them on the CPU.  The operands are randn windows inside NaN, so a read outside the
logical operand poisons the output; the output is a window inside a guarded buffer, and every case also asserts that nothing
outside the [M, N] block changed a bit and that a second identical call gives equal bits (no atomics in these kernels).  Each
case prints its |got - ref64| / gate; the module prints the worst per kernel when it is done."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(os.path.dirname(HERE), "sw-nerf_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import generic_units_ref as GR    # noqa: E402
import wgrad_units_ref as WR      # noqa: E402
from swnerf import _lib, generic  # noqa: E402

pytestmark = pytest.mark.gpu
WORST = {}
U = GR.U
ACTS = ((GR.ACT_NONE, "none"), (GR.ACT_RELU, "relu"), (GR.ACT_ELU, "elu"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert (_lib.ACT_NONE, _lib.ACT_RELU, _lib.ACT_ELU) == (GR.ACT_NONE, GR.ACT_RELU, GR.ACT_ELU)
    yield torch.device("cuda:0")
    print("\n[generic units] worst |got - ref64| / gate per kernel (<= 1 passes):")
    for k in sorted(WORST):
        print(f"  {k:40s} {WORST[k]:.3e}")


def _note(key, what, r, n):
    WORST[key] = max(WORST.get(key, 0.0), r)
    print(f"{what}: |got - ref64| / gate = {r:.3e} (n = {n})")
    assert r <= 1.0, f"{what}: {r:.3e} of the gate (n = {n})"


def _at(t, floats):
    return ctypes.c_void_p(t.data_ptr() + 4 * floats)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _gemm(dev, c, o=None, act=GR.ACT_NONE, with_bias=True, entry=None):
    """The case's GEMM through the C ABI into a guarded [M, ldc] window.  BT: swnerf_linear (`entry` None; act NONE / RELU) or
    swnerf_linear_act; NN: swnerf_gemm_nn.  The gate, then the three invariants.  -> the [M, N] result"""
    L = _lib.lib()
    assert GR.generic_branch(c.M, c.N, c.K, c.lda, c.ldb, c.bt, c.a_off, c.b_off) == c.branch
    d = (o if o is not None else GR.operands(torch, c)).to(dev)
    assert d.abuf.data_ptr() % 16 == 0 and d.bbuf.data_ptr() % 16 == 0          # the offsets count from aligned buffers
    g = torch.Generator(device=dev).manual_seed(c.M + 131 * c.N + c.ldc)
    out = WR.Guarded(torch, (c.M, c.ldc), g, dev)
    a, b, y, st = _at(d.abuf, c.a_off), _at(d.bbuf, c.b_off), _lib.ptr(out.win), _lib.stream_of(d.abuf)
    bias = _lib.ptr(d.bias) if with_bias else None

    def call():
        if not c.bt:
            assert act == GR.ACT_NONE and not with_bias
            _lib.check(L.swnerf_gemm_nn(a, c.lda, c.M, c.K, b, c.ldb, c.N, y, c.ldc, st), "gemm_nn")
        elif entry is None:
            assert act != GR.ACT_ELU
            _lib.check(L.swnerf_linear(a, c.lda, c.M, c.K, b, bias, c.N, int(act == GR.ACT_RELU), y, c.ldc, st), "linear")
        else:
            _lib.check(L.swnerf_linear_act(a, c.lda, c.M, c.K, b, bias, c.N, act, y, c.ldc, st), "linear_act")
        torch.cuda.synchronize()

    call()
    got = out.win[:, :c.N].clone()
    ref, mag = d.reference(act, with_bias)
    what = f"{GR.case_id(c)} {dict(ACTS)[act]}{'' if with_bias or not c.bt else ' no bias'}{' linear_act' if entry else ''}"
    _note(c.branch, what, GR.gate_ratio(got, ref, mag, c.K), c.K + 2)
    assert out.untouched(), f"{what}: wrote outside the output window"
    assert _same_bits(out.win[:, c.N:], out.c0[:, c.N:]), f"{what}: wrote columns N..ldc"
    call()
    assert _same_bits(out.win[:, :c.N], got), f"{what}: a second call gave other bits"
    assert out.untouched() and _same_bits(out.win[:, c.N:], out.c0[:, c.N:])
    return got


# ======================================================================================================================
# a - c. every kernel at its tile, chunk and load-width edges
@pytest.mark.parametrize("c", GR.CASES, ids=GR.case_id)
def test_gemm_kernel_edges(dev, c):
    """generic_units_ref.CASES: the 64 x 64 kernels (ld = row + 3, bases one float off; odd K = a half-empty last MFMA step; N = 130
    below 128 rows = three column blocks), the 128 x 128 kernels on 4-byte loads (leading dimensions no multiple of 4; 257 x 260 =
    three blocks either way) and on 16-byte loads (K = 4 .. 100: the K edge inside, at and past a 32-chunk), X . W^T through
    swnerf_linear with its bias and A . B through swnerf_gemm_nn."""
    _gemm(dev, c, with_bias=c.bt)


# d. the guarded fall-back.  generic_launch computes `vec` from lda % 4, ldb % 4, both bases % 16, K % 4 and (NN) N % 4 BEFORE it picks
# a kernel, and the <.., false> kernels contain no 16-byte load, so none of these runs can issue a misaligned access.
@pytest.mark.parametrize("c", list(GR.VEC_BASE.values()) + GR.DISQUALIFIED, ids=GR.case_id)
def test_one_disqualifier_falls_back(dev, c):
    """From the 16-byte case 129 x 68 x 36 (run as it is first), one condition broken per run: lda + 1, ldb + 1 (NN; the weight
    of swnerf_linear has no leading dimension of its own), either base one float on, K = 35, N = 66 (NN).  The restated dispatch
    names the 4-byte kernel (asserted in _gemm against the case's `branch`), and the result passes the same gate."""
    assert c.branch.endswith(",true>") == (c.group == "vec")
    _gemm(dev, c, with_bias=c.bt)


# ======================================================================================================================
# e. epilogues
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("act", [a for a, _ in ACTS], ids=[n for _, n in ACTS])
@pytest.mark.parametrize("c", GR.EPILOGUE, ids=GR.case_id)
def test_epilogues(dev, c, act, with_bias):
    """NONE / RELU / ELU with a bias and with bias = NULL through swnerf_linear_act, on one case of the 64 x 64 kernel and one of
    each 128 x 128 variant; NONE and RELU through swnerf_linear's `relu` flag as well.  ELU on pre-activations of about [-8, 3]."""
    o = GR.elu_operands(torch, c) if act == GR.ACT_ELU else None
    got = _gemm(dev, c, o, act, with_bias, entry="linear_act")
    if act != GR.ACT_ELU:
        assert _same_bits(got, _gemm(dev, c, o, act, with_bias)), "swnerf_linear and swnerf_linear_act disagree"
    if act == GR.ACT_RELU:
        assert bool((got >= 0).all()) and bool((got == 0).any()) and bool((got > 0).any())
    if act == GR.ACT_ELU and with_bias:                 # (without the bias of -2.5 the range is about [-5, 5])
        assert bool((got > -1.0000002).all()) and bool((got < -0.99).any()) and bool((got > 1).any())


@pytest.mark.parametrize("c", GR.EPILOGUE, ids=GR.case_id)
def test_nan_in_x_stays_in_its_row(dev, c):
    """Non-finite behaviour as it is (include/swnerf.h states it): a NaN at x[r, k] makes exactly row r of the output NaN under
    NONE and ELU and no other entry leaves the gate; under RELU that row is 0, because fmaxf returns the non-NaN operand."""
    r, k = c.M // 2, c.K - 1
    others = [i for i in range(c.M) if i != r]
    for act, name in ACTS:
        o = GR.elu_operands(torch, c) if act == GR.ACT_ELU else GR.operands(torch, c)
        o.a[r, k] = float("nan")
        L, d = _lib.lib(), o.to(dev)
        out = WR.Guarded(torch, (c.M, c.ldc), torch.Generator(device=dev).manual_seed(c.M + act), dev)
        _lib.check(L.swnerf_linear_act(_at(d.abuf, c.a_off), c.lda, c.M, c.K, _at(d.bbuf, c.b_off), _lib.ptr(d.bias), c.N, act,
                                       _lib.ptr(out.win), c.ldc, _lib.stream_of(d.abuf)), "linear_act")
        torch.cuda.synchronize()
        got = out.win[:, :c.N]
        ref, mag = d.reference(act)
        _note(c.branch, f"{GR.case_id(c)} {name}, NaN at x[{r}, {k}], the other rows", GR.gate_ratio(got[others], ref[others], mag[others], c.K), c.K + 2)
        if act == GR.ACT_RELU:
            assert bool((_bits(got[r]) == 0).all()), "relu of a NaN row is +0"
        else:
            assert bool(torch.isnan(got[r]).all()), f"{name}: row {r} must be NaN"
        assert out.untouched() and _same_bits(out.win[:, c.N:], out.c0[:, c.N:])


# ======================================================================================================================
# f. the elementwise backward kernels
def _elementwise(dev, n, seed):
    """y (special values in turn, generic_units_ref.special_y) as a window of a larger buffer, dy in a guarded one"""
    y = GR.special_y(torch, n, torch.Generator().manual_seed(seed)).to(dev)
    g = torch.Generator(device=dev).manual_seed(seed + n)
    yb, dy = WR.Guarded(torch, (n,), g, dev), WR.Guarded(torch, (n,), g, dev)
    yb.win.copy_(y)
    return y, yb, dy


@pytest.mark.parametrize("n", GR.ELEMENTWISE_N)
def test_relu_mask(dev, n):
    """swnerf_relu_mask: dy = y > 0 ? dy : 0, bit for bit - +0.0, -0.0, -1.0 and NaN give +0, the smallest denormal passes dy;
    n around one 256-thread block and at 256 blocks + 1."""
    y, yb, dy = _elementwise(dev, n, 11)
    _lib.check(_lib.lib().swnerf_relu_mask(_lib.ptr(dy.win), _lib.ptr(yb.win), n, _lib.stream_of(y)), "relu_mask")
    torch.cuda.synchronize()
    want = torch.where(y > 0, dy.c0, torch.zeros_like(dy.c0))
    if n >= 8:
        assert bool((_bits(want[:2]) == 0).all()) and _same_bits(want[2], dy.c0[2]) and bool((_bits(want[3:5]) == 0).all())
    assert _same_bits(dy.win, want)
    assert dy.untouched() and yb.untouched() and _same_bits(yb.win, y)


@pytest.mark.parametrize("n", GR.ELEMENTWISE_N)
def test_elu_grad(dev, n):
    """swnerf_elu_grad: dy *= (y > 0 ? 1 : y + 1).  The kernel forms y + 1 in fp32 (exact for y <= -0.5 by Sterbenz, a rounding of
    relative size u above) and rounds the product once: against dy . fl32(y + 1) in float64 it is held to ONE rounding,
    u |dy (y + 1)|, and against dy . (y + 1) all in float64 to the two, (2 u + u^2) |dy (y + 1)|.  y > 0 (the smallest denormal
    included) passes dy bit for bit, y = -1 gives a zero, a NaN in y a NaN."""
    y, yb, dy = _elementwise(dev, n, 13)
    _lib.check(_lib.lib().swnerf_elu_grad(_lib.ptr(dy.win), _lib.ptr(yb.win), n, _lib.stream_of(y)), "elu_grad")
    torch.cuda.synchronize()
    got, d64, pos, nan = dy.win.double(), dy.c0.double(), y > 0, torch.isnan(y)
    assert _same_bits(dy.win[pos], dy.c0[pos])
    assert torch.equal(torch.isnan(dy.win), nan)
    ok = ~pos & ~nan
    one = torch.ones_like(d64)
    for what, fac, n_round in (("fl32(y + 1)", torch.where(pos, one, (y + 1.0).double()), 1.0),
                               ("y + 1 in float64", torch.where(pos, one, y.double() + 1.0), 2.0 + U)):
        want = d64 * fac
        err, gate = (got - want).abs()[ok], (n_round * U * want.abs())[ok]
        worst = float((err / gate.clamp_min(1e-300)).max()) if int(ok.sum()) else 0.0
        print(f"elu_grad n={n} vs dy . ({what}): |got - ref64| / gate = {worst:.3e}")
        assert bool((err <= gate).all()), what
    if n >= 8:
        assert float(dy.win[3]) == 0.0
    assert dy.untouched() and yb.untouched() and _same_bits(yb.win, y)


# ======================================================================================================================
# g. generic._Linear under autograd
class _Spy:
    """Counts the C entry points that get called (the pattern of tests/test_gpu_dnerf_train.py)."""

    def __init__(self, lib, calls):
        object.__setattr__(self, "_l", lib)
        object.__setattr__(self, "_calls", calls)

    def __getattr__(self, name):
        f = getattr(self._l, name)
        if not name.startswith("swnerf_"):
            return f

        def wrapped(*a, **k):
            self._calls[name] = self._calls.get(name, 0) + 1
            return f(*a, **k)
        return wrapped


def _spy(monkeypatch):
    calls = {}
    real = _lib.lib()
    while isinstance(real, _Spy):
        real = real._l
    spy = _Spy(real, calls)
    monkeypatch.setattr(_lib, "lib", lambda: spy)
    return calls


def _layer(dev, M, K, N, with_bias, seed, grad=(True, True)):
    """x [M, K], W [N, K] (pre-activations of standard deviation 1.3), b [N], dY [M, N]"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((M, K), generator=g).to(dev).requires_grad_(grad[0])
    w = (torch.randn((N, K), generator=g) * (1.3 / K ** 0.5)).to(dev).requires_grad_(grad[1])
    b = (torch.randn((N,), generator=g) * 0.5).to(dev).requires_grad_(grad[1]) if with_bias else None
    return x, w, b, torch.randn((M, N), generator=g).to(dev)


def _forward_gate(what, y, x, w, b, act):
    x64, w64 = x.detach().double(), w.detach().double()
    ref, mag = x64 @ w64.T, x64.abs() @ w64.abs().T
    if b is not None:
        ref, mag = ref + b.detach().double(), mag + b.detach().double().abs()
    K = x.shape[1]
    if act == GR.ACT_RELU:
        ref = ref.clamp_min(0)
    elif act == GR.ACT_ELU:
        ref, mag = torch.where(ref > 0, ref, torch.expm1(ref)), mag + GR.ELU_ABS / ((K + 2) * U)
    _note("_Linear forward", f"{what} y", GR.gate_ratio(y.detach(), ref, mag, K), K + 2)


def _masked(dY, y, act):
    """dY' in float64 from the kernel's own fp32 y: neither the forward's rounding nor a ReLU flip enters the backward check"""
    d64, y = dY.double(), y.detach()
    if act == GR.ACT_RELU:
        return d64 * (y > 0)
    if act == GR.ACT_ELU:
        return d64 * torch.where(y > 0, torch.ones_like(d64), y.double() + 1.0)
    return d64


def _backward_gates(what, x, w, b, dYp, dx, dw, db):
    """dX within (N + 3) u |dY'| |W|: N products and N - 1 additions, two roundings of dY' itself (the ELU factor), one to spare;
    dW / db within (M + 514) u: the bound of tests/test_gemm_tn_ordered.py"""
    M, N = dYp.shape
    x64, w64 = x.detach().double(), w.detach().double()
    if dx is not None:
        _note("_Linear dX", f"{what} dX", WR.ratio(dx, dYp @ w64, dYp.abs() @ w64.abs(), N + 3), N + 3)
    if dw is not None:
        _note("_Linear dW", f"{what} dW", WR.ratio(dw, dYp.T @ x64, dYp.abs().T @ x64.abs(), M + 514), M + 514)
    if db is not None:
        _note("_Linear db", f"{what} db", WR.ratio(db, dYp.sum(0), dYp.abs().sum(0), M + 514), M + 514)


def _train_once(x, w, b, act, ordered, dY=None):
    for t in (x, w, b):
        if t is not None:
            t.grad = None
    y = generic._Linear.apply(x, w, b, act, ordered)
    if dY is None:
        y.sum().backward()                                  # dY arrives as a stride-0 expand of one float
    else:
        y.backward(dY)
    torch.cuda.synchronize()
    return y, x.grad, w.grad, None if b is None else b.grad


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("ordered", [False, True], ids=["atomic", "ordered"])
@pytest.mark.parametrize("act", [a for a, _ in ACTS], ids=[n for _, n in ACTS])
def test_linear_autograd(dev, act, ordered, with_bias):
    """130 x 37 -> 70: y against float64 with the GEMM's gate; dX, dW, db against float64 evaluated at the kernel's own y.  With
    ordered=True two backward passes give equal bits."""
    M, K, N = 130, 37, 70
    x, w, b, dY = _layer(dev, M, K, N, with_bias, 100 + 10 * act + ordered)
    what = f"_Linear {M}x{K}->{N} {dict(ACTS)[act]} {'ordered' if ordered else 'atomic'}{'' if with_bias else ' no bias'}"
    y, dx, dw, db = _train_once(x, w, b, act, ordered, dY)
    assert (db is None) == (not with_bias)
    _forward_gate(what, y, x, w, b, act)
    _backward_gates(what, x, w, b, _masked(dY, y, act), dx, dw, db)
    if ordered:
        y2, dx2, dw2, db2 = _train_once(x, w, b, act, ordered, dY)
        assert _same_bits(y, y2) and _same_bits(dx, dx2) and _same_bits(dw, dw2) and (db is None or _same_bits(db, db2))


@pytest.mark.parametrize("N", [257, 260])
def test_linear_autograd_second_gemm_tn_call(dev, monkeypatch, N):
    """More than 256 outputs on the atomic path: two swnerf_gemm_tn calls, the second with 1 (N = 257) and 4 (N = 260) rows of dW
    at o0 = 256, its A operand a column window of dY at an offset of 256 floats."""
    calls = _spy(monkeypatch)
    M, K = 130, 37
    x, w, b, dY = _layer(dev, M, K, N, True, N)
    y, dx, dw, db = _train_once(x, w, b, GR.ACT_RELU, False, dY)
    assert calls.get("swnerf_gemm_tn") == 2 and calls.get("swnerf_gemm_nn") == 1 and "swnerf_gemm_tn_ordered" not in calls
    what = f"_Linear {M}x{K}->{N} relu atomic"
    _forward_gate(what, y, x, w, b, GR.ACT_RELU)
    dYp = _masked(dY, y, GR.ACT_RELU)
    assert bool((dYp[:, 256:] != 0).any())
    _backward_gates(what, x, w, b, dYp, dx, dw, db)


@pytest.mark.parametrize("act", [GR.ACT_NONE, GR.ACT_RELU], ids=["none", "relu"])
def test_linear_autograd_expanded_dy(dev, act):
    """loss = y.sum(): autograd hands backward() a stride-0 expand of a single 1.0, which _c32 must copy before a kernel reads it
    with a leading dimension of N."""
    M, K, N = 130, 37, 70
    x, w, b, _ = _layer(dev, M, K, N, True, 7 + act)
    y, dx, dw, db = _train_once(x, w, b, act, False, None)
    what = f"_Linear {M}x{K}->{N} {dict(ACTS)[act]}, loss = y.sum()"
    _backward_gates(what, x, w, b, _masked(torch.ones_like(y), y, act), dx, dw, db)


class _Ctx:
    pass


def test_linear_backward_launches_only_what_is_needed(dev, monkeypatch):
    """Frozen weights: backward returns dw = db = None and calls no swnerf_gemm_tn* entry.  x without a gradient: dx is None and
    swnerf_gemm_nn is not called.  Both through autograd (launch counts, the gradients that remain inside their gates) and on
    _Linear.backward itself (the returned tuple)."""
    M, K, N = 130, 37, 70
    calls = _spy(monkeypatch)
    x, w, b, dY = _layer(dev, M, K, N, True, 21, grad=(True, False))
    y, dx, dw, db = _train_once(x, w, b, GR.ACT_RELU, False, dY)
    assert dw is None and db is None
    assert not [k for k in calls if k.startswith("swnerf_gemm_tn")] and calls.get("swnerf_gemm_nn") == 1 and calls.get("swnerf_relu_mask") == 1
    _backward_gates("_Linear frozen weights", x, w, b, _masked(dY, y, GR.ACT_RELU), dx, None, None)
    calls.clear()
    x, w, b, dY = _layer(dev, M, K, N, True, 22, grad=(False, True))
    y, dx, dw, db = _train_once(x, w, b, GR.ACT_RELU, True, dY)
    assert dx is None and "swnerf_gemm_nn" not in calls and calls.get("swnerf_gemm_tn_ordered") == 1 and "swnerf_gemm_tn" not in calls
    _backward_gates("_Linear x without grad", x, w, b, _masked(dY, y, GR.ACT_RELU), None, dw, db)
    # the returned tuple itself
    ctx = _Ctx()
    ctx.saved_tensors, ctx.act, ctx.ordered, ctx.has_bias = (x.detach(), w.detach(), y.detach()), GR.ACT_RELU, False, True
    for needs, n_nn, n_tn in (((True, False, False, False, False), 1, 0), ((False, True, True, False, False), 0, 1),
                              ((False, False, True, False, False), 0, 1), ((False, False, False, False, False), 0, 0)):
        calls.clear()
        ctx.needs_input_grad = needs
        gdx, gdw, gdb, g3, g4 = generic._Linear.backward(ctx, dY)
        torch.cuda.synchronize()
        assert (gdx is not None) == needs[0] and (gdw is not None) == (needs[1] or needs[2]) and (gdb is not None) == (needs[1] or needs[2])
        assert g3 is None and g4 is None
        assert calls.get("swnerf_gemm_nn", 0) == n_nn and calls.get("swnerf_gemm_tn", 0) == n_tn, (needs, calls)
        _backward_gates(f"_Linear.backward needs={needs[:3]}", x, w, b, _masked(dY, y, GR.ACT_RELU), gdx, gdw, gdb)
