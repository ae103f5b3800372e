"""csrc/wgrad_kernels.hip unit by unit against float64: every branch of swnerf_gemm_tn's dispatch, the two one-pass narrow
kernels (swnerf_deform_narrow_grads = narrow_plan_kernel, swnerf_canon_narrow_grads = narrow5_kernel), the slot -> column
scatters (swnerf_unslot_grad, swnerf_unslot_grad_time) and the two un-fold kernels (swnerf_feature_finish,
swnerf_tnerf_feature_finish), called through the C ABI.

The gate is the one of tests/test_gemm_tn_ordered.py, per entry and from the number format alone: the kernels sum fp32 products
in fp32 and combine the workgroups' slices with float atomics, so with u = 2^-24 and n = M + 514 (at most M additions inside the
slices, at most 512 slices, the add into C)
    |got - ref64| <= n u (|A|^T |B| + |C0|)        and        |bias - ref64| <= n u (sum |A| + |b0|),
C0 / b0 the non-zero content accumulated into.  The un-fold kernels' sums have a fixed length K: n = K + 2 there (each test's
docstring counts its K).  Every output is a window inside a larger buffer of non-zero floats, and everything outside the window
must come back bit for bit: that is how this module sees a stray write (it makes no claim about stray reads).  Each test prints
its worst |got - ref| / gate per product; the module prints the worst of all when it is done."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(os.path.dirname(HERE), "sw-nerf_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import tnerf_train_ref as TR    # noqa: E402
import wgrad_units_ref as WR    # noqa: E402
from swnerf import _lib         # noqa: E402

pytestmark = pytest.mark.gpu
WORST = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    yield torch.device("cuda:0")
    print("\n[wgrad units] worst |got - ref64| / gate per product (<= 1 passes):")
    for k in sorted(WORST):
        print(f"  {k:34s} {WORST[k]:.3e}")


def _gate(what, got, ref, mag, n):
    """one product inside its gate; the ratio goes to the printed table first"""
    r = WR.ratio(got, ref, mag, n)
    WORST[what] = max(WORST.get(what, 0.0), r)
    print(f"{what}: |got - ref64| / gate = {r:.3e} (n = {n})")
    assert r <= 1.0, f"{what}: {r:.3e} of the gate (n = {n})"


def _at(t, floats):
    return ctypes.c_void_p(t.data_ptr() + 4 * floats)


# ======================================================================================================================
# 1. swnerf_gemm_tn: one case per dispatch branch.  (No, Ni, layout); the kernel named next to each group is what the case is meant
# to reach at M >= 4096 - test_gemm_tn_branch asserts it against the restated branch list (wgrad_units_ref.gemm_tn_branch).
# layouts (lda, a_col, ldb, b_col): "win" = A columns 4.. of [M, No + 12], B columns 8.. of [M, Ni + 8] (16-byte aligned windows
# whenever No and Ni are multiples of 4); "act" = windows of two [M, 2432] buffers like `grad` / `act`.
def _layout(kind, No, Ni):
    return {"win": (No + 12, 4, Ni + 8, 8),
            "act": (2432, 512, 2432, 1024),
            "act_off1": (2432, 513, 2432, 1024),            # A one float off 16-byte alignment
            "draw_col3": (4, 3, Ni + 8, 8),                  # A = column 3 of a [M, 4] tensor (d sigma of d raw)
            "draw_cols012": (4, 0, Ni + 8, 8),               # A = columns 0..2 of one (d rgb of d raw)
            "draw_x90": (4, 0, 90, 0)}[kind]                 # ... against x[:, :63] with ld 90


GEMM_CASES = [
    # the tiled wave grids: first and last shape of each, and the T-NeRF / step shapes on them
    ("gemm_tn_tiled_kernel<1,1,1,4>", 4, 4, "win"), ("gemm_tn_tiled_kernel<1,1,1,4>", 32, 128, "win"),
    ("gemm_tn_tiled_kernel<1,1,1,4>", 4, 64, "win"),
    ("gemm_tn_tiled_kernel<1,2,1,4>", 4, 132, "win"), ("gemm_tn_tiled_kernel<1,2,1,4>", 32, 256, "win"),
    ("gemm_tn_tiled_kernel<1,1,4,1>", 36, 4, "win"), ("gemm_tn_tiled_kernel<1,1,4,1>", 128, 32, "win"),
    ("gemm_tn_tiled_kernel<1,1,4,1>", 64, 32, "win"),
    ("gemm_tn_tiled_kernel<1,1,8,1>", 132, 32, "win"), ("gemm_tn_tiled_kernel<1,1,8,1>", 256, 32, "win"),
    ("gemm_tn_tiled_kernel<1,1,8,2>", 36, 36, "win"), ("gemm_tn_tiled_kernel<1,1,8,2>", 256, 64, "win"),
    # the first shapes past the grids
    ("gemm_tn_kernel<true,true>", 36, 68, "win"), ("gemm_tn_kernel<true,true>", 128, 96, "win"),
    ("gemm_tn_kernel<true,true>", 128, 128, "win"), ("gemm_tn_kernel<true,true>", 64, 128, "win"),
    ("gemm_tn_kernel<true,true>", 128, 256, "win"),
    # the 4-byte-DMA variants
    ("gemm_tn_kernel<true,false>", 128, 283, "win"),
    ("gemm_tn_kernel<false,true>", 1, 256, "draw_col3"), ("gemm_tn_kernel<false,true>", 3, 128, "draw_cols012"),
    ("gemm_tn_kernel<false,false>", 3, 63, "draw_x90"),
    # grid y = 3 (three column blocks) and 6 (three column blocks x two halves of C's rows)
    ("gemm_tn_kernel<true,true>", 4, 600, "win"), ("gemm_tn_kernel<true,true>", 256, 600, "win"),
    # the 256 x 256 DMA kernel
    ("gemm_tn_dma_kernel<false>", 256, 256, "act"),
]
ALIGNED = [c for c in GEMM_CASES if c[3] in ("win", "act") and c[1] % 4 == 0 and c[2] % 4 == 0]
NO_BIAS = [GEMM_CASES[i] for i in (1, 4, 6, 9, 11, 14, 17, 18, 20, 23)]        # one per branch
SWEEP = [("gemm_tn_tiled_kernel<1,1,8,2>", 256, 64, "win"), ("gemm_tn_tiled_kernel<1,2,1,4>", 4, 256, "win"),
         ("gemm_tn_dma_kernel<false>", 256, 256, "act")]
_id = lambda c: f"{c[1]}x{c[2]}-{c[3]}"


def _gemm(dev, M, No, Ni, lay, with_bias=True, A=None):
    """swnerf_gemm_tn on column windows of wider A / B into the window [1:1+No, 5:5+Ni] of a non-zero C and [3:3+No] of a non-zero
    bias buffer; gate, then everything outside the windows bit-unchanged.  Returns (A buffer, C window, its gate)."""
    L = _lib.lib()
    lda, a_col, ldb, b_col = lay
    g = torch.Generator(device=dev).manual_seed(1000003 * No + 1009 * Ni + M + lda)
    ldc = Ni + 9
    B = torch.randn((M, ldb), generator=g, device=dev)
    Cb = torch.randn((No + 2, ldc), generator=g, device=dev)
    bb = torch.randn((No + 7,), generator=g, device=dev)
    if A is None:
        A = torch.randn((M, lda), generator=g, device=dev)
    C0, b0 = Cb.clone(), bb.clone()
    _lib.check(L.swnerf_gemm_tn(_at(A, a_col), lda, No, _at(B, b_col), ldb, Ni, M, _at(Cb, ldc + 5), ldc,
                                _at(bb, 3) if with_bias else None, _lib.stream_of(A)), "gemm_tn")
    torch.cuda.synchronize()
    a64, b64 = A[:, a_col:a_col + No].double(), B[:, b_col:b_col + Ni].double()
    c0 = C0[1:1 + No, 5:5 + Ni].double()
    n = M + 514
    tag = f"gemm_tn {No}x{Ni}"
    mag = a64.abs().T @ b64.abs() + c0.abs()
    _gate(tag + " C", Cb[1:1 + No, 5:5 + Ni], c0 + a64.T @ b64, mag, n)
    outside = torch.ones_like(Cb, dtype=torch.bool)
    outside[1:1 + No, 5:5 + Ni] = False
    assert torch.equal(Cb[outside], C0[outside]), "C was written outside its window"
    if with_bias:
        _gate(tag + " bias", bb[3:3 + No], b0[3:3 + No].double() + a64.sum(0), a64.abs().sum(0) + b0[3:3 + No].double().abs(), n)
        assert torch.equal(bb[:3], b0[:3]) and torch.equal(bb[3 + No:], b0[3 + No:]), "bias was written outside its window"
    else:
        assert torch.equal(bb, b0)
    return A, Cb[1:1 + No, 5:5 + Ni], n * WR.U * mag


@pytest.mark.parametrize("case", GEMM_CASES, ids=_id)
def test_gemm_tn_branch(dev, case):
    """Every branch of swnerf_gemm_tn at M = 4097: 32-row slices, the last workgroup with a single row.  The case's kernel is
    asserted against the restated branch list, so the table above cannot drift from what it claims to reach."""
    kernel, No, Ni, kind = case
    lay = _layout(kind, No, Ni)
    assert WR.gemm_tn_branch(No, Ni, 4097, *lay) == kernel
    if (No, Ni) in ((4, 600), (256, 600)):
        assert WR.gemm_tn_grid_y(No, Ni) == (3 if No == 4 else 6)
    _gemm(dev, 4097, No, Ni, lay)


@pytest.mark.parametrize("case", ALIGNED, ids=_id)
def test_gemm_tn_small_batch(dev, case):
    """The same aligned shapes at M = 33 - below the 4096-row threshold they all go through gemm_tn_kernel<true,true>, the path
    every small training batch takes: one workgroup, a full slab and a one-row slab."""
    _, No, Ni, kind = case
    lay = _layout(kind, No, Ni)
    assert WR.gemm_tn_branch(No, Ni, 33, *lay) == "gemm_tn_kernel<true,true>"
    _gemm(dev, 33, No, Ni, lay)


@pytest.mark.parametrize("M", [1, 31, 32, 33, 4095, 4096, 50007])
@pytest.mark.parametrize("case", SWEEP, ids=_id)
def test_gemm_tn_row_counts(dev, case, M):
    """Row counts around a slab (31 / 32 / 33), a single row, both sides of the 4095 / 4096 switch between gemm_tn_kernel and the
    double-buffered kernels, and ragged slices (50 007 rows: 224-row slices on the tiled / DMA kernels, the last one short)."""
    kernel, No, Ni, kind = case
    lay = _layout(kind, No, Ni)
    assert WR.gemm_tn_branch(No, Ni, M, *lay) == (kernel if M >= 4096 else "gemm_tn_kernel<true,true>")
    _gemm(dev, M, No, Ni, lay)


@pytest.mark.parametrize("case", NO_BIAS, ids=_id)
def test_gemm_tn_without_bias(dev, case):
    """One case per branch with bias = NULL: C inside the gate, the bias buffer untouched."""
    kernel, No, Ni, kind = case
    lay = _layout(kind, No, Ni)
    assert WR.gemm_tn_branch(No, Ni, 4097, *lay) == kernel
    _gemm(dev, 4097, No, Ni, lay, with_bias=False)


def test_gemm_tn_misaligned_a_falls_back(dev):
    """256 x 256 at M = 4096 with A one float off 16-byte alignment: gemm_tn_kernel<false,true> instead of the DMA kernel, the same
    sums - both inside the gate against the same float64 product (the same A values, shifted by one column in their buffer)."""
    lay, off = _layout("act", 256, 256), _layout("act_off1", 256, 256)
    assert WR.gemm_tn_branch(256, 256, 4096, *lay) == "gemm_tn_dma_kernel<false>"
    assert WR.gemm_tn_branch(256, 256, 4096, *off) == "gemm_tn_kernel<false,true>"
    A, c_dma, gate = _gemm(dev, 4096, 256, 256, lay)
    A1 = torch.empty_like(A)
    A1[:, 1:] = A[:, :-1]
    A1[:, 0] = 1.0
    _, c_off, _ = _gemm(dev, 4096, 256, 256, off, A=A1)
    assert torch.equal(A1[:, 513:769], A[:, 512:768])
    # the same B, C0 and A values in both runs (one seed): two roundings of ONE float64 product, each inside the gate above, so
    # within twice the gate of each other
    assert bool(((c_dma.double() - c_off.double()).abs() <= 2 * gate).all())


# ======================================================================================================================
# 2. the one-pass narrow kernels
RAGGED = [1, 7, 15, 16, 17, 4097, 49157]      # < a 16-row slab | one slab less a row | one slab | a one-row tail | 32-row slices,
#                                               the last workgroup one row | 208-row slices, the last one short (69 rows)


def _narrow_inputs(dev, M, ldg, lda, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=g, device=dev)
    rows = max(M, 1)
    return g, r(rows, ldg), r(rows, lda), r(rows, WR.XS_LD), r(rows, 4)


def _narrow_check(what, M, outs, products, sums):
    """outs: name -> Guarded; products: name -> (A64, B64); sums: name -> A64"""
    n = M + 514
    for k, (a, b) in products.items():
        c0 = outs[k].c0.double()
        _gate(f"{what} {k}", outs[k].win, c0 + a.T @ b, a.abs().T @ b.abs() + c0.abs(), n)
    for k, a in sums.items():
        c0 = outs[k].c0.double()
        _gate(f"{what} {k}", outs[k].win, c0 + a.sum(0), a.abs().sum(0) + c0.abs(), n)
    for k, o in outs.items():
        assert o.untouched(), f"{what}: wrote outside {k}"


def _deform(dev, M, ldg, lda):
    L = _lib.lib()
    g, grad, act, xs, gdx = _narrow_inputs(dev, M, ldg, lda, 7 * M + ldg + 3 * lda)
    outs = {k: WR.Guarded(torch, s, g, dev) for k, s in (("c0s", (256, 64)), ("cts", (256, 32)), ("w4", (4, 256)), ("b_l0", (256,)), ("b4", (4,)))}
    _lib.check(L.swnerf_deform_narrow_grads(_lib.ptr(grad), ldg, _lib.ptr(act), lda, _lib.ptr(xs), _lib.ptr(gdx), M,
                                            *[_lib.ptr(outs[k].win) for k in ("c0s", "cts", "w4", "b_l0", "b4")], _lib.stream_of(grad)),
               "deform_narrow_grads")
    torch.cuda.synchronize()
    dp0, h7, x, gd = grad[:, :256].double(), act[:, 1792:2048].double(), xs.double(), gdx.double()
    _narrow_check("deform_narrow", M, outs, dict(c0s=(dp0, x[:, :64]), cts=(dp0, x[:, 64:96]), w4=(gd, h7)), dict(b_l0=dp0, b4=gd))


@pytest.mark.parametrize("M", RAGGED)
def test_deform_narrow_grads(dev, M):
    """swnerf_deform_narrow_grads (narrow_plan_kernel) against float64: c0s += d pre_0^T xs[:, :64], cts += d pre_0^T xs[:, 64:96],
    w4 += g_dx^T h7 (ALL four rows: the fourth column of g_dx is non-zero here), b_l0 += sum d pre_0, b4 += sum g_dx, into
    non-zero outputs, over the ragged row counts of RAGGED."""
    _deform(dev, M, WR.ACT_LD, WR.ACT_LD)


@pytest.mark.parametrize("M,ldg,lda", [(4097, 2436, 2436), (4097, 2440, 2432), (17, 2432, 2444)])
def test_deform_narrow_grads_leading_dimensions(dev, M, ldg, lda):
    """Leading dimensions above 2432, equal and unequal for grad_d and act_d."""
    _deform(dev, M, ldg, lda)


def test_deform_narrow_grads_refusals(dev):
    """Refused before anything is launched - outputs bit-unchanged: a leading dimension below 2432 or no multiple of 4, a
    misaligned xs_d, M < 0.  M == 0 returns 0 and does nothing."""
    L = _lib.lib()
    g, grad, act, xs, gdx = _narrow_inputs(dev, 16, 2440, 2440, 11)
    xs = torch.randn((17, WR.XS_LD), generator=g, device=dev)
    outs = [WR.Guarded(torch, s, g, dev) for s in ((256, 64), (256, 32), (4, 256), (256,), (4,))]
    o = [_lib.ptr(t.win) for t in outs]
    st = _lib.stream_of(grad)
    f = L.swnerf_deform_narrow_grads
    bad = {"ldg < 2432": (_lib.ptr(grad), 2428, _lib.ptr(act), 2432, _lib.ptr(xs), _lib.ptr(gdx), 16),
           "lda < 2432": (_lib.ptr(grad), 2432, _lib.ptr(act), 2428, _lib.ptr(xs), _lib.ptr(gdx), 16),
           "ldg % 4": (_lib.ptr(grad), 2433, _lib.ptr(act), 2432, _lib.ptr(xs), _lib.ptr(gdx), 16),
           "lda % 4": (_lib.ptr(grad), 2432, _lib.ptr(act), 2434, _lib.ptr(xs), _lib.ptr(gdx), 16),
           "xs_d off alignment": (_lib.ptr(grad), 2432, _lib.ptr(act), 2432, _at(xs, 1), _lib.ptr(gdx), 16),
           "M < 0": (_lib.ptr(grad), 2432, _lib.ptr(act), 2432, _lib.ptr(xs), _lib.ptr(gdx), -1)}
    for k, a in bad.items():
        assert f(*a, *o, st) == -1 and b"deform_narrow_grads" in L.swnerf_last_error(), k
    assert f(_lib.ptr(grad), 2432, _lib.ptr(act), 2432, _lib.ptr(xs), _lib.ptr(gdx), 0, *o, st) == 0
    torch.cuda.synchronize()
    assert all(t.unchanged() for t in outs)


@pytest.mark.parametrize("M", RAGGED)
def test_canon_narrow_grads(dev, M):
    """swnerf_canon_narrow_grads (narrow5_kernel) over the same ragged row counts, each of its five products and four biases held
    to the per-entry gate."""
    L = _lib.lib()
    g, grad, act, xs, d_out = _narrow_inputs(dev, M, WR.ACT_LD, WR.ACT_LD, 13 * M + 5)
    names = ("c0s", "cvs", "G", "a4w", "rgb4", "b_l0", "b_hv", "a4b", "rgb4b")
    shapes = ((256, 64), (128, 32), (128, 256), (4, 256), (4, 128), (256,), (128,), (4,), (4,))
    outs = {k: WR.Guarded(torch, s, g, dev) for k, s in zip(names, shapes)}
    _lib.check(L.swnerf_canon_narrow_grads(_lib.ptr(grad), WR.ACT_LD, _lib.ptr(act), WR.ACT_LD, _lib.ptr(xs), _lib.ptr(d_out), M,
                                           *[_lib.ptr(outs[k].win) for k in names], _lib.stream_of(grad)), "canon_narrow_grads")
    torch.cuda.synchronize()
    dp0, dphv, h7, hv = grad[:, :256].double(), grad[:, 2304:2432].double(), act[:, 1792:2048].double(), act[:, 2304:2432].double()
    x, dr = xs.double(), d_out.double()
    _narrow_check("canon_narrow", M, outs, dict(c0s=(dp0, x[:, :64]), cvs=(dphv, x[:, 64:96]), G=(dphv, h7), a4w=(dr, h7), rgb4=(dr, hv)),
                  dict(b_l0=dp0, b_hv=dphv, a4b=dr, rgb4b=dr))


# ======================================================================================================================
# 3. slot order -> reference columns
SENTINEL = -7777.0


def _unslot(dev, rows, nslots, cols, col0, ncols, call):
    """Cs [rows, nslots + 3] of distinct integers -> rows 1..rows of a sentinel-filled W [rows + 2, col0 + ncols + 5]; bit equality
    with the numpy scatter (every reference column exactly once, pad slots dropped, everything else still the sentinel)."""
    ld_s, ldw = nslots + 3, col0 + ncols + 5
    cs = np.arange(1, rows * ld_s + 1, dtype=np.float32).reshape(rows, ld_s)
    want = np.full((rows + 2, ldw), SENTINEL, np.float32)
    assert WR.scatter(cs[:, :nslots], cols, want[1:1 + rows], col0) == list(range(ncols))
    Cs = torch.from_numpy(cs).to(dev)
    W = torch.full((rows + 2, ldw), SENTINEL, device=dev)
    _lib.check(call(_lib.ptr(Cs), ld_s, rows, _at(W, ldw), ldw, col0, _lib.stream_of(W)), "unslot")
    got = W.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("rows", [1, 128, 256])
def test_unslot_grad_position_block(dev, rows):
    """swnerf_unslot_grad on the gamma(x) slots (slot0 = 0, nslots = 64) for every (L_pos, L_dir) in 0..10 x 0..4."""
    L = _lib.lib()
    for Lp in range(11):
        for Ld in range(5):
            cols = [WR.xs_col(f, Lp, Ld) for f in range(64)]
            _unslot(dev, rows, 64, cols, 0, 3 * (1 + 2 * Lp),
                    lambda cs, ld_s, r, w, ldw, col0, st: L.swnerf_unslot_grad(cs, ld_s, r, 0, 64, Lp, Ld, w, ldw, col0, st))


@pytest.mark.parametrize("rows", [1, 128, 256])
def test_unslot_grad_direction_block(dev, rows):
    """swnerf_unslot_grad on the gamma(d) slots (slot0 = 64, nslots = 32) behind 256 feature columns (col0 = 256), every band pair."""
    L = _lib.lib()
    for Lp in range(11):
        for Ld in range(5):
            cols = [WR.xs_col(64 + f, Lp, Ld) for f in range(32)]
            _unslot(dev, rows, 32, cols, 256, 3 * (1 + 2 * Ld),
                    lambda cs, ld_s, r, w, ldw, col0, st: L.swnerf_unslot_grad(cs, ld_s, r, 64, 32, Lp, Ld, w, ldw, col0, st))


@pytest.mark.parametrize("rows", [1, 128, 256])
def test_unslot_grad_time_block(dev, rows):
    """swnerf_unslot_grad_time for every L_time in 0..10, behind the gamma(x) columns of an L_pos = 10 - L_time embedding
    (col0 = 3 (1 + 2 L_pos))."""
    L = _lib.lib()
    for Lt in range(11):
        cols = [WR.time_slot_col(f, Lt) for f in range(32)]
        _unslot(dev, rows, 32, cols, 3 * (1 + 2 * (10 - Lt)), 1 + 2 * Lt,
                lambda cs, ld_s, r, w, ldw, col0, st: L.swnerf_unslot_grad_time(cs, ld_s, r, 32, Lt, w, ldw, col0, st))


# ======================================================================================================================
# 4. the un-fold kernels
def _finish(dev, what, fn, Hv, Hf, ld):
    """Shared by the two kernels: view layer [Hv, ld] whose first Hf columns take `feature` [Hf, Hf]; the fixed sum lengths K are
    those of the kernel's loops: dWv Hf terms of G . W_f^T plus the outer product (K = Hf + 1), dW_f and db_f Hv terms (K = Hv),
    the alpha / density row a single term (K = 1); n = K + 2."""
    L = _lib.lib()
    g = torch.Generator(device=dev).manual_seed(Hv + ld)
    r = lambda *s: torch.randn(s, generator=g, device=dev)
    G, db, Wv, W_f, b_f, a4w, a4b = r(Hv, Hf), r(Hv), r(Hv, ld), r(Hf, Hf), r(Hf), r(4, Hf), r(4)
    o = {k: WR.Guarded(torch, s, g, dev) for k, s in (("dWv", (Hv, ld)), ("dW_f", (Hf, Hf)), ("db_f", (Hf,)), ("dW_a", (1, Hf)), ("db_a", (1,)))}
    _lib.check(fn(_lib.ptr(G), _lib.ptr(db), _lib.ptr(Wv), ld, _lib.ptr(W_f), _lib.ptr(b_f), _lib.ptr(a4w), _lib.ptr(a4b),
                  _lib.ptr(o["dWv"].win), ld, _lib.ptr(o["dW_f"].win), _lib.ptr(o["db_f"].win), _lib.ptr(o["dW_a"].win), _lib.ptr(o["db_a"].win),
                  _lib.stream_of(G)), what)
    torch.cuda.synchronize()
    c = lambda t: t.double().cpu()
    G64, db64, Wvf, Wf64, bf64 = c(G), c(db), c(Wv)[:, :Hf], c(W_f), c(b_f)
    uW, uWf, ubf = (torch.from_numpy(a) for a in TR.unfold(G64.numpy(), db64.numpy(), Wvf.numpy(), Wf64.numpy(), bf64.numpy()))
    c0 = {k: c(v.c0) for k, v in o.items()}
    _gate(f"{what} dWv", c(o["dWv"].win)[:, :Hf], c0["dWv"][:, :Hf] + uW,
          G64.abs() @ Wf64.abs().T + torch.outer(db64.abs(), bf64.abs()) + c0["dWv"][:, :Hf].abs(), Hf + 3)
    _gate(f"{what} dW_f", c(o["dW_f"].win), c0["dW_f"] + uWf, Wvf.abs().T @ G64.abs() + c0["dW_f"].abs(), Hv + 2)
    _gate(f"{what} db_f", c(o["db_f"].win), c0["db_f"] + ubf, Wvf.abs().T @ db64.abs() + c0["db_f"].abs(), Hv + 2)
    _gate(f"{what} dW_alpha", c(o["dW_a"].win), c0["dW_a"] + c(a4w)[3:4], c(a4w)[3:4].abs() + c0["dW_a"].abs(), 3)
    _gate(f"{what} db_alpha", c(o["db_a"].win), c0["db_a"] + c(a4b)[3:4], c(a4b)[3:4].abs() + c0["db_a"].abs(), 3)
    assert torch.equal(o["dWv"].win[:, Hf:], o["dWv"].c0[:, Hf:]), "columns past the feature block were written"
    for k, v in o.items():
        assert v.untouched(), f"{what}: wrote outside {k}"


def test_tnerf_feature_finish(dev):
    """swnerf_tnerf_feature_finish against tnerf_train_ref.unfold plus the density row (dW_density += a4w[3], db_density +=
    a4b[3]), into non-zero outputs, ld9 = ld_dw9 = 155 (the real [128 | gamma(d)] width at L_dir = 4); columns >= 128 of dW9
    untouched.  K from tnerf_feature_finish_kernel: dW9 128 terms of G . Wf^T plus the outer product (K = 129, n = 131); dWf and
    dbf 64 terms (K = 64, n = 66); the density row one term (K = 1, n = 3)."""
    _finish(dev, "tnerf_feature_finish", _lib.lib().swnerf_tnerf_feature_finish, 64, 128, 155)


def test_feature_finish(dev):
    """swnerf_feature_finish held to the same per-entry gate at ld = 283.  K from feature_finish_kernel: dWv 256 terms of
    G . W_f^T plus the outer product (K = 257, n = 259); dW_f and db_f 128 terms (K = 128, n = 130); the alpha row one term (n = 3)."""
    _finish(dev, "feature_finish", _lib.lib().swnerf_feature_finish, 128, 256, 283)
