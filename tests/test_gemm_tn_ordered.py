"""swnerf_gemm_tn_ordered (csrc/generic_kernels.hip): the generic path's weight gradient with its row slices added in a
fixed order - what the MultiRes level nets take (`reproducible_wgrad`), so that a backward pass repeats bit for bit.

Bound against float64: fp32 products accumulated in fp32 in ANY order stay within (n - 1) u sum_m |a_m b_m| to first
order, u = 2^-24; with the slices' sums (at most 256 slices here, at most 512 on the atomic path) and the add into C there
are at most M + 513 additions per entry on either path, so the gate is (M + 514) u (|A|^T |B|) per entry (and
(M + 514) u sum |A| for the bias) - from the number format alone."""
import ctypes

import numpy as np
import pytest
import torch

from swnerf import _lib, generic

U = 2.0 ** -24
# rows, No, Ni: one slice with an odd row count; tiles that are no multiple of 32 and several slices of odd length (4097 / 9 ->
# 456 rows each, the last one shorter); the joint step's level 0 (16384 rows, width 64, gamma(x) of 20 bands + skip)
SHAPES = [(5, 4, 3), (333, 70, 123), (4097, 33, 65), (16384, 64, 187)]


def test_workspace_sizes_and_argument_errors_without_gpu():
    L = _lib.lib()
    ws = L.swnerf_gemm_tn_ordered_ws_floats
    assert ws(0, 4, 4) == 0 and ws(-1, 4, 4) == 0 and ws(8, 0, 4) == 0 and ws(8, 4, 65537) == 0
    assert ws(5, 4, 3) == 4 * 4 and ws(512, 4, 3) == 16 and ws(513, 4, 3) == 2 * 16 and ws(4097, 33, 65) == 9 * 33 * 66
    assert ws(1 << 22, 64, 187) == 256 * 64 * 188                       # at most 256 slices ...
    assert ws(1 << 22, 256, 255) == 64 * 256 * 256                      # ... and at most 16 MiB of them,
    assert ws(1 << 22, 4096, 4095) == 4096 * 4096                       # unless one partial product alone is larger
    f = L.swnerf_gemm_tn_ordered
    assert f(None, 4, 4, None, 4, 4, 0, None, 4, None, None, 0, None) == 0         # M == 0: nothing to do
    assert f(None, 4, 4, None, 4, 4, 8, None, 4, None, None, 0, None) == -1 and b"gemm_tn_ordered" in L.swnerf_last_error()
    one = ctypes.c_void_p(8)                                            # (never dereferenced: rejected first)
    assert f(one, 3, 4, one, 4, 4, 8, one, 4, None, one, 64, None) == -1           # lda < No
    assert f(one, 4, 4, one, 4, 4, 8, one, 4, None, one, 19, None) == -1 and b"workspace" in L.swnerf_last_error()
    assert f(one, 70000, 70000, one, 4, 4, 8, one, 4, None, one, 1 << 30, None) == -2


@pytest.mark.gpu
@pytest.mark.parametrize("M,No,Ni", SHAPES)
def test_ordered_weight_gradient(M, No, Ni):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(M + No)
    wide = torch.randn((M, Ni + 5), generator=g).to(dev)
    x = wide[:, 2:2 + Ni]                                               # a strided operand, as the skip concatenation's slices are
    dy = torch.randn((M, No), generator=g).to(dev)
    lin = torch.nn.Linear(Ni, No).to(dev)

    def grads(ordered):
        lin.zero_grad()
        xi = x.detach().requires_grad_(True)
        y = generic.linear(xi, lin, ordered=ordered)
        y.backward(dy)
        return lin.weight.grad.clone(), lin.bias.grad.clone(), xi.grad.clone()

    dw, db, dx = grads(True)
    dw2, db2, dx2 = grads(True)
    assert torch.equal(dw, dw2) and torch.equal(db, db2) and torch.equal(dx, dx2)
    a64, b64 = dy.double().cpu(), x.double().cpu()
    n = (M + 514) * U
    ew = float(((dw.double().cpu() - a64.T @ b64).abs() - n * (a64.abs().T @ b64.abs())).max())
    eb = float(((db.double().cpu() - a64.sum(0)).abs() - n * a64.abs().sum(0)).max())
    print(f"M={M} No={No} Ni={Ni}: |dW - dW64| {float((dw.double().cpu() - a64.T @ b64).abs().max()):.3e}, "
          f"|db - db64| {float((db.double().cpu() - a64.sum(0)).abs().max()):.3e}; over the gate by {ew:.3e}, {eb:.3e} (<= 0 passes)")
    assert ew <= 0 and eb <= 0
    # the atomic path computes the same sums: within twice the gate of each other
    dwa, dba, dxa = grads(False)
    assert torch.equal(dx, dxa)
    assert float(((dw - dwa).double().cpu().abs() - 2 * n * (a64.abs().T @ b64.abs())).max()) <= 0


@pytest.mark.gpu
def test_accumulates_into_c_and_bias():
    dev = torch.device("cuda:0")
    L = _lib.lib()
    M, No, Ni = 37, 5, 9
    g = torch.Generator().manual_seed(3)
    A, B = torch.randn((M, No), generator=g).to(dev), torch.randn((M, Ni), generator=g).to(dev)
    C, bias = torch.full((No, Ni + 2), 2.0, device=dev), torch.full((No,), -1.0, device=dev)
    nws = L.swnerf_gemm_tn_ordered_ws_floats(M, No, Ni)
    ws = torch.empty((nws,), device=dev)
    _lib.check(L.swnerf_gemm_tn_ordered(_lib.ptr(A), No, No, _lib.ptr(B), Ni, Ni, M, _lib.ptr(C), Ni + 2, _lib.ptr(bias),
                                        _lib.ptr(ws), nws, None), "gemm_tn_ordered")
    torch.cuda.synchronize()
    assert torch.equal(C[:, Ni:], torch.full((No, 2), 2.0, device=dev))                    # columns past Ni stay untouched
    n = (M + 514) * U                                                   # the gate of the module docstring, |C| = 2 added in
    assert float(((C[:, :Ni].double() - 2.0 - A.double().T @ B.double()).abs() - n * (A.double().abs().T @ B.double().abs() + 2.0)).max()) <= 0
    assert float(((bias.double() + 1.0 - A.double().sum(0)).abs() - n * (A.double().abs().sum(0) + 1.0)).max()) <= 0
