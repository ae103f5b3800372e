"""The yardsticks of tests/test_gpu_generic_units.py, checked on the CPU before any GPU time is spent: the case table reaches
every one of generic_launch's six kernels and names the one each case reaches, and torch's own CPU fp32 result of every case
(F.linear [+ relu / elu], a @ b) lies inside the gate against float64 - so the gate and the operand builders are sound and the
reference alone never uses the gate up."""
import os
import sys
from collections import Counter

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import generic_units_ref as GR    # noqa: E402


def test_table_reaches_every_branch():
    """All six kernels appear in the table, and each case's named kernel is what the restated dispatch gives for its numbers."""
    count = Counter()
    for c in GR.ALL_CASES:
        assert GR.generic_branch(c.M, c.N, c.K, c.lda, c.ldb, c.bt, c.a_off, c.b_off) == c.branch, GR.case_id(c)
        assert c.lda >= c.K and c.ldc >= c.N and c.ldb >= (c.K if c.bt else c.N), GR.case_id(c)
        count[c.branch] += 1
    print("\n[generic units] cases per kernel:")
    for b in GR.BRANCHES:
        print(f"  {b:38s} {count[b]}")
    assert set(count) == set(GR.BRANCHES) and all(count[b] >= 6 for b in GR.BRANCHES)
    assert len({GR.case_id(c) for c in GR.ALL_CASES}) == len(GR.ALL_CASES)


def test_table_hits_every_listed_value():
    """The value lists the three shape tables promise."""
    vals = lambda shapes, i: {s[i] for s in shapes}
    assert vals(GR.SHAPES_64, 0) >= {1, 33, 64, 65, 127} and (129, 63) in {s[:2] for s in GR.SHAPES_64} and (257, 3) in {s[:2] for s in GR.SHAPES_64}
    assert vals(GR.SHAPES_64, 1) >= {1, 5, 63, 64, 65, 130} and vals(GR.SHAPES_64, 2) == {1, 2, 31, 32, 33, 63, 65}
    assert (vals(GR.SHAPES_128, 0), vals(GR.SHAPES_128, 1), vals(GR.SHAPES_128, 2)) == ({128, 129, 255, 257}, {64, 65, 127, 128, 129, 260}, {1, 3, 31, 33, 63, 319})
    assert (257, 260) in {s[:2] for s in GR.SHAPES_128}
    assert vals(GR.SHAPES_VEC_BT, 2) == vals(GR.SHAPES_VEC_NN, 2) == {4, 28, 32, 36, 64, 100}
    assert vals(GR.SHAPES_VEC_BT, 1) == {64, 65, 127, 128, 129, 260} and vals(GR.SHAPES_VEC_NN, 1) == {64, 68, 132, 256}
    for c in GR.CASES:
        if c.group == "tile128":
            assert c.lda % 4 and c.ldc % 4 and (c.bt or c.ldb % 4) and c.a_off == c.b_off == 1
        if c.group == "vec":
            assert c.lda == c.K + 4 and (c.bt or c.ldb == c.N + 8)
    assert len(GR.DISQUALIFIED) == 4 + 6 and len(GR.EPILOGUE) == 3


def test_dispatch_thresholds():
    """The two thresholds and each alignment condition of the restated dispatch on its own."""
    B = GR.generic_branch
    assert B(127, 64, 32, 32, 32, True, 0, 0) == "generic_gemm_kernel<true>" and B(128, 63, 32, 32, 32, True, 0, 0) == "generic_gemm_kernel<true>"
    assert B(128, 64, 32, 32, 32, True, 0, 0) == "generic_gemm128_kernel<true,true>"
    assert B(128, 66, 32, 32, 68, True, 0, 0) == "generic_gemm128_kernel<true,true>"       # N % 4 matters to NN alone
    assert B(128, 66, 32, 32, 68, False, 0, 0) == "generic_gemm128_kernel<false,false>"
    assert B(128, 68, 32, 32, 68, False, 0, 0) == "generic_gemm128_kernel<false,true>"
    assert B(128, 68, 32, 32, 68, False, 4, 8) == "generic_gemm128_kernel<false,true>"
    for kw in (dict(lda=33), dict(ldb=69), dict(a_off=2), dict(b_off=3), dict(K=30)):
        a = dict(M=128, N=68, K=32, lda=32, ldb=68, bt=False, a_off=0, b_off=0)
        a.update(kw)
        assert B(**a) == "generic_gemm128_kernel<false,false>", kw


@pytest.mark.parametrize("c", GR.ALL_CASES, ids=GR.case_id)
def test_cpu_fp32_inside_the_gate(c):
    """torch's CPU fp32 result of the case against float64, through the same reference and gate the GPU test uses; for the BT
    cases with and without bias and under each epilogue (the ELU on its own operand range)."""
    o = GR.operands(torch, c)
    if not c.bt:
        ref, mag = o.reference(with_bias=False)
        r = GR.gate_ratio(o.a @ o.b, ref, mag, c.K)
        print(f"{GR.case_id(c)}: a @ b {r:.3e}")
        assert r <= 1.0
        return
    for act, name in ((GR.ACT_NONE, "none"), (GR.ACT_RELU, "relu"), (GR.ACT_ELU, "elu")):
        oo = GR.elu_operands(torch, c) if act == GR.ACT_ELU else o
        for with_bias in (True, False):
            y = F.linear(oo.a, oo.b, oo.bias if with_bias else None)
            y = F.relu(y) if act == GR.ACT_RELU else F.elu(y) if act == GR.ACT_ELU else y
            ref, mag = oo.reference(act, with_bias)
            r = GR.gate_ratio(y, ref, mag, c.K)
            print(f"{GR.case_id(c)} {name} bias={with_bias}: {r:.3e}")
            assert r <= 1.0


def test_elu_operands_span():
    """The ELU cases' pre-activations cover the saturated tail and the linear side: about [-8, 3]."""
    for c in GR.EPILOGUE:
        o = GR.elu_operands(torch, c)
        pre = o.a.double() @ o.b.double().T + o.bias.double()
        assert float(pre.min()) < -6.0 and float(pre.max()) > 1.5 and float(pre.min()) > -14.0 and float(pre.max()) < 7.0, (float(pre.min()), float(pre.max()))


def test_special_y_holds_every_special_value():
    g = torch.Generator().manual_seed(1)
    y = GR.special_y(torch, 257, g)
    bits = y.view(torch.int32)
    assert int(bits[0]) == 0 and int(bits[1]) == -2 ** 31 and int(bits[2]) == 1 and float(y[3]) == -1.0 and bool(torch.isnan(y[4]))
    assert bool((y[5::8] > 0).any()) and bool((y[5::8] < 0).any()) and int(torch.isnan(y).sum()) == len(y[4::8])
    assert GR.special_y(torch, 1, g).view(torch.int32).tolist() == [0]
