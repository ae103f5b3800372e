"""Yardsticks of tests/test_gpu_generic_units.py and tests/test_generic_units_host.py: the dispatch of generic_launch
(csrc/generic_kernels.hip) restated in plain Python, the table of cases with the kernel each one is meant to reach, the per-entry
gate, and operand builders whose padding is NaN.  Host only: nothing here touches the GPU.

The gate, from the number format alone (the argument of tests/test_gemm_tn_ordered.py).  An entry of the output is a sum of K fp32
products accumulated in fp32 (the MFMA adds them in some order; a zero-padded k adds an exact 0) plus the bias.  Every product is
rounded once and then passes through at most K - 1 additions of the sum and the bias add, every one of them a rounding of relative
size u = 2^-24: K + 1 summands in any order, the standard bound gamma_(K+1) (sum |a_k b_k| + |bias|) with
gamma_n = n u / (1 - n u), and gamma_(K+1) <= (K + 2) u as long as (K + 1)(K + 2) u <= 1, i.e. for every K up to 4000 (the table
stops at 319).  So, per entry,
    |got - ref64| <= (K + 2) u (|A| . |op(B)| + |bias|).
ReLU is 1-Lipschitz and exact on fp32, so the same gate holds against relu(ref64).  ELU is 1-Lipschitz too; csrc/elu.h evaluates
it within 1.2e-7 absolute of expm1 (pinned by tests/test_gpu_tnerf.py), which is added to the gate as it is.  No fudge factor.

Through the C ABI the weight of swnerf_linear / swnerf_linear_act is [N, K] with NO leading dimension of its own (ldb == K), so
the BT rows of the table carry ldb = K: only swnerf_gemm_nn can give B padding columns.  Both can give B an offset base."""
from collections import namedtuple

import wgrad_units_ref as WR

U = WR.U
ELU_ABS = 1.2e-7                 # csrc/elu.h: max abs error of sw_elu against expm1 on [-20, 0]
ACT_NONE, ACT_RELU, ACT_ELU = 0, 1, 2          # SWNERF_ACT_* (include/swnerf.h)

BRANCHES = ("generic_gemm_kernel<true>", "generic_gemm_kernel<false>",
            "generic_gemm128_kernel<true,false>", "generic_gemm128_kernel<true,true>",
            "generic_gemm128_kernel<false,false>", "generic_gemm128_kernel<false,true>")


def generic_branch(M, N, K, lda, ldb, bt, a_off, b_off):
    """The kernel generic_launch picks; a_off / b_off: the operands' bases in floats from a 16-byte-aligned buffer."""
    b = "true" if bt else "false"
    if N >= 64 and M >= 128:
        vec = lda % 4 == 0 and ldb % 4 == 0 and a_off % 4 == 0 and b_off % 4 == 0 and K % 4 == 0 and (bt or N % 4 == 0)
        return "generic_gemm128_kernel<%s,%s>" % (b, "true" if vec else "false")
    return "generic_gemm_kernel<%s>" % b


# ---- the case table -----------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "group branch bt M N K lda ldb ldc a_off b_off")


def case_id(c):
    return f"{c.group}-{'bt' if c.bt else 'nn'}-{c.M}x{c.N}x{c.K}-ld{c.lda}.{c.ldb}.{c.ldc}-off{c.a_off}.{c.b_off}"


def _brow(bt, N, K):
    """row length of B as stored: [N, K] for BT, [K, N] for NN"""
    return K if bt else N


def _unaligned(row):
    """a leading dimension above `row` that is no multiple of 4"""
    return row + 3 if (row + 3) % 4 else row + 2


def _case(group, branch, bt, M, N, K, lda, ldb_nn, ldc, a_off, b_off):
    return Case(group, branch, bt, M, N, K, lda, K if bt else ldb_nn, ldc, a_off, b_off)


# a. the 64 x 64 kernel: M in {1, 33, 64, 65, 127} and M >= 128 with N < 64; N in {1, 5, 63, 64, 65, 130}; K in {1, 2, 31, 32, 33,
#    63, 65} - every value at least once.  ld = row length + 3, every base one float off.
SHAPES_64 = [(1, 64, 33), (33, 1, 65), (64, 5, 32), (65, 65, 31), (127, 130, 63), (129, 63, 2), (257, 3, 1), (64, 64, 65),
             (127, 63, 1), (65, 130, 2), (33, 5, 33), (1, 1, 31)]
# b. the 128 x 128 kernel on 4-byte loads: M in {128, 129, 255, 257}, N in {64, 65, 127, 128, 129, 260}, K in {1, 3, 31, 33, 63,
#    319}; 257 x 260 is three row blocks by three column blocks.  Leading dimensions no multiple of 4, bases one float off.
SHAPES_128 = [(128, 64, 1), (129, 65, 3), (255, 127, 31), (257, 260, 33), (128, 128, 63), (129, 129, 319), (255, 64, 33), (257, 128, 3)]
# c. the 128 x 128 kernel on 16-byte loads: K in {4, 28, 32, 36, 64, 100} (one short chunk, a chunk less one load, one chunk, a
#    chunk plus one load, two chunks, K % 32 == 4); lda = K + 4, ldb = N + 8 where B has a leading dimension, aligned bases.
SHAPES_VEC_BT = [(128, 64, 4), (129, 65, 28), (255, 127, 32), (257, 260, 36), (128, 128, 64), (129, 129, 100)]
SHAPES_VEC_NN = [(128, 64, 4), (129, 68, 28), (255, 132, 32), (257, 256, 36), (128, 68, 64), (129, 132, 100)]


def _table():
    t = []
    for bt in (True, False):
        b = "true" if bt else "false"
        for M, N, K in SHAPES_64:
            t.append(_case("tile64", f"generic_gemm_kernel<{b}>", bt, M, N, K, K + 3, N + 3, N + 3, 1, 1))
        for M, N, K in SHAPES_128:
            t.append(_case("tile128", f"generic_gemm128_kernel<{b},false>", bt, M, N, K, _unaligned(K), _unaligned(N), _unaligned(N), 1, 1))
        for M, N, K in (SHAPES_VEC_BT if bt else SHAPES_VEC_NN):
            t.append(_case("vec", f"generic_gemm128_kernel<{b},true>", bt, M, N, K, K + 4, N + 8, N + 5, 0, 0))
    return t


CASES = _table()

# d. one disqualifier at a time, from the 16-byte case M = 129, N = 68, K = 36 (lda = 40; ldb = 76 for NN, K for BT)
VEC_BASE = {bt: _case("vec", "generic_gemm128_kernel<%s,true>" % ("true" if bt else "false"), bt, 129, 68, 36, 40, 76, 73, 0, 0)
            for bt in (True, False)}


def _disqualified():
    t = []
    for bt in (True, False):
        base = VEC_BASE[bt]
        fb = "generic_gemm128_kernel<%s,false>" % ("true" if bt else "false")
        brk = [("lda+1", dict(lda=base.lda + 1)), ("a_base+1", dict(a_off=1)), ("b_base+1", dict(b_off=1)),
               ("K=35", dict(K=35, ldb=35) if bt else dict(K=35))]            # (BT: the weight's rows are K long, so ldb follows K)
        if not bt:
            brk += [("ldb+1", dict(ldb=base.ldb + 1)), ("N=66", dict(N=66))]
        for name, kw in brk:
            t.append(base._replace(group="fallback:" + name, branch=fb, **kw))
    return t


DISQUALIFIED = _disqualified()
# e. the epilogue cases: one per kernel family (and the 16-byte variant of the second), BT by construction
EPILOGUE = [c for c in CASES if c.bt and (c.M, c.N, c.K) in ((65, 65, 31), (129, 65, 3), (129, 65, 28))]
ALL_CASES = CASES + list(VEC_BASE.values()) + DISQUALIFIED


# ---- operands: randn windows inside NaN ------------------------------------------------------------------------------------------
class Operands:
    """A [M, K] at float a_off of a flat buffer with lda floats per row; B [N, K] (BT) or [K, N] (NN) at b_off with ldb per row;
    bias [N].  Every float of the two buffers outside the logical operands is NaN: columns K..lda of A, columns past B's row
    length, the floats before an offset base.  to(dev) moves the BUFFERS (so the bases keep their offsets from an aligned
    allocation) and rebuilds the views."""

    def __init__(self, torch, c, abuf, bbuf, bias):
        self.torch, self.c, self.abuf, self.bbuf, self.bias = torch, c, abuf, bbuf, bias
        br, rows_b = _brow(c.bt, c.N, c.K), (c.N if c.bt else c.K)
        self.a = abuf[c.a_off:c.a_off + c.M * c.lda].view(c.M, c.lda)[:, :c.K]
        self.b = bbuf[c.b_off:c.b_off + rows_b * c.ldb].view(rows_b, c.ldb)[:, :br]

    def to(self, dev):
        return Operands(self.torch, self.c, self.abuf.to(dev), self.bbuf.to(dev), self.bias.to(dev))

    def reference(self, act=ACT_NONE, with_bias=True):
        """(ref64, mag): act(A . op(B) + bias) in float64 and |A| . |op(B)| + |bias| (the ELU's pinned absolute error folded into
        mag, so that (K + 2) u mag is the whole gate)"""
        torch, c = self.torch, self.c
        a64, b64 = self.a.double(), self.b.double()
        opb = b64.T if c.bt else b64
        ref, mag = a64 @ opb, a64.abs() @ opb.abs()
        if with_bias:
            ref, mag = ref + self.bias.double(), mag + self.bias.double().abs()
        if act == ACT_RELU:
            ref = ref.clamp_min(0)
        elif act == ACT_ELU:
            ref = torch.where(ref > 0, ref, torch.expm1(ref))
            mag = mag + ELU_ABS / ((c.K + 2) * U)
        return ref, mag


def operands(torch, c, a_scale=1.0, bias_mean=0.0, bias_std=1.0):
    """seeded by the case's numbers; on the CPU"""
    g = torch.Generator().manual_seed(1000003 * c.M + 1009 * c.N + 31 * c.K + 7 * c.lda + 3 * c.ldb + c.a_off + 2 * c.b_off + (5 if c.bt else 0))
    rows_b = c.N if c.bt else c.K
    abuf = torch.full((c.a_off + c.M * c.lda,), float("nan"))
    bbuf = torch.full((c.b_off + rows_b * c.ldb,), float("nan"))
    bias = torch.randn((c.N,), generator=g) * bias_std + bias_mean
    o = Operands(torch, c, abuf, bbuf, bias)
    o.a.copy_(torch.randn((c.M, c.K), generator=g) * a_scale)
    o.b.copy_(torch.randn(tuple(o.b.shape), generator=g))
    assert int(torch.isnan(abuf).sum()) == abuf.numel() - c.M * c.K and int(torch.isnan(bbuf).sum()) == bbuf.numel() - o.b.numel()
    return o


def elu_operands(torch, c):
    """pre-activations of about [-8, 3]: standard deviation 1.3 around a bias near -2.5"""
    return operands(torch, c, a_scale=1.3 / c.K ** 0.5, bias_mean=-2.5, bias_std=0.2)


def gate_ratio(got, ref, mag, K):
    """max |got - ref64| / ((K + 2) u mag): <= 1 passes"""
    return WR.ratio(got, ref, mag, K + 2)


# ---- the elementwise kernels (include/swnerf.h: relu_mask dy = y > 0 ? dy : 0;  elu_grad dy *= y > 0 ? 1 : y + 1) --------------
ELEMENTWISE_N = [1, 255, 256, 257, 65537]


def special_y(torch, n, gen):
    """y with, in turn, +0.0, -0.0, the smallest denormal, -1.0 (saturated ELU), NaN and three ordinary values of either sign"""
    y = torch.randn((n,), generator=gen)
    sp = torch.tensor([0.0, -0.0, 2.0 ** -149, -1.0, float("nan")])
    for j in range(5):
        y[j::8] = sp[j]
    return y
