"""Yardsticks of the bf16x3 weight-gradient GEMM (csrc/wgrad_x3_kernels.hip; tests/test_gpu_wgrad_x3.py, tests/test_wgrad_x3_host.py):
the operand split, the three-term product and the two "one cross term missing" products in float64, the gate and the seeded operands.

Split: hi = bf16(v), lo = bf16(v - hi), both round to nearest even; bf16 keeps 8 significand bits, so |v - hi| <= 2^-8 |v| and
|v - hi - lo| <= 2^-16 |v|.  Of  a b = (a_hi + a_lo + ra)(b_hi + b_lo + rb)  the kernel keeps a_hi b_hi + a_hi b_lo + a_lo b_hi; the dropped
a_lo b_lo and the two residual terms are each <= 2^-16 |a| |b| (to first order), four such terms at most: 2^-14 |a| |b|.  With u = 2^-24 and
n = 3 M + 514 (three fp32 accumulations per row, at most 512 slices, the add into C), per entry
    |got - ref64| <= (2^-14 + n u) (|A|^T |B|) + n u |C0|.
The gate is loose - a kernel that dropped a cross term passes it on random data (such an error is ~2^-9 per product and sums like a random
walk) - so there is a discriminating condition next to it: max |got - ref64| <= 1/16 of the smaller of the two max errors that the float64
products with ONE cross term missing make.  On randn operands the three-term product sits 325-350 x below those."""
import functools

import torch

U = 2.0 ** -24
LD = 2432                 # SW_ACT_LD: the leading dimension of the `grad` / `act` buffers the GEMM's operands are windows of
A_COL, B_COL = 512, 1024  # where the seeded operand columns sit in their [M, LD] buffers (16-byte aligned)
NWIN = 2                  # 256-column windows of seeded content per buffer
# (M, half the entries zeroed as ReLU-masked rows are): what the GPU tests run and the host test emulates
CASES = [(4096, False), (4096, True), (4100, False), (24581, False), (24581, True)]


def split(v):
    """fp32 tensor -> (hi, lo) as fp32 tensors holding bf16 values (torch's bfloat16 conversion rounds to nearest even)"""
    v = v.float()
    hi = v.bfloat16().float()
    return hi, (v - hi).bfloat16().float()           # (v - hi is exact in fp32: hi is v's leading bits, rounded)


def products(A, B):
    """A [M, No], B [M, Ni] fp32 -> float64 [No, Ni]: the exact A^T B, the three-term bf16x3 product, and the two products with one
    cross term missing (A_lo B_hi dropped; A_hi B_lo dropped)."""
    (ah, al), (bh, bl) = (tuple(x.double() for x in split(T_)) for T_ in (A, B))
    hh, hl, lh = ah.T @ bh, ah.T @ bl, al.T @ bh
    return A.double().T @ B.double(), hh + hl + lh, hh + hl, hh + lh


def reference(A, B):
    """What check() needs of one operand pair, computed once: (exact A^T B, |A|^T |B|, the smaller of the two max errors that a product
    with one cross term missing makes), float64."""
    ref, _, no_lh, no_hl = products(A, B)
    return ref, A.double().abs().T @ B.double().abs(), min(float((no_lh - ref).abs().max()), float((no_hl - ref).abs().max()))


def bound(mag, C0, M):
    """the per-entry gate, float64 [No, Ni]; mag = |A|^T |B|"""
    n = 3 * M + 514
    return (2.0 ** -14 + n * U) * mag + n * U * C0.double().abs()


@functools.lru_cache(maxsize=None)
def operands(M, zeros, seed=0):
    """The seeded operand columns of a case, on the CPU: A, B [M, 256 NWIN] fp32 (the GPU tests copy them into their device buffers)."""
    g = torch.Generator().manual_seed(7919 * M + 2 * seed + int(zeros))
    A, B = (torch.randn((M, 256 * NWIN), generator=g) for _ in range(2))
    if zeros:
        A, B = (T_ * (torch.rand((M, 256 * NWIN), generator=g) < 0.5) for T_ in (A, B))
    return A, B


def check(what, got, M, reference_, C0):
    """got [256, 256] (fp32 or float64) = C0 + the product under test of the M-row operands that reference_ = reference(A, B) was made of.
    Prints, then asserts the gate and the 1/16 condition; returns (worst |got - ref64| / gate, max |got - ref64| / the dropped-term error)."""
    ref, mag, dropped = reference_
    err = (got.double() - (C0.double() + ref)).abs()
    gate = bound(mag, C0, M)
    assert bool((gate > 0).all())
    r_gate = float((err / gate).max())
    r_drop = float(err.max()) / dropped
    print(f"{what}: max |got - ref64| = {float(err.max()):.3e}, {r_gate:.3e} of the gate; a dropped cross term makes {dropped:.3e} "
          f"({1 / max(r_drop, 1e-300):.0f} x)")
    assert r_gate <= 1.0, f"{what}: {r_gate:.3e} of the gate"
    assert r_drop <= 1.0 / 16, f"{what}: max error {float(err.max()):.3e} is more than 1/16 of a dropped cross term's {dropped:.3e}"
    return r_gate, r_drop
