"""Yardsticks of tests/test_gpu_wgrad_units.py (and of the slot-map table in tests/test_host_math.py): the embedding slot
maps of csrc/swnerf_common.h restated in plain Python, the per-entry gate of tests/test_gemm_tn_ordered.py, the branch list of
swnerf_gemm_tn restated from its shape / alignment / row-count tests, and guarded buffers (a window inside a buffer whose
every other float must stay bit for bit what it was)."""
import numpy as np

U = 2.0 ** -24
XS_LD = 96           # SW_XS_LD
ACT_LD = 2432        # SW_ACT_LD


# ---- csrc/swnerf_common.h: reference column of an operand slot (-1: zero pad) ----------------------------------------------
def pos_col(a, h, L):
    if a < 30:
        k, c = divmod(a, 3)
        return 3 + 6 * k + 3 * h + c if k < L else -1
    if a == 30:
        return 0 if h == 0 else 2
    return 1 if h == 0 else -1


def dir_col(a, h, L):
    if a < 12:
        k, c = divmod(a, 3)
        return 3 + 6 * k + 3 * h + c if k < L else -1
    if a == 12:
        return 0 if h == 0 else 2
    if a == 13:
        return 1 if h == 0 else -1
    return -1


def time_col(a, h, L):
    if a < 10:
        return 1 + 2 * a + h if a < L else -1
    if a == 10:
        return 0 if h == 0 else -1
    return -1


def xs_col(f, Lp, Ld):
    kt, g, h, e = f >> 5, (f >> 3) & 3, (f >> 2) & 1, f & 3
    r = 4 * g + e
    return pos_col(16 * kt + r, h, Lp) if kt < 2 else dir_col(r, h, Ld)


def time_slot_col(f, Lt):
    """slot f (0..31) of the gamma(t) k-tile, as unslot_time_kernel decodes it"""
    g, h, e = (f >> 3) & 3, (f >> 2) & 1, f & 3
    return time_col(4 * g + e, h, Lt)


def scatter(Cs, cols, W, col0):
    """W[o][col0 + cols[f]] = Cs[o][f] for every slot f with cols[f] >= 0 (numpy, in place); asserts that no column is hit twice"""
    real = [c for c in cols if c >= 0]
    assert len(set(real)) == len(real)
    for f, c in enumerate(cols):
        if c >= 0:
            W[:, col0 + c] = Cs[:, f]
    return sorted(real)


# ---- the gate (tests/test_gemm_tn_ordered.py): fp32 products summed in fp32 in any order, n additions per entry ------------
def ratio(got, ref, mag, n):
    """max over entries of |got - ref| / (n u mag): <= 1 passes.  got fp32, ref / mag float64 torch tensors of one shape."""
    gate = n * U * mag
    err = (got.double() - ref).abs()
    assert bool((gate > 0).all())
    return float((err / gate).max())


# ---- swnerf_gemm_tn's branch list (wgrad_kernels.hip), for operands whose BUFFERS are 16-byte aligned ----------------------
def gemm_tn_branch(No, Ni, M, lda, a_col, ldb, b_col):
    al_a, al_b = a_col % 4 == 0 and lda % 4 == 0, b_col % 4 == 0 and ldb % 4 == 0
    if al_a and al_b and M >= 4096:
        if No == 256 and Ni == 256:
            return "gemm_tn_dma_kernel<false>"
        if No % 4 == 0 and Ni % 4 == 0:
            if No <= 32 and Ni <= 128:
                return "gemm_tn_tiled_kernel<1,1,1,4>"
            if No <= 32 and Ni <= 256:
                return "gemm_tn_tiled_kernel<1,2,1,4>"
            if No <= 128 and Ni <= 32:
                return "gemm_tn_tiled_kernel<1,1,4,1>"
            if Ni <= 32:
                return "gemm_tn_tiled_kernel<1,1,8,1>"
            if Ni <= 64:
                return "gemm_tn_tiled_kernel<1,1,8,2>"
    va, vb = al_a and No % 4 == 0, al_b and Ni % 4 == 0
    return "gemm_tn_kernel<%s,%s>" % ("true" if va else "false", "true" if vb else "false")


def gemm_tn_grid_y(No, Ni):
    return ((Ni + 255) // 256) * (2 if No > 128 else 1)


# ---- guarded buffers ------------------------------------------------------------------------------------------------------------
class Guarded:
    """`shape` floats of standard-normal content inside a flat buffer with `pad` more on either side; after the kernel ran,
    untouched() tells whether everything outside the window is bit for bit what it was."""
    def __init__(self, torch, shape, gen, dev, pad=67):
        n = int(np.prod(shape))
        self.buf = torch.randn((n + 2 * pad,), generator=gen, device=dev)
        self.win = self.buf[pad:pad + n].view(*shape)
        self.before = self.buf.clone()
        self.c0 = self.before[pad:pad + n].view(*shape)
        self.pad, self.n, self.torch = pad, n, torch

    def untouched(self):
        p, n = self.pad, self.n
        return self.torch.equal(self.buf[:p], self.before[:p]) and self.torch.equal(self.buf[p + n:], self.before[p + n:])

    def unchanged(self):
        return self.torch.equal(self.buf, self.before)
