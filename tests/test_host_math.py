"""Host-compiled (g++) checks of csrc/swnerf_common.h: the sin/cos used by every kernel, the
linspace restatement, and that the embedding slot maps cover each reference column exactly once."""
import os
import subprocess

import numpy as np
import torch

import wgrad_units_ref as WR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SRC = r'''
#include "swnerf_common.h"
#include <stdio.h>
#include <stdlib.h>
int main() {
  double worst = 0; srand(3);
  for (int it = 0; it < 3000000; ++it) {
    float x = ((float)rand() / RAND_MAX * 2 - 1) * 6.0f; int k = rand() % 10; float y = x * (float)(1 << k);
    for (int c = 0; c < 2; ++c) { double e = fabs((double)sw_sin_or_cos(y, c) - (c ? cos((double)y) : sin((double)y))); if (e > worst) worst = e; }
  }
  printf("%.6e\n", worst);
  int sizes[] = {64, 128, 192, 100, 33, 2};
  for (int s = 0; s < 6; ++s) { for (int i = 0; i < sizes[s]; ++i) printf("%.9g ", sw_linspace(0.f, 1.f, sizes[s], i)); printf("\n"); }
  for (int L = 0; L <= 10; ++L) { for (int a = 0; a < 32; ++a) for (int h = 0; h < 2; ++h) printf("%d ", sw_pos_col(a, h, L)); printf("\n"); }
  for (int L = 0; L <= 4; ++L) { for (int a = 0; a < 16; ++a) for (int h = 0; h < 2; ++h) printf("%d ", sw_dir_col(a, h, L)); printf("\n"); }
  for (int L = 0; L <= 10; ++L) { for (int a = 0; a < 16; ++a) for (int h = 0; h < 2; ++h) printf("%d ", sw_time_col(a, h, L)); printf("\n"); }
  for (int h = 0; h < 2; ++h) { for (int r = 0; r < 16; ++r) printf("%d ", sw_frow(r, h)); printf("\n"); }
  printf("%d %d %d %d\n", SW_CANON_STEPS, SW_DEFORM_STEPS, SW_CANON_FLOATS, SW_DNERF_FLOATS);
  for (int f = 0; f < SW_XS_LD; ++f) printf("%d ", sw_xs_col(f, 10, 4)); printf("\n");
  for (int f = 0; f < SW_XS_LD; ++f) printf("%d ", sw_xs_col(f, 6, 2)); printf("\n");
  printf("%d %d %d\n", SW_BWD_IG_STEPS, SW_BWD_DN_STEPS, SW_XS_LD);
  // every band swnerf_embed accepts, through the function embed_kernel calls (sw_embed_sincos), and that function's two halves
  // against each other: the bands below SW_SINCOS_F32_BANDS are sw_sincos_pair = sw_sin_or_cos bit for bit
  int same = 1;
  for (int k = 0; k < 24; ++k) {
    double w = 0;
    for (int it = 0; it < 400002; ++it) {
      float x = it < 400000 ? ((float)rand() / RAND_MAX * 2 - 1) * 6.0f : (it & 1 ? 6.0f : -6.0f);
      float y = x * (float)(1 << k), s, c;
      sw_embed_sincos(x, k, &s, &c);
      double es = fabs((double)s - sin((double)y)), ec = fabs((double)c - cos((double)y));
      if (es > w) w = es;
      if (ec > w) w = ec;
      if (k < SW_SINCOS_F32_BANDS && (s != sw_sin_or_cos(y, 0) || c != sw_sin_or_cos(y, 1))) same = 0;
    }
    printf("%.6e ", w);
  }
  printf("\n%d %d\n", same, SW_SINCOS_F32_BANDS);
  // the slot -> column table of the fused training pass's encodings for every band pair the kernels accept
  for (int Lp = 0; Lp <= 10; ++Lp) for (int Ld = 0; Ld <= 4; ++Ld) { for (int f = 0; f < SW_XS_LD; ++f) printf("%d ", sw_xs_col(f, Lp, Ld)); printf("\n"); }
  return 0;
}
'''


def test_common_header_on_host(tmp_path):
    (tmp_path / "t.cpp").write_text(SRC)
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-mfma", "-I", os.path.join(ROOT, "sw-nerf_amd", "csrc"),
                    str(tmp_path / "t.cpp"), "-o", str(tmp_path / "t"), "-lm"], check=True)
    lines = subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert float(lines[0]) < 1.2e-7                                   # max |err| of sin/cos vs double libm, |y| <= 3072
    for ln, n in zip(lines[1:7], (64, 128, 192, 100, 33, 2)):         # == torch.linspace on CPU, bit for bit
        assert np.array_equal(np.array(ln.split(), np.float32), torch.linspace(0., 1., n).numpy())
    k = 7
    for L in range(11):                                               # every column of gamma(x), once
        cols = [int(c) for c in lines[k + L].split() if int(c) >= 0]
        assert sorted(cols) == list(range(3 * (1 + 2 * L)))
    k += 11
    for L in range(5):
        cols = [int(c) for c in lines[k + L].split() if int(c) >= 0]
        assert sorted(cols) == list(range(3 * (1 + 2 * L)))
    k += 5
    for L in range(11):
        cols = [int(c) for c in lines[k + L].split() if int(c) >= 0]
        assert sorted(cols) == list(range(1 + 2 * L))
    k += 11
    rows = [int(c) for c in (lines[k] + " " + lines[k + 1]).split()]
    assert sorted(rows) == list(range(32))                            # the MFMA C/D map is a bijection onto the tile rows
    canon, deform, cf, df = (int(x) for x in lines[k + 2].split())
    # 4 MFMAs per step, 2048 MACs per MFMA on a 32-row tile; the 1-/3-output heads (256+384 resp. 768 MACs per row)
    # run on the VALU, everything else (but the folded feature_linear) is in the stream with <= 1 % padding
    # feature_linear (65536 MACs per row, no activation behind it) is folded into the view layer at pack time: not executed
    assert 0 <= canon * 4 * 2048 - (593408 - 65536 - 256 - 384) * 32 <= 0.01 * 593408 * 32
    assert 0 <= deform * 4 * 2048 - (497152 - 768) * 32 <= 0.01 * 497152 * 32
    assert canon % 8 == 0 and deform % 8 == 0
    # the fused training pass's slot-ordered encodings (xs): slots 0..63 cover gamma(x), 64..95 gamma(d), each reference
    # column exactly once (what swnerf_unslot_grad relies on); the fused D-NeRF backward stream = IG stream + 7 trunk layers
    for ln, (Lp, Ld) in zip(lines[k + 3:k + 5], ((10, 4), (6, 2))):
        cols = [int(c) for c in ln.split()]
        assert len(cols) == 96
        assert sorted(c for c in cols[:64] if c >= 0) == list(range(3 * (1 + 2 * Lp)))
        assert sorted(c for c in cols[64:] if c >= 0) == list(range(3 * (1 + 2 * Ld)))
    ig, dn, xld = (int(x) for x in lines[k + 5].split())
    assert dn == ig + 7 * 256 and dn % 16 == 0 and xld == 96
    # the standalone embedder's sin/cos, per band k = 0 .. 23 (swnerf_embed accepts L <= 24), |x| <= 6, |y| <= 5.1e7: the same
    # bound as the fused kernels' range above; the float reduction alone gives 6e-7 in band 19 and 0.2 in band 23
    band = [float(v) for v in lines[k + 6].split()]
    assert len(band) == 24
    for kb, e in enumerate(band):
        assert e < 1.2e-7, f"band {kb}: max |err| {e:.3e} (all bands: {band})"
    same, nf32 = (int(x) for x in lines[k + 7].split())
    assert same == 1 and nf32 == 10                                   # L_pos, L_time <= 10 in the fused kernels: their bits
    # the plain-Python restatement of the slot maps (wgrad_units_ref: the yardstick of the unslot kernels' GPU tests) is the header's,
    # entry for entry: sw_pos_col / sw_dir_col / sw_time_col for every L, and sw_xs_col for every (L_pos, L_dir) in 0..10 x 0..4
    ints = lambda ln: [int(c) for c in ln.split()]
    for L in range(11):
        assert ints(lines[7 + L]) == [WR.pos_col(a, h, L) for a in range(32) for h in range(2)], L
        assert ints(lines[23 + L]) == [WR.time_col(a, h, L) for a in range(16) for h in range(2)], L
    for L in range(5):
        assert ints(lines[18 + L]) == [WR.dir_col(a, h, L) for a in range(16) for h in range(2)], L
    table = lines[k + 8:]
    assert len(table) == 55
    for ln, (Lp, Ld) in zip(table, ((Lp, Ld) for Lp in range(11) for Ld in range(5))):
        cols = ints(ln)
        assert cols == [WR.xs_col(f, Lp, Ld) for f in range(WR.XS_LD)], (Lp, Ld)
        assert sorted(c for c in cols[:64] if c >= 0) == list(range(3 * (1 + 2 * Lp)))
        assert sorted(c for c in cols[64:] if c >= 0) == list(range(3 * (1 + 2 * Ld)))
    # the gamma(t) k-tile shares the slot decoding (g, h, e) of sw_xs_col: unslot_time_kernel's map, every L_time
    for Lt in range(11):
        cols = [WR.time_slot_col(f, Lt) for f in range(32)]
        assert sorted(c for c in cols if c >= 0) == list(range(1 + 2 * Lt))


def test_embed_kernel_multiply_shift_divisions_are_exact():
    """csrc/misc_kernels.hip embed_kernel maps job j of a workgroup to (row, slot) with (j * ceil(2^24 / Q)) >> 24 in 32-bit
    arithmetic, and slot p to (band, component) with (p * ceil(2^24 / d)) >> 24: exact - and free of 32-bit overflow - for every
    (d <= 16, L <= 24) swnerf_embed accepts, at the rows-per-workgroup its launch picks (EMB_ROWS = 64, halved while the image exceeds 64 KB)."""
    for d in range(1, 17):
        d_magic = ((1 << 24) + d - 1) // d
        for L in range(0, 25):
            C, Q = d * (1 + 2 * L), d * (1 + L)
            R = 64
            while R > 1 and R * C * 4 > 64 * 1024:
                R >>= 1
            q_magic = ((1 << 24) + Q - 1) // Q
            j = np.arange(R * Q, dtype=np.uint64)
            assert int(j[-1]) * q_magic < 2 ** 32, (d, L, R)
            assert np.array_equal((j * np.uint64(q_magic)) >> np.uint64(24), j // np.uint64(Q)), (d, L, R)
            pslot = np.arange(max(d * L, 1), dtype=np.uint64)
            assert int(pslot[-1]) * d_magic < 2 ** 32
            assert np.array_equal((pslot * np.uint64(d_magic)) >> np.uint64(24), pslot // np.uint64(d)), (d, L)


def test_compositing_arithmetic_is_defined_once():
    """raw2outputs' arithmetic (ray.py:155-198) lives in csrc/composite.h alone: the literals that mark it - the 1e10 last
    interval and the 1e-10 of the survival factor, the disparity clamp and the backward's branch - appear in no other file of
    csrc/, so a kernel cannot grow a written-out copy of its own again."""
    csrc = os.path.join(ROOT, "sw-nerf_amd", "csrc")
    found = {lit: sorted(f for f in os.listdir(csrc) if lit in open(os.path.join(csrc, f), errors="replace").read())
             for lit in ("1e10f", "1e-10f")}
    assert found == {"1e10f": ["composite.h"], "1e-10f": ["composite.h"]}, found
