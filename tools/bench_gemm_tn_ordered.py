#!/usr/bin/env python3
"""swnerf_gemm_tn_ordered (the reproducible weight gradient of the generic path) against swnerf_gemm_tn (float
atomics) at the joint step's level-0 shape and at width 256: median and minimum of 10 device-event timings after 3 warm-up calls.
  python tools/bench_gemm_tn_ordered.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sw-nerf_amd"))

import torch  # noqa: E402
from swnerf import _lib  # noqa: E402

SHAPES = [(16384, 64, 187), (131072, 256, 256), (1 << 20, 256, 256), (1 << 20, 256, 319)]        # rows, No, Ni


def main():
    L = _lib.lib()
    dev = torch.device("cuda:0")
    for M, No, Ni in SHAPES:
        A, B = torch.randn((M, No), device=dev), torch.randn((M, Ni), device=dev)
        C, b = torch.zeros((No, Ni), device=dev), torch.zeros((No,), device=dev)
        nws = L.swnerf_gemm_tn_ordered_ws_floats(M, No, Ni)
        ws = torch.empty((nws,), device=dev)
        ordered = lambda: _lib.check(L.swnerf_gemm_tn_ordered(_lib.ptr(A), No, No, _lib.ptr(B), Ni, Ni, M, _lib.ptr(C), Ni, _lib.ptr(b),
                                                              _lib.ptr(ws), nws, None), "gemm_tn_ordered")
        atomic = lambda: _lib.check(L.swnerf_gemm_tn(_lib.ptr(A), No, No, _lib.ptr(B), Ni, Ni, M, _lib.ptr(C), Ni, _lib.ptr(b), None), "gemm_tn")
        for name, f in (("ordered", ordered), ("atomic", atomic)):
            for _ in range(3):
                f()
            torch.cuda.synchronize()
            ts = []
            for _ in range(10):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            ts.sort()
            print(f"M={M} No={No} Ni={Ni} {name}: median {ts[5] * 1e3:.0f} us  min {ts[0] * 1e3:.0f} us  "
                  f"({2 * M * No * Ni / ts[5] / 1e9:.1f} TFLOP/s)", flush=True)


if __name__ == "__main__":
    main()
