#!/usr/bin/env python3
"""Capture golden vectors G15 from the UNMODIFIED reference (build container only): multires_dnerf/pyramid.py on CPU -
generate_laplacian_pyramid_batch (4 levels) and reconstruct_image_from_pyramid_batch of seeded [0,1) images.  Stored per
case: the input, the reference's four levels, its reconstruction of them, the kernel, and per array `ref_dist`: the
reference's own max abs distance from the float64 restatement tests/pyramid_ref.py (the yardstick of the gates in
tests/test_gpu_pyramid.py).
Run: python tests/golden/make_golden_pyramid.py <path of the reference checkout>   (or SWNERF_REFERENCE=<path>)"""
import importlib.util
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pyramid_ref as R  # noqa: E402

# name: (seed, shape, kernel_size, sigma); 4 levels each
CASES = {
    "a": (1501, (2, 16, 16, 3), 3, 1.0),
    "b": (1502, (2, 17, 31, 3), 3, 1.0),
    "c": (1503, (1, 37, 53, 3), 3, 1.0),
    "d": (1504, (1, 37, 53, 3), 5, 1.5),
}
LEVELS = 4


def case_input(name):
    seed, shape, _, _ = CASES[name]
    return np.random.Generator(np.random.PCG64(seed)).random(shape, dtype=np.float32)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SWNERF_REFERENCE")
    if not ref:
        raise SystemExit(__doc__)
    import torch
    # pyramid.py imports dataloader.load_blender, which needs packages that are not installed; it uses nothing of it
    for name in ("dataloader", "dataloader.load_blender"):
        sys.modules.setdefault(name, types.ModuleType(name))
    try:
        import PIL.Image  # noqa: F401
    except Exception:
        sys.modules["PIL"] = types.ModuleType("PIL")
        sys.modules["PIL.Image"] = types.ModuleType("PIL.Image")
        sys.modules["PIL"].Image = sys.modules["PIL.Image"]
    spec = importlib.util.spec_from_file_location("ref_pyramid", os.path.join(ref, "multires_dnerf", "pyramid.py"))
    P = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(P)
    out = {}
    for name, (seed, shape, k, sigma) in CASES.items():
        x = case_input(name)
        with torch.no_grad():
            pyr = P.generate_laplacian_pyramid_batch(torch.from_numpy(x), levels=LEVELS, kernel_size=k, sigma=sigma)
            rec = P.reconstruct_image_from_pyramid_batch(pyr)
            kern = P.create_gaussian_kernel(k, sigma)
        pyr = [p.contiguous().numpy() for p in pyr]
        rec = rec.contiguous().numpy()
        want = R.generate(x, LEVELS, k, sigma)
        out[f"{name}_input"] = x
        out[f"{name}_kernel"] = kern.numpy()
        dist = []
        for l in range(LEVELS):
            out[f"{name}_level{l}"] = pyr[l]
            dist.append(np.abs(pyr[l].astype(np.float64) - want[l]).max())
        out[f"{name}_recon"] = rec
        # the reference's reconstruction of ITS levels against the exact reconstruction of the same levels
        dist.append(np.abs(rec.astype(np.float64) - R.reconstruct(pyr)).max())
        out[f"{name}_ref_dist"] = np.asarray(dist, np.float64)            # level0..3, recon
        out[f"{name}_roundtrip_dist"] = np.float64(np.abs(rec.astype(np.float64) - x).max())
        print(name, shape, k, sigma, [p.shape for p in pyr], "ref_dist", dist, "roundtrip", out[f"{name}_roundtrip_dist"])
    path = os.path.join(HERE, "g15_pyramid.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
