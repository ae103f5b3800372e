#!/usr/bin/env python3
"""Capture g17_dynamic_query.npz from the UNMODIFIED reference (build container only): the grid query of the two time-conditioned
nets at one frame time - DirectTemporalNeRF through d_nerf/run_dnerf.py:run_network and TNeRF through
t_nerf/run_tnerf.py:run_network - on the G10 grid (cases.G10_BOUNDS, 6^3 points) with 8 generate_viewdirs directions
(nerf/extract_mesh.py:7-24) at t = 0 and t = 0.5.  Seeded weights (cases.weights_dnerf, cases_tnerf.weights); only OUTPUTS and a
checksum of the inputs are stored: per direction the raw [V,M,4], its mean over the directions, sigma and (D-NeRF) dx.
T-NeRF is recorded twice: `tnerf_*_raw` is the reference's TNeRF with its parameters in float64 on the runner's float32 encodings
(what tests/tnerf_ref.forward restates: encodings in float32, everything after in float64), `tnerf_*_raw_f32` the same module in
the runner's own float32 - 8 layers of float32 rounding (about 6e-6) apart, more than the G10 rows' tolerance, which compares
float32 with float32.
Modules that are absent offline and not on this path are empty stand-ins.
Run: python tests/golden/make_golden_dynamic_query.py"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cases  # noqa: E402
import cases_tnerf  # noqa: E402

REF = "/root/reference"
for name in ["imageio", "lpips", "skimage", "skimage.measure", "skimage.metrics", "trimesh", "cv2", "configargparse",
             "torch.utils.tensorboard", "tqdm", "dataloader", "dataloader.load_blender_dnerf"]:
    try:
        importlib.import_module(name)
    except Exception:
        sys.modules[name] = types.ModuleType(name)
sys.modules["skimage"].measure = sys.modules["skimage.measure"]
for attr in ("peak_signal_noise_ratio", "structural_similarity"):
    if not hasattr(sys.modules["skimage.metrics"], attr):
        setattr(sys.modules["skimage.metrics"], attr, None)
if not hasattr(sys.modules["torch.utils.tensorboard"], "SummaryWriter"):
    sys.modules["torch.utils.tensorboard"].SummaryWriter = object
for attr in ("tqdm", "trange"):
    if not hasattr(sys.modules["tqdm"], attr):
        setattr(sys.modules["tqdm"], attr, lambda x, *a, **k: x)
if not hasattr(sys.modules["dataloader.load_blender_dnerf"], "load_blender_data"):
    sys.modules["dataloader.load_blender_dnerf"].load_blender_data = None

import torch  # noqa: E402
sys.path.insert(0, REF)
import embedder as EMB  # noqa: E402
import model as MODEL   # noqa: E402


def _load(path, name):
    cwd = os.getcwd()
    os.chdir(os.path.dirname(path))
    sys.path.insert(0, os.path.dirname(path))
    try:
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        os.chdir(cwd)
        sys.path.pop(0)
    return mod


EM = _load(os.path.join(REF, "nerf", "extract_mesh.py"), "ref_extract_mesh")
DRUN = _load(os.path.join(REF, "d_nerf", "run_dnerf.py"), "ref_dnerf_run")
TRUN = _load(os.path.join(REF, "t_nerf", "run_tnerf.py"), "ref_tnerf_run")
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
TIMES = (0.0, 0.5)


def grid_points():
    """the points of nerf/extract_mesh.py sample_grid :40-46 on the G10 grid, float32 as batch_query_fn makes them (:157)"""
    ax = [np.linspace(b[0], b[1], cases.G10_RES) for b in cases.G10_BOUNDS]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=-1).astype(np.float32)


@torch.no_grad()
def main():
    e10, _ = EMB.get_embedder(10, 3, 0)
    e4, _ = EMB.get_embedder(4, 3, 0)
    et, _ = EMB.get_embedder(10, 1, 0)
    pts = grid_points()
    vd = EM.generate_viewdirs(cases.G10_VIEWS).astype(np.float32)
    M, V = len(pts), len(vd)
    sd_d, sd_t = cases.weights_dnerf(), cases_tnerf.weights()
    dn = MODEL.NeRF.get_by_name("direct_temporal", D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27,
                                input_ch_time=21, use_viewdirs=True, embed_fn=e10, zero_canonical=True)
    dn.load_state_dict({k: T(v) for k, v in sd_d.items()}, strict=True)
    tn = MODEL.TNeRF(**cases_tnerf.NET)
    tn.load_state_dict({k: T(v) for k, v in sd_t.items()}, strict=True)
    tn64 = MODEL.TNeRF(**cases_tnerf.NET).double()
    tn64.load_state_dict({k: T(v).double() for k, v in sd_t.items()}, strict=True)
    tn64_fn = lambda inp, vdir, dyn_t: tn64(inp.double(), vdir.double(), dyn_t.double())     # run_network hands over float32 encodings
    out = {"crc": cases.checksum(pts, vd, np.array(TIMES), *[sd_d[k] for k in sorted(sd_d)], *[sd_t[k] for k in sorted(sd_t)])}
    for t in TIMES:
        tag = "t0" if t == 0.0 else "t5"
        ft = torch.full((M, 1), t)
        raws, dxs, traws, traws32 = [], [], [], []
        for v in range(V):
            dirs = T(vd[v][None]).expand(M, 3)
            o, dx = DRUN.run_network(T(pts)[:, None], dirs, ft, dn.eval(), embed_fn=e10, embeddirs_fn=e4, embedtime_fn=et, netchunk=65536)
            raws.append(o[:, 0].numpy())
            dxs.append(dx[:, 0].numpy())
            o = TRUN.run_network(T(pts)[:, None], dirs, ft, tn.eval(), embed_fn=e10, embeddirs_fn=e4, embedtime_fn=et, netchunk=65536)
            traws32.append(o[:, 0].numpy())
            o = TRUN.run_network(T(pts)[:, None], dirs, ft, tn64_fn, embed_fn=e10, embeddirs_fn=e4, embedtime_fn=et, netchunk=65536)
            traws.append(o[:, 0].numpy())
        raws, dxs, traws, traws32 = np.stack(raws), np.stack(dxs), np.stack(traws), np.stack(traws32)
        assert traws.dtype == np.float64 and traws32.dtype == np.float32
        assert all(np.array_equal(dxs[0], d) for d in dxs) and all(np.array_equal(raws[0][:, 3], r[:, 3]) for r in raws)
        out[f"dnerf_{tag}_raw"] = raws                           # [V,M,4]
        out[f"dnerf_{tag}_mean"] = raws[..., :3].astype(np.float64).mean(0)
        out[f"dnerf_{tag}_sigma"] = raws[0][:, 3]
        out[f"dnerf_{tag}_dx"] = dxs[0]
        out[f"tnerf_{tag}_raw"] = traws
        out[f"tnerf_{tag}_raw_f32"] = traws32
        out[f"tnerf_{tag}_mean"] = traws[..., :3].mean(0)
        out[f"tnerf_{tag}_sigma"] = traws[0][:, 3]
        print(f"t = {t}: D-NeRF sigma [{raws[0][:, 3].min():.2f}, {raws[0][:, 3].max():.2f}], |dx| max {np.abs(dxs[0]).max():.3f}; "
              f"T-NeRF sigma [{traws[0][:, 3].min():.2f}, {traws[0][:, 3].max():.2f}], rgb > 0 {float((traws[..., :3] > 0).mean()):.2f}, "
              f"max |float64 - float32| {np.abs(traws - traws32).max():.2e}")
    path = os.path.join(HERE, "g17_dynamic_query.npz")
    np.savez_compressed(path, **out)
    print("wrote g17_dynamic_query.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
