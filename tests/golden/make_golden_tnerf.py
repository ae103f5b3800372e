#!/usr/bin/env python3
"""Capture golden vectors G14 from the UNMODIFIED reference (build container only): TNeRF (model.py:152-210) and
render_rays / create_nerf of t_nerf/run_tnerf.py on seeded weights (cases_tnerf.py).  Only OUTPUTS (plus a checksum
of the seeded inputs) are stored.
Run: python tests/golden/make_golden_tnerf.py"""
import inspect
import os
import sys
import tempfile
import types
import importlib
import importlib.util
import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cases_tnerf as C  # noqa: E402

REF = "/root/reference"
for name in ["imageio", "lpips", "skimage", "skimage.metrics", "cv2", "configargparse", "torch.utils.tensorboard", "tqdm",
             "dataloader", "dataloader.load_blender_dnerf"]:
    try:
        importlib.import_module(name)
    except Exception:
        sys.modules[name] = types.ModuleType(name)
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
import embedder as EMB     # noqa: E402
import model as MODEL      # noqa: E402


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


RUN = _load(os.path.join(REF, "t_nerf", "run_tnerf.py"), "ref_tnerf_run")
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
out = {"checksum": C.inputs_checksum()}

# runner record: create_nerf's return, the render functions' parameter lists
for fn in ("batchify", "run_network", "render_rays", "batchify_rays", "render", "render_path", "create_nerf"):
    out[f"sig_{fn}"] = np.array([p for p in inspect.signature(getattr(RUN, fn)).parameters])
args = types.SimpleNamespace(multires=10, i_embed=0, use_viewdirs=True, multires_views=4, netdepth=8, netchunk=65536,
                             nerf_type="original", lrate=5e-4, do_half_precision=False, ft_path=None, no_reload=True,
                             perturb=1., N_samples=64, white_bkgd=True, raw_noise_std=0.5, dataset_type="blender",
                             no_ndc=False, lindisp=False, N_importance=128)
with tempfile.TemporaryDirectory() as d:
    os.makedirs(os.path.join(d, "exp"))
    args.basedir, args.expname = d, "exp"
    torch.manual_seed(0)
    tr, te, start, gv, opt = RUN.create_nerf(args)
out["runner_train_keys"] = np.array(list(tr.keys()))
out["runner_test_keys"] = np.array(list(te.keys()))
out["runner_values"] = np.array([tr["N_importance"], start, len(gv), sum(p.numel() for p in gv)], np.int64)
out["runner_classes"] = np.array([type(tr["network_fn"]).__name__, type(opt).__name__])
out["runner_test_perturb_noise"] = np.array([float(te["perturb"]), float(te["raw_noise_std"])])

# seed-0 initial state_dict: names, shapes, per-tensor sums
torch.manual_seed(0)
net0 = MODEL.TNeRF(**C.NET)
sd0 = net0.state_dict()
out["init_names"] = np.array(list(sd0.keys()))
out["init_shapes"] = np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sd0.values()], np.int64)
out["init_sums"] = np.array([float(v.double().sum()) for v in sd0.values()])

torch.set_grad_enabled(False)
net = MODEL.TNeRF(**C.NET)
net.load_state_dict({k: T(v) for k, v in C.weights().items()}, strict=True)
embed_fn, _ = EMB.get_embedder(10, 3, 0)
embedtime_fn, _ = EMB.get_embedder(10, 1, 0)
embeddirs_fn, _ = EMB.get_embedder(4, 3, 0)

# TNeRF.forward rows (inp = [gamma(x) | gamma(d)], sliced inside forward)
pts, dirs, t = C.forward_rows()
vd = embeddirs_fn(T(dirs))
fw = net(torch.cat([embed_fn(T(pts)), vd], -1), vd, embedtime_fn(T(t)))
out["fwd"] = fw.numpy()

query = lambda inputs, viewdirs, ts, network_fn: RUN.run_network(inputs, viewdirs, ts, network_fn, embed_fn=embed_fn,
                                                                 embeddirs_fn=embeddirs_fn, embedtime_fn=embedtime_fn,
                                                                 netchunk=1024 * 64)
rb = T(C.rays())
N, S = C.N_RAYS, C.N_SAMPLES
for name, kw in C.CASES.items():
    kw = dict(kw)
    real_rand = torch.rand
    if kw.get("z_vals"):
        kw["z_vals"] = T(C.given_z())
    if kw.get("raw_noise_std", 0) > 0:
        kw["pytest"] = True                     # noise = np.random.seed(0); rand(N, S) * raw_noise_std (run_tnerf.py:371-374)
    if kw.get("perturb", 0) > 0:
        torch.rand = lambda *a, **k: T(C.legacy_rand(N, S))       # the stratified draw, injected
    try:
        ret = RUN.render_rays(rb, net, query, S, retraw=True, **kw)
    finally:
        torch.rand = real_rand
    for k in ("rgb_map", "disp_map", "acc_map"):
        out[f"{name}_{k}"] = ret[k].numpy()
    out[f"{name}_raw"] = ret["raw"][:C.KEEP].numpy()
    out[f"{name}_z_vals"] = ret["z_vals"][:C.KEEP].numpy()
    raw = ret["raw"]
    print(f"{name}: acc [{float(ret['acc_map'].min()):.3f}, {float(ret['acc_map'].max()):.3f}] mean {float(ret['acc_map'].mean()):.3f}; "
          f"raw rgb>0 {float((raw[..., :3] > 0).float().mean()):.2f}, sigma>0 {float((raw[..., 3] > 0).float().mean()):.2f}")

# sign coverage: the fraction of positive pre-activations at every ELU and at the colour ReLU (det case rows)
pts_all = (rb[:, None, :3] + rb[:, None, 3:6] * T(out["det_z_vals"][:1]).expand(N, S)[..., None]).reshape(-1, 3)
inp = torch.cat([embed_fn(pts_all), embedtime_fn(torch.full((pts_all.shape[0], 1), C.FRAME_TIME))], -1)
x, fr = inp, []
for i in range(8):
    pre = net.layers[i][0](x)
    fr.append(float((pre > 0).float().mean()))
    x = net.layers[i][1](pre)
    if i == 4:
        x = torch.cat([inp, x], -1)
out["pos_fraction"] = np.array(fr)
print("positive fraction before each ELU:", np.round(fr, 2))
np.savez_compressed(os.path.join(HERE, "g14_tnerf.npz"), **out)
print("wrote g14_tnerf.npz", os.path.getsize(os.path.join(HERE, "g14_tnerf.npz")), "bytes")
