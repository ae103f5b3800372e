"""T-NeRF on the host (no GPU): the TNeRF module's layout and initialisation against the reference (G14), the float64
restatement tests/tnerf_ref.py against the reference's outputs, the runner mirror, the drop-in export, the packed size
and the argument errors of the new kind and entry points (all rejected before any device call)."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "sw-nerf_amd"), os.path.join(HERE, "golden"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import cases_tnerf as C  # noqa: E402
import tnerf_ref as R    # noqa: E402

G = np.load(os.path.join(HERE, "golden", "g14_tnerf.npz"))


def test_g14_inputs_unchanged():
    assert int(G["checksum"][0]) == int(C.inputs_checksum()[0])


def test_tnerf_parameters_match_reference():
    from swnerf.model import TNeRF
    net = TNeRF(**C.NET)
    sd = net.state_dict()
    assert list(sd.keys()) == [str(n) for n in G["init_names"]]
    shapes = [[d for d in s if d] for s in G["init_shapes"].tolist()]
    assert [list(v.shape) for v in sd.values()] == shapes
    assert sum(p.numel() for p in net.parameters()) == 164036


def test_tnerf_seed0_init_matches_reference():
    from swnerf.model import TNeRF
    torch.manual_seed(0)
    sd = TNeRF(**C.NET).state_dict()
    sums = np.array([float(v.double().sum()) for v in sd.values()])
    np.testing.assert_allclose(sums, G["init_sums"], rtol=0, atol=1e-9)


def _sd64():
    return {k: torch.from_numpy(v).double() for k, v in C.weights().items()}


def test_float64_restatement_forward():
    pts, dirs, t = C.forward_rows()
    T = torch.from_numpy
    ed = R.embed(T(dirs), 4)
    fw = R.forward(_sd64(), torch.cat([R.embed(T(pts), 10), ed], -1), ed, R.embed(T(t), 10)).numpy()
    # the reference runs in float32 through 11 layers: ~1e-6 relative (measured 5.3e-6 absolute on values up to 6.7)
    np.testing.assert_allclose(fw, G["fwd"][0], rtol=0, atol=1e-5)


@pytest.mark.parametrize("name", list(C.CASES))
def test_float64_restatement_render_rays(name):
    kw = dict(C.CASES[name])
    N, S = C.N_RAYS, C.N_SAMPLES
    T = torch.from_numpy
    z = T(C.given_z()) if kw.pop("z_vals", False) else None
    tr = T(C.legacy_rand(N, S)) if kw.pop("perturb", 0) else None
    std = kw.pop("raw_noise_std", 0)
    nz = T(C.legacy_rand(N, S)) * std if std else None
    r = R.render_rays(_sd64(), T(C.rays()), S, z_vals=z, t_rand=tr, noise=nz, **kw)
    for k in ("rgb_map", "disp_map", "acc_map"):
        np.testing.assert_allclose(r[k].numpy(), G[f"{name}_{k}"], rtol=0, atol=1e-6, err_msg=k)
    np.testing.assert_allclose(r["raw"].numpy()[:C.KEEP], G[f"{name}_raw"], rtol=0, atol=1e-5)            # measured <= 6.9e-6
    np.testing.assert_array_equal(r["z_vals"].numpy()[:C.KEEP], G[f"{name}_z_vals"])


def test_render_tnerf_parameter_lists():
    import inspect
    from swnerf import render_tnerf
    for fn in ("batchify", "run_network", "render_rays", "batchify_rays", "render", "render_path"):
        assert list(inspect.signature(getattr(render_tnerf, fn)).parameters) == [str(p) for p in G[f"sig_{fn}"]], fn


def _args(tmp_path):
    return types.SimpleNamespace(multires=10, i_embed=0, use_viewdirs=True, multires_views=4, netdepth=8, netchunk=65536,
                                 nerf_type="original", lrate=5e-4, do_half_precision=False, ft_path=None, no_reload=True,
                                 perturb=1., N_samples=64, white_bkgd=True, raw_noise_std=0.5, dataset_type="blender",
                                 no_ndc=False, lindisp=False, N_importance=128, basedir=str(tmp_path), expname="exp")


def test_create_tnerf_matches_reference_record(tmp_path):
    from swnerf.runner import create_tnerf
    tr, te, start, gv, opt = create_tnerf(_args(tmp_path), device="cpu")
    assert list(tr.keys()) == [str(k) for k in G["runner_train_keys"]]
    assert list(te.keys()) == [str(k) for k in G["runner_test_keys"]]
    assert [tr["N_importance"], start, len(gv), sum(p.numel() for p in gv)] == G["runner_values"].tolist()
    assert [type(tr["network_fn"]).__name__, type(opt).__name__] == [str(c) for c in G["runner_classes"]]
    assert [float(te["perturb"]), float(te["raw_noise_std"])] == G["runner_test_perturb_noise"].tolist()
    a = _args(tmp_path)
    a.do_half_precision = True
    with pytest.raises(NotImplementedError):
        create_tnerf(a, device="cpu")


def test_dropin_exports_tnerf():
    import importlib.util
    import swnerf.model
    spec = importlib.util.spec_from_file_location("dropin_model_t", os.path.join(ROOT, "sw-nerf_amd", "dropin", "model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.TNeRF is swnerf.model.TNeRF


@pytest.fixture(scope="module")
def L():
    from swnerf import _lib
    return _lib.lib()


def test_packed_floats_tnerf(L):
    steps = 40 + 544
    assert L.swnerf_packed_floats(3) == (steps + 16) * 256 + 45 * 32 + 64 * 160 + 64 == 165344
    assert L.swnerf_packed_floats(7) == 0


def _err(L):
    return L.swnerf_last_error().decode()


def test_tnerf_argument_errors_without_gpu(L):
    from swnerf import _lib
    fake = ctypes.c_void_p(16)                          # never dereferenced: every case fails before any device call

    def args(**kw):
        a = _lib.PassArgs()
        a.ray_batch, a.n_rays, a.cols, a.kind, a.packed = fake.value, 4, 12, _lib.NET_TNERF, fake.value
        a.L_pos, a.L_dir, a.L_time, a.n_samples = 10, 4, 10, 64
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for kw, msg in ((dict(n_importance=8), "N_importance"), (dict(cols=11), "12-column"), (dict(L_dir=0), "L_dir"),
                    (dict(L_pos=11), "exceed (10,4,10)"), (dict(L_time=12), "exceed (10,4,10)"), (dict(L_dir=5), "exceed (10,4,10)")):
        assert L.swnerf_render_pass(args(**kw), None) != 0, kw
        assert msg in _err(L), (kw, _err(L))
    arr = (ctypes.c_void_p * 24)(*([fake.value] * 24))
    assert L.swnerf_pack_net(3, arr, 10, 0, 10, fake, None) != 0 and "T-NeRF" in _err(L)
    assert L.swnerf_pack_net(3, arr, 11, 4, 10, fake, None) != 0
    arr[5] = None
    assert L.swnerf_pack_net(3, arr, 10, 4, 10, fake, None) != 0 and "params[5]" in _err(L)
    assert L.swnerf_linear_act(fake, 4, 4, 4, fake, None, 4, 3, fake, 4, None) != 0 and "unknown activation" in _err(L)
    assert L.swnerf_elu_grad(None, fake, 4, None) != 0 and "elu_grad" in _err(L)
    assert L.swnerf_elu_grad(None, None, 0, None) == 0
