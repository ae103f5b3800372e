"""CPU-only checks of the creators in swnerf/runner.py (create_nerf, create_dnerf, create_tnerf, create_multires) on
device="cpu": the key order of the returned dictionaries (result_dict and user code iterate them), what the test dictionary
changes, the grad_vars counts, and that the `network_query_fn` lambda still carries the encoders and the time-discretisation flag
as the free variables render.closure_embedders / render_tnerf._time_discr look for - a render that misses them drops from the
fused pass to the op path without an error."""
from types import SimpleNamespace

import pytest
import torch

from swnerf import render, render_tnerf, runner
from swnerf.embedder import EmbedFn

HEAD = ["network_query_fn", "perturb", "N_importance", "network_fine", "N_samples", "network_fn", "use_viewdirs", "white_bkgd",
        "raw_noise_std"]
NERF_KEYS = HEAD + ["ndc", "lindisp"]
DNERF_KEYS = HEAD + ["use_two_models_for_fine", "ndc", "lindisp"]
TNERF_KEYS = ["network_query_fn", "perturb", "N_importance", "network_fn", "N_samples", "use_viewdirs", "white_bkgd", "raw_noise_std",
              "ndc", "lindisp"]


def options(tmp, **over):
    a = dict(expname="e", basedir=str(tmp), netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, lrate=5e-4, netchunk=1024 * 64,
             no_reload=True, ft_path=None, N_samples=64, N_importance=128, perturb=1., use_viewdirs=True, i_embed=0, multires=10,
             multires_views=4, raw_noise_std=1., dataset_type="blender", white_bkgd=True, no_ndc=False, lindisp=False,
             nerf_type="direct_temporal", not_zero_canonical=False, use_two_models_for_fine=True, do_half_precision=False, layer_num=2)
    a.update(over)
    return SimpleNamespace(**a)


def check_train_test(train, test, keys):
    assert list(train) == keys and list(test) == keys
    assert train["perturb"] == 1. and train["raw_noise_std"] == 1. and test["perturb"] is False and test["raw_noise_std"] == 0.
    for k in keys:
        if k not in ("perturb", "raw_noise_std"):
            assert test[k] is train[k] or test[k] == train[k], k


def check_closure(kw, timed):
    emb = render.closure_embedders(kw["network_query_fn"])
    assert set(emb) == ({"embed_fn", "embeddirs_fn", "embedtime_fn"} if timed else {"embed_fn", "embeddirs_fn"})
    assert all(isinstance(v, EmbedFn) for v in emb.values())
    return emb


def test_create_nerf(tmp_path):
    train, test, start, grad_vars, optimizer = runner.create_nerf(options(tmp_path), device="cpu")
    check_train_test(train, test, NERF_KEYS)
    assert start == 0 and len(grad_vars) == 48 and train["network_fine"] is not None and train["ndc"] is False
    emb = check_closure(train, False)
    assert (emb["embed_fn"].multires, emb["embeddirs_fn"].multires) == (10, 4)
    with torch.no_grad():
        assert render.fused_plan(train["network_query_fn"], [train["network_fn"], train["network_fine"]]) == (10, 4, 0)
    llff, llff_test, *_ = runner.create_nerf(options(tmp_path, dataset_type="llff"), device="cpu")
    assert list(llff) == HEAD and list(llff_test) == HEAD


def test_create_dnerf(tmp_path):
    train, test, start, grad_vars, optimizer = runner.create_dnerf(options(tmp_path), device="cpu")
    check_train_test(train, test, DNERF_KEYS)
    assert start == 0 and len(grad_vars) == 84 and train["use_two_models_for_fine"] is True
    emb = check_closure(train, True)
    assert (emb["embed_fn"].multires, emb["embeddirs_fn"].multires, emb["embedtime_fn"].multires) == (10, 4, 10)
    with torch.no_grad():
        assert render.fused_plan(train["network_query_fn"], [train["network_fn"], train["network_fine"]], need_time=True) == (10, 4, 10)
    assert render_tnerf._time_discr(train["network_query_fn"]) is True
    one, *_ = runner.create_dnerf(options(tmp_path, use_two_models_for_fine=False, nerf_type="original"), device="cpu")
    assert list(one) == DNERF_KEYS and one["network_fine"] is None


def test_create_tnerf(tmp_path):
    train, test, start, grad_vars, optimizer = runner.create_tnerf(options(tmp_path), device="cpu")
    check_train_test(train, test, TNERF_KEYS)
    assert start == 0 and len(grad_vars) == 24 and train["N_importance"] == 0 and "network_fine" not in train
    check_closure(train, True)
    assert render_tnerf._time_discr(train["network_query_fn"]) is True
    with torch.no_grad():
        assert render_tnerf.tnerf_plan(train["network_query_fn"], train["network_fn"]) is None       # a CPU net: no fused pass
    temporal, *_ = runner.create_tnerf(options(tmp_path, nerf_type="temporal"), device="cpu")
    assert render_tnerf._time_discr(temporal["network_query_fn"]) is False


def test_create_multires(tmp_path):
    trains, tests, starts, grads, optimizers = runner.create_multires(options(tmp_path, reproducible_wgrad=True), device="cpu")
    assert len(trains) == len(tests) == len(grads) == len(optimizers) == 2 and starts == [0, 0]
    for level, (train, test, grad_vars) in enumerate(zip(trains, tests, grads)):
        check_train_test(train, test, DNERF_KEYS)
        assert len(grad_vars) == 84
        emb = check_closure(train, True)
        # multires_dnerf.py:665: position, TIME, VIEWS
        assert (emb["embed_fn"].multires, emb["embedtime_fn"].multires, emb["embeddirs_fn"].multires) == runner.MULTIRES_CHANNELS[level]
        assert render_tnerf._time_discr(train["network_query_fn"]) is True
        assert train["network_fn"].reproducible_wgrad is True and train["network_fine"].reproducible_wgrad is True
    plain, *_ = runner.create_multires(options(tmp_path, layer_num=1), device="cpu")
    assert plain[0]["network_fn"].reproducible_wgrad is False
    assert not hasattr(runner.create_dnerf(options(tmp_path), device="cpu")[0]["network_fn"], "reproducible_wgrad")


@pytest.mark.parametrize("name", ["create_dnerf", "create_tnerf", "create_multires"])
def test_half_precision_is_refused_by_name(tmp_path, name):
    with pytest.raises(NotImplementedError, match=f"swnerf.{name}: do_half_precision"):
        getattr(runner, name)(options(tmp_path, do_half_precision=True), device="cpu")
