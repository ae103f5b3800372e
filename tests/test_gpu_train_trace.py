"""The launch structure of the fused training passes: which `swnerf_*` entry is called, in which order and on which stream, and
what a forward pass leaves allocated - what the float64 gradient tests cannot see.

For each of the four kinds (canon, noview, dnerf, tnerf) one `loss.backward()` goes through the runner's render_rays (T-NeRF
inside `fused_train()`): n = 10 rays, S = 33 (two 32-row tiles per ray, the second ragged: 64 padded rows per ray), N_importance
= 0, perturb = 0, raw_noise_std = 0, white_bkgd, a fresh seeded net on the default bands (so the pack calls appear), with
render.TRAIN_BWD_CHUNK_ROWS = 256: chunks of 4, 4 and 2 rays for every kind (D-NeRF's divisor of 2 meets the floor of 4 rays).

A recorder around `_lib.lib()` (the spy of tests/test_gpu_bands.py) notes (name, where) of every `swnerf_*` call: "main" when
the trailing stream argument is the current stream, "side" for any other stream (wgrad._Fan), "-" for a call that takes none
(the size queries).  EXPECTED and FORWARD_BYTES below were obtained by running THIS module, unchanged, on the commit before the
training passes moved into swnerf/train_pass.py - it only goes through render_rays, so it runs there as it is.  They are not
derived from the code they check.  FORWARD_BYTES is the allocator's count of requested bytes (memory_stats "requested_bytes.all.current":
what torch.cuda.memory_allocated() counts, without the rounding to whole blocks) after the forward minus before it.  memory_allocated()
itself hands back whole blocks - a cached block up to 1 MiB larger than a request is not split - so its difference depends on what
earlier tests of the process left in the cache: it read 8 662 016 for the no-view net in a process of its own and 8 681 984 behind the
rest of the suite.  It is printed beside the asserted figure.  The requested bytes read the same on that commit in a process of
their own and behind tests/test_gpu_tnerf_train.py and tests/test_gpu_backward.py (in whole blocks there: 9 118 208, 8 662 016,
19 929 600, 3 783 168).

The no-view net's `views_linears` belongs to the module but no pass reads it (tests/test_gpu_bands.py), so its gradient stays
None; every other parameter of every kind must have a finite gradient of its own shape."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N_RAYS, S, CHUNK_ROWS = 10, 33, 256
KINDS = ("canon", "noview", "dnerf", "tnerf")


def _net(kind):
    import swnerf.model as model
    from swnerf.embedder import get_embedder
    torch.manual_seed(7)
    if kind == "canon":
        m = model.vallina_NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
    elif kind == "noview":
        m = model.vallina_NeRF(D=8, W=256, input_ch=63, input_ch_views=0, output_ch=5, skips=[4], use_viewdirs=False)
    elif kind == "dnerf":
        m = model.DirectTemporalNeRF(D=8, W=256, input_ch=63, input_ch_views=27, input_ch_time=21, output_ch=5, skips=[4],
                                     use_viewdirs=True, embed_fn=get_embedder(10, 3, 0)[0], zero_canonical=True)
    else:
        m = model.TNeRF(8, 63, 27, 21, 128, 4)
    return m.to(DEV).train()


def _query(kind):
    """The lambda the runners' create_* build (nerf/run.py:248-251, run_dnerf.py:281-286, run_tnerf.py:270-276)"""
    import swnerf.render as render, swnerf.render_dnerf as rd, swnerf.render_tnerf as rt
    from swnerf.embedder import get_embedder
    embed_fn, _ = get_embedder(10, 3, 0)
    embeddirs_fn = None if kind == "noview" else get_embedder(4, 3, 0)[0]
    embedtime_fn, _ = get_embedder(10, 1, 0)
    if kind in ("canon", "noview"):
        return lambda inputs, viewdirs, network_fn: render.run_network(inputs, viewdirs, network_fn, embed_fn=embed_fn,
                                                                       embeddirs_fn=embeddirs_fn)
    mod = rd if kind == "dnerf" else rt
    return lambda inputs, viewdirs, ts, network_fn: mod.run_network(inputs, viewdirs, ts, network_fn, embed_fn=embed_fn,
                                                                    embeddirs_fn=embeddirs_fn, embedtime_fn=embedtime_fn)


def _rays(kind):
    """[o, d, near, far, (t = 0.5), (viewdirs)]: origins on a sphere of radius 4 looking at the unit ball"""
    rng = np.random.default_rng(3)
    o = rng.normal(size=(N_RAYS, 3))
    o = 4. * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = rng.uniform(-1, 1, (N_RAYS, 3)) - o
    v = d / np.linalg.norm(d, axis=1, keepdims=True)
    cols = [o, d, np.full((N_RAYS, 1), 2.), np.full((N_RAYS, 1), 6.)]
    if kind in ("dnerf", "tnerf"):
        cols.append(np.full((N_RAYS, 1), 0.5))
    if kind != "noview":
        cols.append(v)
    return torch.from_numpy(np.concatenate(cols, 1).astype(np.float32)).to(DEV)


def trace(kind, monkeypatch):
    """One training step of `kind` -> (the recorded [(name, where)], bytes the forward left allocated, the net)"""
    import swnerf.render as render, swnerf.render_dnerf as rd, swnerf.render_tnerf as rt
    from swnerf import _lib
    net, q, rb = _net(kind), _query(kind), _rays(kind)
    target = torch.rand((N_RAYS, 3), generator=torch.Generator().manual_seed(5)).to(DEV)
    monkeypatch.setattr(render, "TRAIN_BWD_CHUNK_ROWS", CHUNK_ROWS)
    monkeypatch.delenv("SWNERF_TRAIN_OP_PATH", raising=False)
    calls = []
    real = _lib.lib()

    class Recorder:
        def __getattr__(self, name):
            f = getattr(real, name)
            if not name.startswith("swnerf_"):
                return f

            def wrapped(*a):
                where = "-"
                if _lib.SIGNATURES[name][1][-1:] == ["void*"]:          # the trailing `void* stream` of include/swnerf.h
                    st = getattr(a[-1], "value", a[-1]) or 0
                    where = "main" if st == torch.cuda.current_stream(DEV).cuda_stream else "side"
                calls.append((name, where))
                return f(*a)
            return wrapped
    monkeypatch.setattr(_lib, "lib", lambda: Recorder())
    kw = dict(N_importance=0, perturb=0., raw_noise_std=0., white_bkgd=True)
    live = lambda: (torch.cuda.memory_stats(DEV)["requested_bytes.all.current"], torch.cuda.memory_allocated(DEV))
    gc.collect()
    torch.cuda.synchronize()
    before = live()
    with torch.enable_grad():
        if kind in ("canon", "noview"):
            ret = render.render_rays(rb, net, q, S, **kw)
        elif kind == "dnerf":
            ret = rd.render_rays(rb, net, q, S, **kw)
        else:
            with rt.fused_train():
                ret = rt.render_rays(rb, net, q, S, **kw)
        torch.cuda.synchronize()
        forward_bytes, in_blocks = (a - b for a, b in zip(live(), before))
        print(f"\n[trace] {kind}: the forward left {forward_bytes} requested bytes allocated ({in_blocks} in whole blocks)")
        loss = ((ret["rgb_map"] - target) ** 2).mean()
        if kind == "dnerf":                                  # run_dnerf.py:690-725 puts a gradient on position_delta as well
            loss = loss + 1e-3 * (ret["position_delta"] ** 2).mean()
        loss.backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(_lib, "lib", lambda: real)
    return calls, forward_bytes, net


def _c(text):
    """'name where, name where, ...' -> [(swnerf_name, where)]"""
    return [("swnerf_" + c.split()[0], c.split()[1]) for c in text.split(",")]


_STATIC_FWD = "train_rows -, act_floats_per_row -, mask_floats -, xs_floats_per_row -, render_pass_train main"
EXPECTED = {
    "canon": (_c("packed_floats -, pack_net main, " + _STATIC_FWD + ", packed_bwd_floats_kind -, pack_net_bwd_kind main")
              + 3 * _c("render_pass_backward main, gemm_tn_group main, canon_narrow_grads main")
              + _c("unslot_grad main, unslot_grad main, unslot_grad main, feature_finish main")),
    "noview": (_c("packed_floats -, pack_net_noview main, " + _STATIC_FWD + ", packed_bwd_noview_floats -, pack_net_bwd_noview main")
               + 3 * _c("render_pass_backward_noview main, gemm_tn_group main, gemm_tn side, gemm_tn side")
               + _c("unslot_grad main, unslot_grad main")),
    "dnerf": (_c("packed_floats -, pack_net main, train_rows -, act_floats_per_row -, xs_floats_per_row -, mask_floats -, "
                 "render_pass_train_dnerf main, packed_bwd_floats_kind -, pack_net_bwd_kind main")
              + 3 * _c("render_pass_backward_dnerf main, gemm_tn_group main, canon_narrow_grads main, deform_narrow_grads main")
              + _c("unslot_grad main, unslot_grad main, unslot_grad main, feature_finish main, "
                   "unslot_grad main, unslot_grad main, unslot_grad_time main")),
    "tnerf": (_c("packed_floats -, pack_net main, train_rows -, tnerf_act_floats_per_row -, tnerf_xs_floats_per_row -, "
                 "render_pass_train_tnerf main, packed_bwd_tnerf_floats -, pack_net_bwd_tnerf main")
              + 3 * (_c("render_pass_backward_tnerf main") + 13 * _c("gemm_tn side"))
              + _c("unslot_grad main, unslot_grad_time main, unslot_grad main, unslot_grad_time main, unslot_grad main, "
                   "tnerf_feature_finish main")),
}
FORWARD_BYTES = {"canon": 9115920, "noview": 8660024, "dnerf": 19927432, "tnerf": 3781136}


@pytest.mark.parametrize("kind", KINDS)
def test_training_step_call_trace(kind, monkeypatch):
    """The recorded calls equal the literal list, the forward leaves the recorded number of bytes allocated, and every parameter
    a pass trains has a finite gradient of its own shape."""
    calls, forward_bytes, net = trace(kind, monkeypatch)
    assert calls == EXPECTED[kind], "\n".join(f"{i}: {c}" for i, c in enumerate(calls))
    assert forward_bytes == FORWARD_BYTES[kind]
    for name, p in net.named_parameters():
        if kind == "noview" and name.startswith("views_linears"):
            assert p.grad is None, name
            continue
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), name
