"""The weight-pack cache (swnerf/packing.py) on the GPU, for every packed stream of every model family: two calls hand out
the same tensor; after an in-place parameter update the call hands out ANOTHER tensor that equals the stream of a freshly
built module with the same state_dict, and the tensor handed out before still holds what it held (render.prepack and
parallel.frame_renderer read it on other streams).  Launches the pack kernels only, no render."""
import pytest
import torch

from swnerf import _lib, fit2d, model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

_net = dict(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
_bwd = lambda kind: (lambda m: m.packed_bwd(kind))
_fwd, _x3 = (lambda m: m.packed()[1]), (lambda m: m.packed_x3()[0])
# family: (constructor, the parameter that is updated, {stream: call -> blob})
FAMILIES = {
    "views": (lambda: model.vallina_NeRF(**_net), "pts_linears.3.weight",
              {"fwd": _fwd, "x3": _x3, "bwd": _bwd(_lib.BWD_CANON), "bwd_input_grad": _bwd(_lib.BWD_CANON_INPUT_GRAD)}),
    "noview": (lambda: model.vallina_NeRF(**{**_net, "input_ch_views": 0, "use_viewdirs": False}), "pts_linears.3.weight",
               {"fwd": lambda m: m.packed_noview()[0], "bwd": lambda m: m.packed_bwd_noview()}),
    "dnerf_canonical": (lambda: model.DirectTemporalNeRF(input_ch_time=21, **_net), "_occ.pts_linears.3.weight",
                        {"fwd": _fwd, "x3": _x3, "bwd": _bwd(_lib.BWD_CANON), "bwd_input_grad": _bwd(_lib.BWD_CANON_INPUT_GRAD),
                         "bwd_fused": _bwd(_lib.BWD_DNERF_FUSED)}),
    "dnerf_deformation": (lambda: model.DirectTemporalNeRF(input_ch_time=21, **_net), "_time.3.weight",
                          {"fwd": _fwd, "x3": _x3, "bwd_deform": _bwd(_lib.BWD_DEFORM), "bwd_fused": _bwd(_lib.BWD_DNERF_FUSED)}),
    "tnerf": (lambda: model.TNeRF(depth=8, in_feat=63, dir_feat=27, time_feat=21, net_dim=128, skip_layer=4), "layers.3.0.weight",
              {"fwd": _fwd, "bwd": lambda m: m.packed_bwd()}),
    "fit2d": (lambda: fit2d.Model(input_dimension=2 + 4 * 4, layer_num=2), "model.3.weight", {"fwd": lambda m: m.packed()}),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_repack_hands_out_a_new_tensor_and_leaves_the_old_one(family):
    make, name, streams = FAMILIES[family]
    torch.manual_seed(0)
    m = make().to(DEV)
    old = {s: call(m) for s, call in streams.items()}
    kept = {s: blob.clone() for s, blob in old.items()}
    for s, call in streams.items():
        assert call(m) is old[s], s
    with torch.no_grad():
        dict(m.named_parameters())[name].add_(0.25)
    new = {s: call(m) for s, call in streams.items()}
    twin = make()
    twin.load_state_dict(m.state_dict())
    twin = twin.to(DEV)
    for s, call in streams.items():
        assert new[s] is not old[s] and call(m) is new[s], s
        assert torch.equal(old[s], kept[s]), s                                   # never rewritten in place
        assert not torch.equal(new[s], kept[s]), s                               # and the update is in the new one
        assert torch.equal(new[s], call(twin)), s
    torch.cuda.synchronize()


def test_streams_of_untouched_parameters_are_kept():
    """The key covers exactly the tensors a stream is packed from: an update of the deformation net repacks neither canonical
    backward stream, and the other way round."""
    make, _, _ = FAMILIES["dnerf_canonical"]
    m = make().to(DEV)
    canon, deform = m.packed_bwd(_lib.BWD_CANON), m.packed_bwd(_lib.BWD_DEFORM)
    with torch.no_grad():
        m._time[3].weight.add_(0.25)
    assert m.packed_bwd(_lib.BWD_CANON) is canon and m.packed_bwd(_lib.BWD_DEFORM) is not deform
    deform = m.packed_bwd(_lib.BWD_DEFORM)
    with torch.no_grad():
        m._occ.pts_linears[3].weight.add_(0.25)
    assert m.packed_bwd(_lib.BWD_CANON) is not canon and m.packed_bwd(_lib.BWD_DEFORM) is deform


def test_fit2d_training_forward_invalidates_through_stats_version():
    """The batch-norm kernels write running_mean / running_var through raw pointers, which torch's version counter does not see."""
    torch.manual_seed(0)
    m = fit2d.Model(input_dimension=2 + 4 * 4, layer_num=2).to(DEV)
    old = m.packed()
    kept = old.clone()
    m.train()
    m.forward_layers(torch.rand(33, 18, device=DEV))
    new = m.packed()
    assert new is not old and m.packed() is new and torch.equal(old, kept) and not torch.equal(new, kept)
    twin = fit2d.Model(input_dimension=2 + 4 * 4, layer_num=2)
    twin.load_state_dict(m.state_dict())
    assert torch.equal(new, twin.to(DEV).packed())
