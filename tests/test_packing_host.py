"""CPU-only checks of swnerf/packing.py: the keyed cache (layer 1) on CPU tensors with a counting build, and the refusal the
weight-pack wrapper (layer 2) makes for every packed stream of a module that is not on the GPU - before the library is loaded."""
import copy

import pytest
import torch
import torch.nn as nn

from swnerf import _lib, fit2d, model, packing


class Counter:
    def __init__(self):
        self.n = 0

    def __call__(self, tensors):
        self.n += 1
        return [self.n, len(tensors)]


def test_cache_returns_the_same_object_until_a_tensor_changes_or_moves():
    cache, build = {}, Counter()
    a, b = torch.zeros(3), torch.zeros(2, 2)
    first = packing.cached(cache, "s", [a, b], build)
    assert first == [1, 2] and packing.cached(cache, "s", [a, b], build) is first and build.n == 1
    with torch.no_grad():
        b.add_(1.)                                                              # changed in place
    second = packing.cached(cache, "s", [a, b], build)
    assert second is not first and second == [2, 2] and packing.cached(cache, "s", [a, b], build) is second
    a.data = a.data.clone()                                                     # moved
    third = packing.cached(cache, "s", [a, b], build)
    assert third is not second and build.n == 3 and packing.cached(cache, "s", [a, b], build) is third
    assert first == [1, 2] and second == [2, 2]                                 # a rebuild leaves what it handed out before alone


def test_cache_extra_key_part_and_independent_slots():
    cache, build = {}, Counter()
    a = torch.zeros(3)
    x = packing.cached(cache, "x", [a], build, extra=(0,))
    assert packing.cached(cache, "x", [a], build, extra=(0,)) is x and build.n == 1
    y = packing.cached(cache, "y", [a], build, extra=(0,))                      # another slot: its own build ...
    assert y is not x and build.n == 2 and packing.cached(cache, "x", [a], build, extra=(0,)) is x     # ... and x stays
    x1 = packing.cached(cache, "x", [a], build, extra=(1,))                     # extra changed: x rebuilds, y does not
    assert x1 is not x and build.n == 3 and packing.cached(cache, "y", [a], build, extra=(0,)) is y
    assert set(cache) == {"x", "y"} and type(cache) is dict


def test_cache_dict_survives_deepcopy_of_its_module():
    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = nn.Linear(2, 2)
            self._pack_cache = {}

        def packed(self, build):
            return packing.cached(self._pack_cache, "fwd", list(self.parameters()), build)

    m, build = M(), Counter()
    blob = m.packed(build)
    twin = copy.deepcopy(m)
    assert type(twin._pack_cache) is dict and twin._pack_cache is not m._pack_cache
    assert m.packed(build) is blob and build.n == 1
    assert twin.packed(build) is not blob and build.n == 2                      # the copy's parameters live elsewhere: its own build
    assert m.packed(build) is blob


def _streams():
    views = model.vallina_NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
    noview = model.vallina_NeRF(D=8, W=256, input_ch=63, input_ch_views=0, output_ch=5, skips=[4], use_viewdirs=False)
    dnerf = model.DirectTemporalNeRF(D=8, W=256, input_ch=63, input_ch_views=27, input_ch_time=21, output_ch=5, skips=[4],
                                     use_viewdirs=True)
    tnerf = model.TNeRF(depth=8, in_feat=63, dir_feat=27, time_feat=21, net_dim=128, skip_layer=4)
    picture = fit2d.Model(input_dimension=2 + 4 * 4, layer_num=2)
    out = [("views." + n, getattr(views, n)) for n in ("packed", "packed_bwd", "packed_x3")]
    out += [("views.packed_bwd(1)", lambda: views.packed_bwd(_lib.BWD_CANON_INPUT_GRAD))]
    out += [("noview." + n, getattr(noview, n)) for n in ("packed_noview", "packed_bwd_noview")]
    out += [("dnerf." + n, getattr(dnerf, n)) for n in ("packed", "packed_x3")]
    out += [(f"dnerf.packed_bwd({k})", lambda k=k: dnerf.packed_bwd(k)) for k in (_lib.BWD_CANON, _lib.BWD_CANON_INPUT_GRAD, _lib.BWD_DEFORM,
                                                                                 _lib.BWD_DNERF_FUSED)]
    out += [("tnerf." + n, getattr(tnerf, n)) for n in ("packed", "packed_bwd")]
    return out + [("fit2d.packed", picture.packed)]


def test_every_packed_stream_refuses_a_cpu_module_before_the_library_loads(monkeypatch):
    def no_library():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "lib", no_library)
    for name, call in _streams():
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == "swnerf: module parameters must be on the GPU (call .to('cuda')); no CPU fallback", name
