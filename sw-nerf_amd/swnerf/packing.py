"""The one cache in front of every weight-pack entry point (model.py, fit2d.py).  The rule, written once: a packed stream is
reused while no tensor it was built from changed in place (optimizer step, load_state_dict) or moved; otherwise it is built
again into a NEW tensor - a blob that another stream may still read (render.prepack, parallel.frame_renderer) is never
overwritten."""
import ctypes

import torch

from . import _lib

NOT_ON_GPU = "swnerf: module parameters must be on the GPU (call .to('cuda')); no CPU fallback"


def cached(cache, slot, tensors, build, extra=()):
    """cache[slot]'s object while (data_ptr, _version) of every tensor, followed by `extra`, is what it was built for; else
    build(tensors), stored and returned.  `cache` is a plain dict on the module (modules are deep-copied and pickled); `extra`
    is a tuple for what torch's version counter does not see."""
    key = tuple((t.data_ptr(), t._version) for t in tensors) + tuple(extra)
    hit = cache.get(slot)
    if hit is None or hit[0] != key:
        hit = cache[slot] = (key, build(tensors))
    return hit[1]


def pack_weights(cache, slot, tensors, n_floats, pack, what, extra=(), keyed_on=None):
    """The float32 device tensor of n_floats(lib) floats that pack(lib, pointer array of `tensors` as fp32-contiguous, blob
    pointer, stream) -> rc fills on the current stream, cached under `slot` on `keyed_on` (default: `tensors`) and `extra`.
    Tensors off the GPU are refused before the library is touched."""
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(NOT_ON_GPU)

    def build(_):
        L = _lib.lib()
        t32 = [t.detach() if (t.dtype == torch.float32 and t.is_contiguous()) else t.detach().float().contiguous() for t in tensors]
        arr = (ctypes.c_void_p * len(t32))(*[t.data_ptr() for t in t32])
        blob = torch.empty(n_floats(L), dtype=torch.float32, device=tensors[0].device)
        _lib.check(pack(L, arr, _lib.ptr(blob), _lib.stream_of(blob)), what)
        return blob
    return cached(cache, slot, tensors if keyed_on is None else keyed_on, build, extra)
