"""CPU-only checks of the fused optimizer's host side (csrc/optim_kernels.hip, swnerf/optim.py, runner._make_optimizer): the launch
planner as a pure function over sizes (every element of every tensor in exactly one block, the caps respected, list order kept),
the argument refusals of swnerf_adam_step (returned before anything touches the GPU), the Python refusals, the param-group keys
(torch's own, so that state dicts pass between the two optimizers) and `args.optimizer` in every creator."""
import ctypes
import inspect
from types import SimpleNamespace

import pytest
import torch

from swnerf import _lib, optim, runner

T_CAP, B_CAP, CHUNK, DESC = optim.caps()


def check_plan(sizes):
    rows = optim.launch_plan(sizes)
    # list order: rows sorted by (tensor, start), launches never decreasing
    assert rows == sorted(rows, key=lambda r: (r[1], r[2]))
    assert [r[0] for r in rows] == sorted(r[0] for r in rows)
    # every element exactly once: per tensor the blocks tile [0, n) without gap or overlap
    for t, n in enumerate(sizes):
        mine = [r for r in rows if r[1] == t]
        pos = 0
        for _, _, start, count in mine:
            assert start == pos and count >= 1 and start % CHUNK == 0, (t, start, pos)
            pos += count
        assert pos == n, (t, pos, n)
    assert all(0 <= r[1] < len(sizes) for r in rows)
    # caps per launch
    n_launches = rows[-1][0] + 1 if rows else 0
    for l in range(n_launches):
        mine = [r for r in rows if r[0] == l]
        tensors = sorted({r[1] for r in mine})
        assert 1 <= len(mine) <= B_CAP, (l, len(mine))
        assert len(tensors) <= T_CAP and tensors[-1] - tensors[0] < T_CAP, (l, tensors)       # a launch addresses tensors first .. first + 31
        chunk = max(r[3] for r in mine)
        assert chunk <= 16 * CHUNK
        if chunk > CHUNK:
            assert len(tensors) == 1                                            # only a launch that one tensor fills alone widens its blocks
    return rows, n_launches


def test_caps():
    assert (T_CAP, B_CAP, CHUNK) == (32, 320, 4096)
    assert DESC <= 4096 - 256                                                   # the by-value descriptor and the implicit arguments: 4 KB


def test_plan_small_sizes_one_launch():
    rows, n_launches = check_plan([1, 3, 255, 256, 257, 4099])
    assert n_launches == 1 and len(rows) == 7                                   # 4099 = one chunk + 3
    assert rows[-2:] == [(0, 5, 0, 4096), (0, 5, 4096, 3)]


def test_plan_one_more_tensor_than_the_cap():
    rows, n_launches = check_plan([5] * (T_CAP + 1))
    assert n_launches == 2 and [r[0] for r in rows] == [0] * T_CAP + [1]
    rows, n_launches = check_plan([1, 3, 255, 256, 257, 4099] + [5] * 70)       # the GPU test's list
    assert n_launches == 3


def test_plan_tensor_larger_than_one_launch():
    n = B_CAP * CHUNK * 16 + 5                                                  # one launch of the widest blocks, and 5 floats more
    rows, n_launches = check_plan([7, n, 9])
    assert n_launches == 3                                                      # [7 and the first chunks of n] [the rest of n, wide] [its tail and 9]
    check_plan([n])
    check_plan([B_CAP * CHUNK])                                                 # exactly one launch of plain chunks
    assert check_plan([B_CAP * CHUNK])[1] == 1
    assert check_plan([B_CAP * CHUNK + 1])[1] == 1                              # two chunks per block
    rows, n_launches = check_plan([1 << 26])                                    # the benchmark's tensor
    assert n_launches == 4 and all(r[3] == 16 * CHUNK for r in rows if r[0] < 3)    # 3 x 320 blocks of 16 chunks, the rest in blocks of 4


def test_plan_empty_tensors_and_lists():
    assert optim.launch_plan([]) == []
    assert optim.launch_plan([0, 0]) == []
    rows, n_launches = check_plan([0, 5, 0, 0, 4097, 0])
    assert n_launches == 1 and [r[1] for r in rows] == [1, 4, 4]
    with pytest.raises(RuntimeError, match="adam_plan"):
        optim.launch_plan([-1])
    with pytest.raises(RuntimeError, match="adam_plan"):
        optim.launch_plan([(1 << 40) + 1])


def _step_args(**over):
    one = 1 << 12                                                               # never dereferenced: rejected first
    n = over.pop("n_tensors", 2)
    cnt = max(n, 1)
    ptrs = lambda: (ctypes.c_void_p * cnt)(*([one] * cnt))
    a = dict(n_tensors=n, p=ptrs(), g=ptrs(), m=ptrs(), v=ptrs(), n=(ctypes.c_int64 * cnt)(*([8] * cnt)),
             step=(ctypes.c_double * cnt)(*([1.0] * cnt)), lr=(ctypes.c_double * cnt)(*([1e-3] * cnt)),
             wd=(ctypes.c_double * cnt)(*([0.0] * cnt)), beta1=0.9, beta2=0.999, eps=1e-8, decoupled=0, grad_scale=1.0, stream=None)
    for k, val in over.items():
        if isinstance(val, tuple):                                              # (index, value): one entry of an array
            a[k][val[0]] = val[1]
        else:
            a[k] = val
    return list(a.values())


def test_adam_step_validates_before_any_device_call():
    L = _lib.lib()
    err = lambda: L.swnerf_last_error().decode()
    call = lambda **o: L.swnerf_adam_step(*_step_args(**o))
    assert call(n_tensors=0) == 0                                               # an empty list
    assert call(n_tensors=0, p=None, g=None, m=None, v=None, n=None, step=None, lr=None, wd=None) == 0
    assert call(n_tensors=-1) == -1 and "adam_step" in err()
    for name in ("p", "g", "m", "v", "n", "step", "lr", "wd"):
        assert call(**{name: None}) == -1 and "adam_step" in err() and "NULL" in err(), name
    for name in ("p", "g", "m", "v"):
        assert call(**{name: (1, None)}) == -1 and "NULL" in err() and "tensor 1" in err(), name
    assert call(n=(1, -1)) == -1 and "elements" in err()
    assert call(n=(0, (1 << 40) + 1)) == -1 and "elements" in err()
    for bad in (-1e-3, float("nan"), float("inf")):
        assert call(lr=(1, bad)) == -1 and "lr" in err(), bad
        assert call(eps=bad) == -1 and "eps" in err(), bad
        assert call(wd=(0, bad)) == -1 and "weight_decay" in err(), bad
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        assert call(beta1=bad) == -1 and "betas" in err(), bad
        assert call(beta2=bad) == -1 and "betas" in err(), bad
    assert call(step=(0, 0.0)) == -1 and "step" in err()
    assert call(grad_scale=float("inf")) == -1 and "grad_scale" in err()


def test_empty_tensors_launch_nothing_without_a_gpu():
    """n[i] == 0 for every tensor: accepted, NULL pointers included, and nothing is launched (this machine may have no GPU)."""
    L = _lib.lib()
    z = (ctypes.c_int64 * 2)(0, 0)
    assert L.swnerf_adam_step(*_step_args(n=z, p=(0, None), g=(1, None))) == 0


def test_param_group_keys_are_torchs():
    """the defaults a group is built from, read off the constructors: torch's keys and values (tests/test_gpu_optim.py compares the
    groups of two live optimizers)"""
    p = torch.nn.Parameter(torch.zeros(3))
    for ours, theirs in ((optim.Adam, torch.optim.Adam), (optim.AdamW, torch.optim.AdamW)):
        want = theirs([p]).defaults
        sig = inspect.signature(ours.__init__).parameters
        mine = {k: sig[k].default for k in want if k in sig}
        if ours is optim.AdamW:
            mine["decoupled_weight_decay"] = True                               # what AdamW passes on to Adam
        assert mine == want, (ours, mine, want)


def test_python_refusals_without_a_gpu():
    cpu = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        optim.Adam([cpu])
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        optim.AdamW([cpu])
    for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(NotImplementedError, match=flag):
            optim.Adam([cpu], **{flag: True})
    with pytest.raises(NotImplementedError, match="amsgrad"):
        optim.AdamW([cpu], amsgrad=True)
    for bad in (dict(lr=-1.), dict(eps=-1.), dict(betas=(1., .999)), dict(betas=(.9, 1.)), dict(weight_decay=-1.)):
        with pytest.raises(ValueError):
            optim.Adam([cpu], **bad)
    with pytest.raises(TypeError, match="float32"):
        optim.Adam([torch.nn.Parameter(torch.zeros(4, dtype=torch.float16))])
    with pytest.raises(TypeError, match="float32"):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))])
    opt = torch.optim.Adam([cpu])
    assert len(opt.param_groups) == 1                                           # (torch's own takes them: the refusals are ours)


def _nerf_args(**over):
    a = dict(expname="x", basedir="/nonexistent", netdepth=2, netwidth=32, netdepth_fine=2, netwidth_fine=32, lrate=5e-4, lrate_decay=500,
             netchunk=1024, no_reload=True, ft_path=None, N_samples=8, N_importance=8, perturb=1., use_viewdirs=True, i_embed=0, multires=4,
             multires_views=2, raw_noise_std=0., dataset_type="blender", white_bkgd=True, no_ndc=False, lindisp=False,
             nerf_type="direct_temporal", not_zero_canonical=False, use_two_models_for_fine=False, do_half_precision=False,
             layer_num=2, L=4)
    a.update(over)
    return SimpleNamespace(**a)


@pytest.mark.parametrize("creator", ["create_nerf", "create_dnerf", "create_tnerf", "create_multires", "create_fit2d"])
def test_unknown_optimizer_is_refused_by_every_creator(creator):
    with pytest.raises(ValueError, match=f"swnerf.{creator}: optimizer must be 'torch' or 'fused', got 'apex'"):
        getattr(runner, creator)(_nerf_args(optimizer="apex"), device="cpu")


@pytest.mark.parametrize("creator", ["create_nerf", "create_dnerf", "create_tnerf", "create_fit2d"])
def test_default_and_torch_give_torchs_optimizer(creator):
    for args in (_nerf_args(), _nerf_args(optimizer="torch")):
        opt = getattr(runner, creator)(args, device="cpu")
        opt = opt[1] if creator == "create_fit2d" else opt[4]
        assert type(opt) is (torch.optim.AdamW if creator == "create_fit2d" else torch.optim.Adam)
    with pytest.raises(RuntimeError, match="must be on the GPU"):               # the fused optimizer has no CPU path
        getattr(runner, creator)(_nerf_args(optimizer="fused"), device="cpu")
