"""Adam and AdamW on the fused multi-tensor HIP step (csrc/optim_kernels.hip): ONE launch per 32 tensors / 320 blocks
updates every parameter of every net of a runner, where torch's default walks the list in several launches per operation.

Both are `torch.optim.Optimizer`s: param_groups, zero_grad, add_param_group, state_dict and load_state_dict are torch's own, the
groups carry torch's keys and the per-parameter state is laid out as torch's (`step`: a float32 CPU scalar, `exp_avg` and
`exp_avg_sq`: fp32 on the parameter's device).  So a checkpoint written with either optimizer loads into the other
(swnerf.checkpoint needs to know nothing), and `lr` is read from the group at every step (runner._step_tail's decay, ExponentialLR).
The arithmetic is torch's single-tensor Adam in fp32, line by line; a parameter without a gradient is passed over with its state
untouched, so the tensors of one step may be at different step counts (the D-NeRF step at t == 0 leaves `_time.*` without one).
amsgrad, maximize, capturable and differentiable are refused; there is no CPU path.

After the launch every updated parameter is marked as modified in place (torch.autograd.graph.increment_version): the weight-pack
cache (swnerf.packing) is keyed on (data_ptr, _version) and would otherwise go on serving the weights of the step before."""
import ctypes

import torch

from . import _lib, packing

_NOT_BUILT = ("amsgrad", "maximize", "capturable", "differentiable")


def _refuse_flags(group, who):
    for flag in _NOT_BUILT:
        if group.get(flag):
            raise NotImplementedError(f"swnerf.optim.{who}: {flag} is not built (use torch.optim.{who})")


def _check_param(p, who):
    if p.dtype != torch.float32:
        raise TypeError(f"swnerf.optim.{who}: parameters must be float32, got {p.dtype}; the HIP path is fp32")
    if not p.is_cuda:
        raise RuntimeError(packing.NOT_ON_GPU)
    if not p.is_contiguous():
        raise ValueError(f"swnerf.optim.{who}: parameters must be contiguous, got shape {tuple(p.shape)} with strides {p.stride()}")


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam's arguments.  `weight_decay` is L2 (added to the gradient) unless decoupled_weight_decay, which is AdamW.
    `foreach` and `fused` are accepted and ignored: they choose among torch's implementations."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        who = type(self).__name__
        if isinstance(lr, torch.Tensor):
            raise TypeError(f"swnerf.optim.{who}: lr must be a number (a tensor lr belongs to torch's capturable path)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                        capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=decoupled_weight_decay)
        _refuse_flags(defaults, who)
        super().__init__(params, defaults)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            _refuse_flags(group, type(self).__name__)
            for p in group["params"]:
                _check_param(p, type(self).__name__)
        except Exception:
            self.param_groups.pop()
            raise

    def _collect(self):
        """-> {(device, betas, eps, decoupled): ([p], [g], [state], [lr], [wd])} over the parameters that have a gradient"""
        who = type(self).__name__
        calls = {}
        for group in self.param_groups:
            _refuse_flags(group, who)                                # load_state_dict replaces the groups' entries wholesale
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                _check_param(p, who)
                if g.is_sparse or g.layout != torch.strided:
                    raise RuntimeError(f"swnerf.optim.{who}: sparse gradients are not built (torch.optim.SparseAdam)")
                if g.is_complex() or g.dtype != torch.float32 or g.device != p.device:
                    raise TypeError(f"swnerf.optim.{who}: the gradient of a float32 parameter on {p.device} is {g.dtype} on {g.device}")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                elif state["step"].is_cuda:                          # a state written by torch's fused / capturable path
                    state["step"] = state["step"].detach().float().cpu()
                b1, b2 = group["betas"]
                key = (p.device, float(b1), float(b2), float(group["eps"]), bool(group["decoupled_weight_decay"]))
                c = calls.setdefault(key, ([], [], [], [], []))
                c[0].append(p)
                c[1].append(g if g.is_contiguous() else g.contiguous())
                c[2].append(state)
                c[3].append(float(group["lr"]))
                c[4].append(float(group["weight_decay"]))
        return calls

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        """One update of every parameter that has a gradient.  grad_scale multiplies every gradient as it is read (a data-parallel
        caller's 1 / world); 1.0 multiplies by exactly 1."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = None
        for (device, b1, b2, eps, decoupled), (ps, gs, states, lrs, wds) in self._collect().items():
            L = L or _lib.lib()
            n = len(ps)
            ms, vs = [s["exp_avg"] for s in states], [s["exp_avg_sq"] for s in states]
            for m, v, p in zip(ms, vs, ps):
                if not (m.is_contiguous() and v.is_contiguous() and m.dtype == v.dtype == torch.float32 and m.device == v.device == device
                        and m.numel() == v.numel() == p.numel()):
                    raise RuntimeError(f"swnerf.optim.{type(self).__name__}: exp_avg / exp_avg_sq of a parameter of shape {tuple(p.shape)} "
                                       "are not float32, contiguous and on its device (a state_dict of another model?)")
            steps = [s["step"] for s in states]
            torch._foreach_add_(steps, 1.0)
            ptrs = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
            dbl = lambda xs: (ctypes.c_double * n)(*xs)
            with torch.cuda.device(device):
                _lib.check(L.swnerf_adam_step(n, ptrs(ps), ptrs(gs), ptrs(ms), ptrs(vs), (ctypes.c_int64 * n)(*[p.numel() for p in ps]),
                                              dbl(torch.stack(steps).tolist()), dbl(lrs), dbl(wds), b1, b2, eps, int(decoupled),
                                              float(grad_scale), _lib.stream_of(ps[0])), "adam_step")
            torch.autograd.graph.increment_version(ps)
        return loss


class AdamW(Adam):
    """torch.optim.AdamW's arguments: Adam with decoupled weight decay, p <- p (1 - lr wd) before the update."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False, foreach=None,
                 capturable=False, differentiable=False, fused=None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize, capturable=capturable,
                         differentiable=differentiable, fused=fused, decoupled_weight_decay=True)


def launch_plan(sizes):
    """The cut of a list of tensor sizes into launches, as swnerf_adam_step makes it: one row (launch, tensor, start, count) per
    block.  Host only."""
    L = _lib.lib()
    n = len(sizes)
    arr = (ctypes.c_int64 * max(n, 1))(*sizes)
    rows = L.swnerf_adam_plan(n, arr, 0, None, None, None, None)
    if rows < 0:
        _lib.check(int(rows), "adam_plan")
    la, te = (ctypes.c_int32 * max(rows, 1))(), (ctypes.c_int32 * max(rows, 1))()
    st, co = (ctypes.c_int64 * max(rows, 1))(), (ctypes.c_int64 * max(rows, 1))()
    _lib.check(min(int(L.swnerf_adam_plan(n, arr, rows, la, te, st, co)), 0), "adam_plan")
    return [(la[r], te[r], st[r], co[r]) for r in range(rows)]


def caps():
    """-> (tensors per launch, blocks per launch, elements per chunk, bytes of the kernel argument)"""
    t, b, c, d = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_size_t()
    _lib.lib().swnerf_adam_caps(ctypes.byref(t), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d))
    return t.value, b.value, c.value, d.value
