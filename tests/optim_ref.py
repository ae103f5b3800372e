"""The yardstick of tests/test_gpu_optim.py: a float64 evaluation of the Adam / AdamW formulas (include/swnerf.h adam_step), the
seeded inputs, and a driver that walks any torch.optim.Optimizer through them.  numpy and torch on the CPU only."""
import numpy as np
import torch

# 1 .. 4099: a lone float, below / at / above a wave and a block, one chunk + 3; 70 x 5: over the tensor cap of a launch (3
# launches); the last tensor is placed 1 float into its storage by the GPU test (every other one is 16-byte aligned)
SIZES = [1, 3, 255, 256, 257, 4099] + [5] * 70 + [1027]
GROUP0 = 40                                     # tensors [0, 40) are param group 0, the rest group 1


def make_params(seed=0):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n).astype(np.float32) for n in SIZES]


def make_grads(steps, seed=1, skip=None):
    """grads[s][i]: float32 of magnitude 10^U(-8, 3) with a random sign, 5 % exact zeros; None where skip(s, i) (s counts from 1)"""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(1, steps + 1):
        row = []
        for i, n in enumerate(SIZES):
            g = (10.0 ** rng.uniform(-8, 3, n) * rng.choice([-1.0, 1.0], n) * (rng.uniform(0, 1, n) >= 0.05)).astype(np.float32)
            row.append(None if skip is not None and skip(s, i) else g)
        out.append(row)
    return out


def adam64(p, g, m, v, t, lr, betas, eps, wd, decoupled, grad_scale=1.0):
    """one step of one tensor in float64; t = the tensor's step count including this update"""
    b1, b2 = betas
    g = g.astype(np.float64) * grad_scale
    if decoupled:
        p = p * (1 - lr * wd)
    elif wd != 0:
        g = g + wd * p
    m = m + (g - m) * (1 - b1)
    v = b2 * v + (1 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps
    p = p - (lr / (1 - b1 ** t)) * m / denom
    return p, m, v


def run64(p0, grads, lrs, betas, eps, wd, decoupled, snaps, state=None):
    """-> {step: (P, M, V, T)}: concatenated float64 arrays and the per-tensor step counts.  state: (p, m, v, t) lists to go on from."""
    if state is None:
        P, M, V, T = [a.astype(np.float64) for a in p0], [np.zeros(a.shape) for a in p0], [np.zeros(a.shape) for a in p0], [0] * len(p0)
    else:
        P, M, V = ([np.asarray(a, np.float64) for a in state[k]] for k in range(3))
        T = list(state[3])
    out = {}
    for s, row in enumerate(grads, 1):
        for i, g in enumerate(row):
            if g is None:
                continue
            T[i] += 1
            P[i], M[i], V[i] = adam64(P[i], g, M[i], V[i], T[i], lrs[i], betas, eps, wd, decoupled)
        if s in snaps:
            out[s] = (np.concatenate(P), np.concatenate(M), np.concatenate(V), list(T))
    return out


def split(arr):
    """a concatenated array back into the per-tensor list"""
    return np.split(np.asarray(arr), np.cumsum(SIZES)[:-1])


def lrs_of(lr0, lr1):
    return [lr0 if i < GROUP0 else lr1 for i in range(len(SIZES))]


def groups(params, lr0, lr1):
    return [{"params": params[:GROUP0], "lr": lr0}, {"params": params[GROUP0:], "lr": lr1}]


def snapshot(opt, params):
    """(P, M, V, T) of an optimizer as float32 numpy; a parameter without state counts as m = v = 0, step 0"""
    P = np.concatenate([p.detach().cpu().numpy().reshape(-1) for p in params])
    M, V, T = [], [], []
    for p in params:
        st = opt.state.get(p, {})
        M.append(st["exp_avg"].detach().cpu().numpy().reshape(-1) if st else np.zeros(p.numel(), np.float32))
        V.append(st["exp_avg_sq"].detach().cpu().numpy().reshape(-1) if st else np.zeros(p.numel(), np.float32))
        T.append(int(st["step"]) if st else 0)
    return P, np.concatenate(M), np.concatenate(V), T


def drive(opt, params, grads, snaps, device="cpu", on_step=None):
    """grads[s][i] -> params[i].grad (None stays None), opt.step(); -> {step: snapshot}"""
    out = {}
    for s, row in enumerate(grads, 1):
        for p, g in zip(params, row):
            p.grad = None if g is None else torch.from_numpy(g).to(device)
        if on_step is not None:
            on_step(s, "before")
        opt.step()
        if on_step is not None:
            on_step(s, "after")
        if s in snaps:
            out[s] = snapshot(opt, params)
    return out


def torch_cpu(cls, p0, grads, lr0, lr1, snaps, **kw):
    """torch.optim.Adam / AdamW on the CPU in fp32 with foreach=False on the same inputs: the reference whose own distance from the
    float64 evaluation sets the gate"""
    params = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in p0]
    return drive(cls(groups(params, lr0, lr1), foreach=False, **kw), params, grads, snaps)


def dist(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def gate(ref64, d_ref):
    """max(4 x d_ref, 4 fp32 ulps of the array's largest magnitude)"""
    return max(4 * d_ref, 4 * float(np.spacing(np.float32(np.abs(ref64).max()))))
