"""tests/dnerf_ref.py can tell a right D-NeRF gradient from a wrong one (no GPU): the fp32 CPU oracle plays the kernel
(O.run_network_dnerf + O.raw2outputs under autograd, dx_value = its own dx).  It must pass the check at 2e-5, and each of
four corruptions of its gradients - of the size the fp32-oracle comparisons of test_gpu_backward.py let through - must fail."""
import numpy as np
import pytest
import torch

import cases
import dnerf_ref
from oracle import nerf_oracle as O

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
TV_W, DX_W = 0.1, 0.05


def _case(n, S, t, tv=False, noise_std=0.0, white=True, with_dx=True):
    """inputs + the oracle's gradients of: image MSE + a linear term on dx (+ TV between t and t - 0.05 on the same depths)"""
    sd_np = cases.weights_dnerf()
    g = cases.g8_inputs(n=n)
    rb = O.make_ray_batch(T(g["rays_o"]), T(g["rays_d"]), 2., 6., frame_time=t)
    z = O.coarse_z(rb[:, 6:7], rb[:, 7:8], S).contiguous()
    rng = np.random.default_rng(31 + n)
    tgt = T(rng.uniform(0, 1, (n, 3)).astype(np.float32))
    gdx = T(rng.standard_normal((n, S, 3)).astype(np.float32))
    noise = T((rng.standard_normal((n, S)) * noise_std).astype(np.float32)) if noise_std > 0 else None
    t2 = t - 0.05

    def ray_loss(ret, idx, with_dx=with_dx):
        c = lambda a: a[idx].to(ret["raw"])
        L = ((ret["rgb_map"] - c(tgt)) ** 2).sum() / (3 * n)
        if with_dx:
            L = L + DX_W * (ret["position_delta"] * c(gdx)).sum() / n
        if tv:
            L = L + TV_W * (ret["position_delta"] - ret["position_delta_2"]).pow(2).sum()
        return L

    def oracle(loss=ray_loss):
        sd = {k: v.clone().requires_grad_(True) for k, v in O.to_torch_sd(sd_np).items()}
        pts = rb[:, None, 0:3] + rb[:, None, 3:6] * z[..., None]
        raw, dx = O.run_network_dnerf(sd, pts, rb[:, -3:], rb[:, 8:9])
        rgb, disp, acc, _, _ = O.raw2outputs(raw, z, rb[:, 3:6], 0., white, noise=noise)
        ret = {"rgb_map": rgb, "disp_map": disp, "acc_map": acc, "raw": raw, "position_delta": dx}
        if tv:
            ret["position_delta_2"] = O.run_network_dnerf(sd, pts, rb[:, -3:], torch.full((n, 1), t2))[1]
        loss(ret, torch.arange(n)).backward()
        return {k: v.grad for k, v in sd.items()}, dx.detach()

    kw = dict(second=(t2, z) if tv else None, noise=noise)
    return sd_np, rb, z, white, ray_loss, oracle, kw


def _run(case, grads, dxv, what):
    sd_np, rb, z, white, ray_loss, _, kw = case
    stats = {}
    fl = dnerf_ref.flip_aware_check(sd_np, rb, z, white, ray_loss, grads, what, dxv, stats=stats, **kw)
    return fl, stats["worst"]


@pytest.mark.parametrize("n,S,t,tv,noise_std", [(12, 24, 0.5, False, 0.), (40, 64, 0.5, False, 0.), (5, 33, 0.0, False, 0.),
                                                (3, 2, 0.25, False, 0.), (12, 24, 0.5, True, 0.), (7, 17, 0.75, False, 0.7)])
def test_oracle_passes_at_2e_5(n, S, t, tv, noise_std):
    case = _case(n, S, t, tv, noise_std, white=(noise_std == 0.))
    grads, dxv = case[5]()
    sd_np, rb, z = case[:3]
    if t == 0.0:
        assert all(grads[k] is None for k in grads if k.startswith("_time")) and float(dxv.abs().max()) == 0.0
    else:
        ex, et, _, _ = dnerf_ref.ray_encodings(rb, z)
        ddx = float((dxv.reshape(-1, 3).double() - dnerf_ref.float64_dx(sd_np, ex, et)).abs().max())
        print(f"\n[parity] fp32 oracle dx vs float64 dx: max |difference| {ddx:.2e}")
        assert ddx < 1e-6
    (flips, risky), worst = _run(case, grads, dxv, f"oracle {n}x{S} t={t}")
    print(f"\n[parity] fp32 oracle as the kernel, {n} x {S} t={t} tv={tv} noise={noise_std}: {flips} flips of {risky} risky units, "
          f"worst residual {worst:.2e} of its tensor's max (gate 2e-5)")


@pytest.fixture(scope="module")
def small():
    case = _case(12, 24, 0.5)
    grads, dxv = case[5]()
    _run(case, grads, dxv, "clean")                      # the uncorrupted gradients pass
    return case, grads, dxv


def test_rejects_scaled_time_out(small):
    case, grads, dxv = small
    bad = dict(grads)
    bad["_time_out.weight"] = grads["_time_out.weight"] * (1 + 2e-4)
    with pytest.raises(AssertionError):
        _run(case, bad, dxv, "scaled _time_out")


def test_rejects_rolled_time_columns(small):
    case, grads, dxv = small
    bad = dict(grads)
    w = grads["_time.0.weight"].clone()
    w[:, 63:84] = torch.roll(w[:, 63:84], 1, dims=1)
    bad["_time.0.weight"] = w
    with pytest.raises(AssertionError):
        _run(case, bad, dxv, "gamma(t) columns rolled")


def test_rejects_dropped_position_delta_term(small):
    case, grads, dxv = small
    bad, _ = case[5](lambda ret, idx: case[4](ret, idx, with_dx=False))
    with pytest.raises(AssertionError):
        _run(case, bad, dxv, "position_delta term dropped")


def test_rejects_jacobian_without_lowest_band(small):
    """d(x+dx) = J_gamma^T d gamma without the sin / cos columns of frequency 2^0: the truth's own graph with that band detached"""
    case, grads, dxv = small
    sd_np, rb, z, white, ray_loss, _, kw = case
    names = list(grads)
    Tr = dnerf_ref.ray_truth(sd_np, names, rb, z, white, ray_loss, dxv, detach_bands=(0,), **kw)
    bad = Tr.named(Tr.grads(torch.arange(rb.shape[0])))
    whole = dnerf_ref.ray_truth(sd_np, names, rb, z, white, ray_loss, dxv, **kw)
    _run(case, whole.named(whole.grads(torch.arange(rb.shape[0]))), dxv, "the truth's own gradient")       # the same graph, band kept: passes
    with pytest.raises(AssertionError):
        _run(case, bad, dxv, "J_gamma without its lowest band")
