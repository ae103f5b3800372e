"""numpy float64 restatement of the loss of a joint MultiRes iteration (multires_dnerf.py:950-996) and of its gradients, on the
restatement of the pyramid in tests/pyramid_ref.py: per level the MSE of rgb (and rgb0) against the level's target patch, the
patches reconstructed through the pyramid (r = rgb_{L-1}, r = rgb_l + up(r)), the MSE of r against the full-image patch, and
  d_rgb_l  = 2 (rgb_l - target_l) / (3 ph_l pw_l) + [add_global] (up^T)^l of 2 (r - full) / (3 ph_0 pw_0)
  d_rgb0_l = 2 (rgb0_l - target_l) / (3 ph_l pw_l).
Everything is float64; patches are [ph, pw, 3] arrays, finest level first."""
import numpy as np

import pyramid_ref as R


def loss_and_grads(rgbs, rgb0s, targets, full, add_global):
    """-> dict(loss, per_level, per_level0, global_loss, reconstructed, d_rgb, d_rgb0); rgb0s: None or a list with None entries"""
    n = len(rgbs)
    rgbs = [np.asarray(r, np.float64).reshape(np.shape(t)) for r, t in zip(rgbs, targets)]
    targets = [np.asarray(t, np.float64) for t in targets]
    rgb0s = [None] * n if rgb0s is None else [None if r is None else np.asarray(r, np.float64).reshape(t.shape) for r, t in zip(rgb0s, targets)]
    full = np.asarray(full, np.float64)
    per_level = [float(np.mean((r - t) ** 2)) for r, t in zip(rgbs, targets)]
    per_level0 = [None if r is None else float(np.mean((r - t) ** 2)) for r, t in zip(rgb0s, targets)]
    recon = R.reconstruct([r[None] for r in rgbs])[0]
    global_loss = float(np.mean((recon - full) ** 2))
    loss = sum(per_level) + sum(m for m in per_level0 if m is not None) + (global_loss if add_global else 0.0)
    d_rgb = [2.0 * (r - t) / r.size for r, t in zip(rgbs, targets)]
    d_rgb0 = [None if r is None else 2.0 * (r - t) / r.size for r, t in zip(rgb0s, targets)]
    if add_global:
        g = R.reconstruct_adjoint((2.0 * (recon - full) / recon.size)[None], [t.shape[:2] for t in targets])
        d_rgb = [d + gl[0] for d, gl in zip(d_rgb, g)]
    return dict(loss=loss, per_level=per_level, per_level0=per_level0, global_loss=global_loss, reconstructed=recon, d_rgb=d_rgb,
                d_rgb0=d_rgb0)
