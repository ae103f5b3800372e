"""The data side of a training step (nerf/run.py:598-696, d_nerf/run_dnerf.py:648-683) on the device: a ray batch is drawn,
computed, packed and paired with its target pixels by ONE kernel launch (csrc/batch_kernels.hip, swnerf_train_batch), and the
photometric loss with its gradient by one more (swnerf_photo_loss).  Nothing of the size of an image is written per step, and
`use_batching` keeps no table of rays: a batch is the image of a run of consecutive integers under a keyed permutation of the
pixel ids, and an epoch is that permutation walked from 0 to its end.  DESIGN.md 6i.

The joint iteration of the MultiRes runner has the same two launches (csrc/patch_kernels.hip): `PatchBatcher` makes
every level's patch rows and targets, `multires_loss` the per-level losses, the reconstruction, the global loss and the gradients;
`key_randint` / `key_normal` / `patch_corner(s)` are its host-side keyed draws.

`perm_index_np` defines the permutation; the device function must equal it bit for bit (tests/test_gpu_batching.py)."""
import ctypes

import numpy as np
import torch

from . import _lib

PERM_ROUNDS = 6
PERM_MAX_N = 1 << 40
_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


def mix64(z):
    """The splitmix64 finaliser on a Python int (mod 2^64)."""
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _hash32(x):
    """The round function's 32-bit integer hash on a uint64 array holding values below 2^32."""
    m = np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & m
    return x ^ (x >> np.uint64(16))


def perm_half_bits(n):
    hb = 1
    while (1 << (2 * hb)) < n:
        hb += 1
    return hb


def perm_index_np(key, n, k):
    """perm(key, n, k): a bijection of [0, n) for any 1 <= n < 2^40 and any 64-bit key, elementwise over the integer array k.
    A balanced Feistel network on 2 * hb bits (the smallest even width with 2^(2 hb) >= n), PERM_ROUNDS rounds, round function
    hash32(half ^ round key) with round key r = the high word of mix64(key + (r + 1) * golden); a result outside [0, n) is
    sent through the network again (cycle walking) - the network is a bijection of [0, 2^(2 hb)), so the walk from a point of
    [0, n) is back in [0, n) after at most 2^(2 hb) - n + 1 applications."""
    n = int(n)
    if not 1 <= n < PERM_MAX_N:
        raise ValueError(f"swnerf.batching.perm_index_np: n {n} outside 1 .. 2^40 - 1")
    k = np.asarray(k, dtype=np.int64)
    if k.size and (k.min() < 0 or k.max() >= n):
        raise ValueError("swnerf.batching.perm_index_np: k outside [0, n)")
    key = int(key) & _M64
    hb = perm_half_bits(n)
    rk = [np.uint64(mix64(key + (r + 1) * _GOLDEN) >> 32) for r in range(PERM_ROUNDS)]
    mask, sh = np.uint64((1 << hb) - 1), np.uint64(hb)
    x = k.astype(np.uint64).reshape(-1).copy()
    todo = np.ones(x.shape, bool)
    for _ in range((1 << (2 * hb)) - n + 1):
        if not todo.any():
            break
        v = x[todo]
        l, r = (v >> sh) & mask, v & mask
        for i in range(PERM_ROUNDS):
            l, r = r, l ^ (_hash32(r ^ rk[i]) & mask)
        v = (l << sh) | r
        x[todo] = v
        todo[todo] = v >= np.uint64(n)
    assert not todo.any()
    return x.astype(np.int64).reshape(k.shape)


def batch_key(seed, counter, stream=0):
    """The 64-bit key of draw `counter` (a step or an epoch) of the sampler seeded with `seed`; `stream` separates the
    per-image draws (0) from the epochs of use_batching (1)."""
    return mix64(mix64((int(seed) & _M64) ^ ((int(stream) & 0xFF) << 56)) + (int(counter) & _M64) * _GOLDEN)


def perm_indices(key, n, k0, count, device=None):
    """perm(key, n, k0 .. k0 + count) on the device -> int64 [count]."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    out = torch.empty((int(count),), dtype=torch.int64, device=dev)
    _lib.check(_lib.lib().swnerf_perm_indices(int(key) & _M64, int(n), int(k0), int(count), _lib.ptr(out), _lib.stream_of(out)), "perm_indices")
    return out


def precrop_window(H, W, frac):
    """nerf/run.py:663-664 -> (dH, dW): the central crop is rows H//2 - dH .. H//2 + dH - 1, columns W//2 - dW .. W//2 + dW - 1."""
    return int(H // 2 * frac), int(W // 2 * frac)


def precrop_crop(H, W, frac):
    """The crop window (y0, x0, h, w) of precrop_window, as image_batch takes it."""
    dH, dW = precrop_window(H, W, frac)
    return H // 2 - dH, W // 2 - dW, 2 * dH, 2 * dW


def time_curriculum_max(i, precrop_iters_time, n_train):
    """d_nerf/run_dnerf.py:650-655: at iteration i < precrop_iters_time the frame is drawn from i_train[:max_sample]; None
    once the curriculum is over."""
    if i >= precrop_iters_time:
        return None
    return max(int(i / float(precrop_iters_time) * n_train), 3)


def lr_at(lrate, lrate_decay, global_step):
    """nerf/run.py:704-706."""
    return lrate * (0.1 ** (global_step / (lrate_decay * 1000)))


class EpochCursor:
    """The cursor of use_batching (nerf/run.py:641-650) over `domain` rays: next(n_rand) -> (epoch, k0, n).  The last batch
    of an epoch is short; the call after it starts the next epoch at 0."""

    def __init__(self, domain):
        self.domain, self.cursor, self.epoch = int(domain), 0, 0

    def next(self, n_rand):
        k0, n, epoch = self.cursor, min(int(n_rand), self.domain - self.cursor), self.epoch
        self.cursor += int(n_rand)
        if self.cursor >= self.domain:
            self.cursor, self.epoch = 0, self.epoch + 1
        return epoch, k0, n


class RayBatcher:
    """Training batches of a set of posed images, made on the device.

    images [N,H,W,3|4] float32 or uint8 (numpy or tensor) stay on the device AS GIVEN (uint8 RGBA: 256 MB for 100 frames of
    800 x 800); a byte converts as the loaders do, (float)((double)u / 255.), and with 4 channels and white_bkgd the target is
    c * a + (1 - a) (nerf/run.py:469-472), per drawn pixel.  poses [N,>=3,4] and times [N] (D-NeRF: rows get 12 columns) are
    device tables.  hwf_or_K: [H, W, focal] (the focal branch of get_rays) or a 3 x 3 K.  Rows are those of
    render.pack_ray_batch: 11 columns, 8 without use_viewdirs, 12 with times."""

    def __init__(self, images, poses, hwf_or_K, i_train, near, far, times=None, ndc=False, use_viewdirs=True, white_bkgd=False,
                 seed=0, device=None):
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise RuntimeError(f"swnerf.batching.RayBatcher: batches are made on the GPU (got device {dev}); there is no CPU path")
        images = torch.as_tensor(images)
        if images.dim() != 4 or images.shape[-1] not in (3, 4) or images.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"swnerf.batching.RayBatcher: images must be [N,H,W,3|4] float32 or uint8, got {tuple(images.shape)} {images.dtype}")
        self.images = images.to(dev).contiguous()
        self.n_images, self.H, self.W, self.channels = (int(s) for s in images.shape)
        poses = torch.as_tensor(np.asarray(poses.cpu() if isinstance(poses, torch.Tensor) else poses, dtype=np.float32))
        if poses.dim() != 3 or poses.shape[0] != self.n_images or poses.shape[1] < 3 or poses.shape[2] != 4:
            raise ValueError(f"swnerf.batching.RayBatcher: poses must be [{self.n_images},>=3,4], got {tuple(poses.shape)}")
        self.c2w = poses[:, :3, :4].contiguous().to(dev)
        self.times, self.times_host = None, None
        if times is not None:
            self.times_host = np.asarray(times.cpu() if isinstance(times, torch.Tensor) else times, dtype=np.float32).reshape(-1)
            if self.times_host.shape[0] != self.n_images:
                raise ValueError(f"swnerf.batching.RayBatcher: times must have {self.n_images} entries, got {self.times_host.shape[0]}")
            if not use_viewdirs:
                raise ValueError("swnerf.batching.RayBatcher: rows with a frame time carry the view directions (12 columns); use_viewdirs=False is not built")
            self.times = torch.from_numpy(self.times_host.copy()).to(dev)
        k = np.asarray(hwf_or_K, dtype=np.float64)
        if k.ndim == 1 and k.shape[0] == 3:
            if (int(k[0]), int(k[1])) != (self.H, self.W):
                raise ValueError(f"swnerf.batching.RayBatcher: hwf says {int(k[0])} x {int(k[1])}, the images are {self.H} x {self.W}")
            self.intr = (float(k[2]), float(k[2]), self.W * 0.5, self.H * 0.5, 1)
        elif k.shape == (3, 3):
            self.intr = (float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2]), 0)
        else:
            raise ValueError("swnerf.batching.RayBatcher: hwf_or_K must be [H, W, focal] or a 3 x 3 K")
        self.i_train_host = np.asarray(i_train, dtype=np.int64).reshape(-1)
        if self.i_train_host.size < 1 or self.i_train_host.min() < 0 or self.i_train_host.max() >= self.n_images:
            raise ValueError(f"swnerf.batching.RayBatcher: i_train must be a non-empty list of indices into the {self.n_images} images")
        self.i_train = torch.from_numpy(self.i_train_host.copy()).to(dev)
        self.all_images = torch.arange(self.n_images, dtype=torch.int64, device=dev)      # image_batch: a one-entry list is a view of this
        self.near, self.far, self.ndc, self.white_bkgd, self.seed = float(near), float(far), bool(ndc), bool(white_bkgd), int(seed)
        self.cols = 12 if times is not None else (11 if use_viewdirs else 8)
        self.device = dev
        self.cursor = EpochCursor(self.i_train_host.size * self.H * self.W)

    def _launch(self, i_train_ptr, n_train, crop, key, k0, n, ids, want_ids):
        y0, x0, h, w = (0, 0, self.H, self.W) if crop is None else (int(c) for c in crop)
        rb = torch.empty((n, self.cols), dtype=torch.float32, device=self.device)
        target = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        ids_out = torch.empty((n,), dtype=torch.int64, device=self.device) if want_ids else None
        fx, fy, cx, cy, fb = self.intr
        _lib.check(_lib.lib().swnerf_train_batch(
            _lib.ptr(self.images), int(self.images.dtype == torch.uint8), self.channels, self.n_images, self.H, self.W,
            _lib.ptr(self.c2w), _lib.ptr(self.times), i_train_ptr, n_train, y0, x0, h, w, fx, fy, cx, cy, fb,
            self.near, self.far, self.cols, int(self.ndc), fx, int(self.white_bkgd), int(key) & _M64, int(k0), int(n),
            _lib.ptr(ids), _lib.ptr(rb), _lib.ptr(target), _lib.ptr(ids_out), _lib.stream_of(rb)), "train_batch")
        return (rb, target, ids_out) if want_ids else (rb, target)

    def image_batch(self, img_i, n_rand, step, crop=None, ids=None, return_ids=False):
        """The `no_batching` draw (nerf/run.py:652-681): n_rand distinct pixels of image img_i inside `crop` = (y0, x0, h, w)
        (None: the whole image), keyed by (seed, step) -> (ray_batch [n_rand, cols], target [n_rand, 3]).  `ids`: explicit
        row-major indices into the window (an int64 array; what np.random.choice(h * w, ...) returns) instead of the draw."""
        img_i = int(img_i)
        if not 0 <= img_i < self.n_images:
            raise ValueError(f"swnerf.batching.RayBatcher.image_batch: image {img_i} of {self.n_images}")
        if ids is not None:
            ids = torch.as_tensor(np.asarray(ids, dtype=np.int64) if not isinstance(ids, torch.Tensor) else ids).to(self.device, torch.int64).contiguous().reshape(-1)
            n_rand = ids.shape[0]
        one = ctypes.c_void_p(self.all_images.data_ptr() + 8 * img_i)
        return self._launch(one, 1, crop, batch_key(self.seed, step, 0), 0, int(n_rand), ids, return_ids)

    def global_batch(self, n_rand, return_ids=False):
        """The `use_batching` draw (nerf/run.py:639-650) over all rays of the training images: the next n_rand entries of this
        epoch's permutation.  The last batch of an epoch is short, the next call starts a new epoch with a new key.  An id is
        (slot in i_train) * H * W + y * W + x."""
        epoch, k0, n = self.cursor.next(n_rand)
        return self._launch(_lib.ptr(self.i_train), self.i_train_host.size, None, batch_key(self.seed, epoch, 1), k0, n, None, return_ids)

    def with_time(self, ray_batch, t):
        """A copy of a 12-column batch at frame time t (a float or a 0-d tensor): the TV-loss renders of run_dnerf.py:700-710."""
        if ray_batch.shape[-1] != 12:
            raise ValueError("swnerf.batching.RayBatcher.with_time: the batch has no frame-time column")
        out = ray_batch.clone()
        out[:, 8] = t
        return out


class _PhotoLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb, target, rgb0):
        N = rgb.shape[0]
        sums = torch.empty((2,), dtype=torch.float64, device=rgb.device)
        losses = torch.empty((3,), dtype=torch.float32, device=rgb.device)
        d_rgb = torch.empty_like(rgb)
        d_rgb0 = torch.empty_like(rgb0) if rgb0 is not None else None
        _lib.check(_lib.lib().swnerf_photo_loss(_lib.ptr(rgb), _lib.ptr(rgb0), _lib.ptr(target), N, _lib.ptr(sums), _lib.ptr(losses),
                                                _lib.ptr(d_rgb), _lib.ptr(d_rgb0), _lib.stream_of(rgb)), "photo_loss")
        ctx.save_for_backward(d_rgb, d_rgb0 if d_rgb0 is not None else torch.empty(0, device=rgb.device))
        ctx.has0 = rgb0 is not None
        ctx.mark_non_differentiable(sums)
        ctx.set_materialize_grads(False)
        return losses[0], losses[1], losses[2], sums

    @staticmethod
    def backward(ctx, g_loss, g_img, g_img0, _):
        d_rgb, d_rgb0 = ctx.saved_tensors
        both = lambda a, b: a if b is None else (b if a is None else a + b)
        ga, gb = both(g_loss, g_img), both(g_loss, g_img0)
        return (None if ga is None else d_rgb * ga, None,
                None if (gb is None or not ctx.has0) else d_rgb0 * gb)


def photometric_loss(rgb, target, rgb0=None):
    """img2mse(rgb, target) [+ img2mse(rgb0, target)] (nerf/run.py:689-696) and its gradient in one launch ->
    (loss, img_loss, img_loss0); img_loss0 is None without rgb0.  The sums are fp64 in a fixed order: equal bits on every run."""
    rgb, target = _lib.dev_f32(rgb, "rgb", 3), _lib.dev_f32(target, "target", 3)
    if rgb0 is not None:
        rgb0 = _lib.dev_f32(rgb0, "rgb0", 3)
    if rgb.dim() != 2 or rgb.shape != target.shape or (rgb0 is not None and rgb0.shape != rgb.shape) or rgb.shape[0] < 1:
        raise ValueError(f"swnerf.batching.photometric_loss: rgb, rgb0 and target must all be [N >= 1, 3], got {tuple(rgb.shape)} / {tuple(target.shape)}")
    loss, img_loss, img_loss0, _ = _PhotoLoss.apply(rgb, target.detach(), rgb0)
    return loss, img_loss, (img_loss0 if rgb0 is not None else None)


# ---- the joint iteration of the MultiRes D-NeRF runner (multires_dnerf.py:905-996; csrc/patch_kernels.hip) ------
PATCH_MAX_LEVELS = _lib.PATCH_MAX_LEVELS
PATCH_MAX_SIDE = _lib.PATCH_MAX_SIDE


def key_word(key, j):
    """Word j of the stream of a 64-bit key (batch_key): mix64(key + (j + 1) * golden), the construction of perm_index_np's round keys."""
    return mix64((int(key) & _M64) + (int(j) + 1) * _GOLDEN)


def key_uniform(key, j):
    """A float64 in [0, 1): the top 53 bits of word j."""
    return (key_word(key, j) >> 11) * (1.0 / (1 << 53))


def key_randint(key, j, lo, hi):
    """An integer in [lo, hi], both ends included as in random.randint: lo + word j mod (hi - lo + 1).  The modulo bias is below
    (hi - lo + 1) / 2^64."""
    lo, hi = int(lo), int(hi)
    if hi < lo:
        raise ValueError(f"swnerf.batching.key_randint: empty range [{lo}, {hi}]")
    return lo + key_word(key, j) % (hi - lo + 1)


def key_normal(key, j, mean, std):
    """A normal draw (Box-Muller on words j and j + 1): mean + std * sqrt(-2 ln(1 - u1)) * cos(2 pi u2), float64."""
    u1, u2 = key_uniform(key, j), key_uniform(key, j + 1)
    return float(mean) + float(std) * float(np.sqrt(-2.0 * np.log1p(-u1)) * np.cos(2.0 * np.pi * u2))


def patch_corner(key, H, W, patch_size, current_iter, n=4000, sigma_factor=4):
    """runner.get_random_patch_coords (multires_dnerf.py:500-561) as a pure function of `key`: before iteration n uniform over the
    central region (key_randint on words 0 and 1), from then on normal around the centre (key_normal on words 0..1 and 2..3) and
    clipped into the image.  An image that is not larger than the patch gives (0, 0)."""
    if H <= patch_size or W <= patch_size:
        return 0, 0
    center_y = (H - patch_size) / 2
    center_x = (W - patch_size) / 2
    if current_iter < n:
        min_y = max(0, int(center_y - H / 4 / 2))
        max_y = min(int(center_y + H / 4 / 2), H - patch_size)
        min_x = max(0, int(center_x - W / 4 / 2))
        max_x = min(int(center_x + W / 4 / 2), W - patch_size)
        return key_randint(key, 0, min_y, max_y), key_randint(key, 1, min_x, max_x)
    y = int(key_normal(key, 0, center_y, H / sigma_factor))
    x = int(key_normal(key, 2, center_x, W / sigma_factor))
    return max(0, min(y, H - patch_size)), max(0, min(x, W - patch_size))


def patch_corners(key, pyr_hwf, base_patch_size=4, cur_iter=0):
    """runner.initialize_patches (multires_dnerf.py:562-585) on patch_corner: one (y, x) per level, finest first - drawn at the
    coarsest level and doubled level by level."""
    H, W = int(pyr_hwf[-1][0]), int(pyr_hwf[-1][1])
    y, x = patch_corner(key, H, W, base_patch_size, cur_iter)
    n = len(pyr_hwf)
    return [(y << (n - 1 - l), x << (n - 1 - l)) for l in range(n)]


def clipped_patch_sizes(pyr_hwf, patch_coords, patch_size_list):
    """(ph, pw) per level of the slice target[y:y + ps, x:x + ps] the reference takes (multires_dnerf.py:932): the patch clipped to
    the level, ph = min(ps, H - y), pw = min(ps, W - x)."""
    if not (len(pyr_hwf) == len(patch_coords) == len(patch_size_list)):
        raise ValueError(f"swnerf.batching.clipped_patch_sizes: {len(pyr_hwf)} levels, {len(patch_coords)} corners, {len(patch_size_list)} patch sizes")
    out = []
    for l, ((H, W, _), (y, x), ps) in enumerate(zip(pyr_hwf, patch_coords, patch_size_list)):
        H, W, y, x, ps = int(H), int(W), int(y), int(x), int(ps)
        if ps < 1 or not (0 <= y < H and 0 <= x < W):
            raise ValueError(f"swnerf.batching.clipped_patch_sizes: level {l}: patch {ps} at ({y}, {x}) of a {H} x {W} image")
        out.append((min(ps, H - y), min(ps, W - x)))
    return out


def _int_array(values):
    return (ctypes.c_int * len(values))(*[int(v) for v in values])


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


class PatchBatcher:
    """The data of a joint MultiRes iteration, made on the device by ONE launch (swnerf_patch_batch) for all levels.

    images [N,H,W,3] float32 (the full-resolution frames), pyr_images: per level [N,H_l,W_l,3] float32 as
    pyramid.generate_laplacian_pyramid_batch returns them, poses [N,>=3,4], times [N], pyr_hwf: [H_l, W_l, focal_l] per level
    (runner.pyramid_hwf), at most PATCH_MAX_LEVELS levels.  Everything lives on the GPU; there is no CPU path."""

    def __init__(self, images, pyr_images, poses, times, pyr_hwf, near, far, device=None):
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise RuntimeError(f"swnerf.batching.PatchBatcher: batches are made on the GPU (got device {dev}); there is no CPU path")
        self.pyr_hwf = [(int(H), int(W), float(f)) for H, W, f in pyr_hwf]
        n_levels = len(self.pyr_hwf)
        if not 1 <= n_levels <= PATCH_MAX_LEVELS or len(pyr_images) != n_levels:
            raise ValueError(f"swnerf.batching.PatchBatcher: {n_levels} levels in pyr_hwf (1..{PATCH_MAX_LEVELS} are built), {len(pyr_images)} in pyr_images")
        images = torch.as_tensor(images)
        if images.dim() != 4 or images.shape[-1] != 3 or images.dtype != torch.float32:
            raise ValueError(f"swnerf.batching.PatchBatcher: images must be [N,H,W,3] float32, got {tuple(images.shape)} {images.dtype}")
        self.n_images = int(images.shape[0])
        if tuple(images.shape[1:3]) != self.pyr_hwf[0][:2]:
            raise ValueError(f"swnerf.batching.PatchBatcher: images are {tuple(images.shape[1:3])}, level 0 of pyr_hwf is {self.pyr_hwf[0][:2]}")
        self.images = images.to(dev).contiguous()
        self.pyr_images = []
        for l, (p, (H, W, _)) in enumerate(zip(pyr_images, self.pyr_hwf)):
            p = torch.as_tensor(p)
            if tuple(p.shape) != (self.n_images, H, W, 3) or p.dtype != torch.float32:
                raise ValueError(f"swnerf.batching.PatchBatcher: pyr_images[{l}] must be {(self.n_images, H, W, 3)} float32, got {tuple(p.shape)} {p.dtype}")
            self.pyr_images.append(p.to(dev).contiguous())
        poses = torch.as_tensor(np.asarray(poses.cpu() if isinstance(poses, torch.Tensor) else poses, dtype=np.float32))
        if poses.dim() != 3 or poses.shape[0] != self.n_images or poses.shape[1] < 3 or poses.shape[2] != 4:
            raise ValueError(f"swnerf.batching.PatchBatcher: poses must be [{self.n_images},>=3,4], got {tuple(poses.shape)}")
        self.c2w = poses[:, :3, :4].contiguous().to(dev)
        self.times_host = np.asarray(times.cpu() if isinstance(times, torch.Tensor) else times, dtype=np.float32).reshape(-1)
        if self.times_host.shape[0] != self.n_images:
            raise ValueError(f"swnerf.batching.PatchBatcher: times must have {self.n_images} entries, got {self.times_host.shape[0]}")
        self.times = torch.from_numpy(self.times_host.copy()).to(dev)
        self.near, self.far, self.device = float(near), float(far), dev
        self._pyr_ptrs = _ptr_array(self.pyr_images)
        self._level_hw = _int_array([v for H, W, _ in self.pyr_hwf for v in (H, W)])
        self._focal = (ctypes.c_double * n_levels)(*[f for _, _, f in self.pyr_hwf])

    def batch(self, img_i, patch_coords, patch_size_list):
        """-> (ray_batches, target_patches, full_patch): per level the packed rows [ph_l * pw_l, 12] of the patch with corner
        patch_coords[l] = (y, x) and side patch_size_list[l], clipped to the level (clipped_patch_sizes), and that patch of
        pyr_images[l] [ph_l, pw_l, 3]; full_patch [ph_0, pw_0, 3] is the level-0 patch of images."""
        img_i = int(img_i)
        if not 0 <= img_i < self.n_images:
            raise ValueError(f"swnerf.batching.PatchBatcher.batch: image {img_i} of {self.n_images}")
        sizes = clipped_patch_sizes(self.pyr_hwf, patch_coords, patch_size_list)
        rows = [torch.empty((ph * pw, 12), dtype=torch.float32, device=self.device) for ph, pw in sizes]
        targets = [torch.empty((ph, pw, 3), dtype=torch.float32, device=self.device) for ph, pw in sizes]
        full = torch.empty((sizes[0][0], sizes[0][1], 3), dtype=torch.float32, device=self.device)
        _lib.check(_lib.lib().swnerf_patch_batch(
            len(sizes), self._pyr_ptrs, self._level_hw, self._focal, _int_array([v for yx in patch_coords for v in yx]),
            _int_array(patch_size_list), _lib.ptr(self.images), self.n_images, _lib.ptr(self.c2w), _lib.ptr(self.times), img_i,
            self.near, self.far, _ptr_array(rows), _ptr_array(targets), _lib.ptr(full), _lib.stream_of(full)), "patch_batch")
        return rows, targets, full


class _MultiresLoss(torch.autograd.Function):
    """forward(add_global, n_levels, full_patch, *targets, *rgbs, *rgb0s) -> (loss, losses, reconstructed); the forward computes the
    gradients of `loss`, the backward scales them.  losses and reconstructed carry no gradient."""

    @staticmethod
    def forward(ctx, add_global, n, full, *ts):
        targets, rgbs, rgb0s = ts[:n], ts[n:2 * n], ts[2 * n:]
        dev = full.device
        losses = torch.empty((_lib.MULTIRES_LOSSES,), dtype=torch.float32, device=dev)
        recon = torch.empty_like(full)
        d_rgb = [torch.empty_like(r) for r in rgbs]
        d_rgb0 = [None if r is None else torch.empty_like(r) for r in rgb0s]
        _lib.check(_lib.lib().swnerf_multires_loss(
            n, _int_array([v for t in targets for v in t.shape[:2]]), _ptr_array(rgbs), _ptr_array(rgb0s), _ptr_array(targets),
            _lib.ptr(full), int(bool(add_global)), _lib.ptr(losses), _lib.ptr(recon), _ptr_array(d_rgb), _ptr_array(d_rgb0),
            _lib.stream_of(full)), "multires_loss")
        ctx.n, ctx.has0 = n, [r is not None for r in rgb0s]
        ctx.save_for_backward(*d_rgb, *[d for d in d_rgb0 if d is not None])
        ctx.mark_non_differentiable(losses, recon)
        return losses[0], losses, recon

    @staticmethod
    def backward(ctx, g_loss, _g_losses, _g_recon):
        n, saved = ctx.n, list(ctx.saved_tensors)
        d_rgb, rest = saved[:n], saved[n:]
        d_rgb0 = [rest.pop(0) if has else None for has in ctx.has0]
        return (None, None, None) + (None,) * n + tuple(d * g_loss for d in d_rgb) + tuple(None if d is None else d * g_loss for d in d_rgb0)


def multires_loss(rgbs, rgb0s, target_patches, full_patch, add_global):
    """The loss of a joint MultiRes iteration (multires_dnerf.py:950-996) and its gradients in ONE launch (swnerf_multires_loss):
    per level mse(rgb_l, target_l) [+ mse(rgb0_l, target_l)], the patches reconstructed through the pyramid, the mse of the
    reconstruction against full_patch, added to the loss with add_global.  rgbs[l] / rgb0s[l]: [ph_l * pw_l, 3] or [ph_l, pw_l, 3];
    rgb0s: None, or a list whose entries may be None; target_patches[l] [ph_l, pw_l, 3] (sides up to PATCH_MAX_SIDE);
    full_patch [ph_0, pw_0, 3].
    -> (loss, per_level, per_level0, global_loss, global_psnr, reconstructed).  Only `loss` is differentiable (with respect to every
    rgb and rgb0): the other values are for the log.  Sums are fp64 in a fixed order: equal bits on every run."""
    n = len(rgbs)
    if not 1 <= n <= PATCH_MAX_LEVELS or len(target_patches) != n or (rgb0s is not None and len(rgb0s) != n):
        raise ValueError(f"swnerf.batching.multires_loss: {n} levels of rgb (1..{PATCH_MAX_LEVELS} are built), {len(target_patches)} of targets")
    rgb0s = [None] * n if rgb0s is None else list(rgb0s)
    targets = [_lib.dev_f32(t, f"target_patches[{l}]", 3).detach() for l, t in enumerate(target_patches)]
    full = _lib.dev_f32(full_patch, "full_patch", 3).detach()
    rs, r0s = [], []
    for l, t in enumerate(targets):
        if t.dim() != 3 or not (1 <= t.shape[0] <= PATCH_MAX_SIDE and 1 <= t.shape[1] <= PATCH_MAX_SIDE):
            raise ValueError(f"swnerf.batching.multires_loss: target_patches[{l}] must be [ph, pw, 3] with sides 1..{PATCH_MAX_SIDE}, got {tuple(t.shape)}")
        for name, r, out in (("rgbs", rgbs[l], rs), ("rgb0s", rgb0s[l], r0s)):
            if r is not None:
                r = _lib.dev_f32(r, f"{name}[{l}]", 3)
                if r.numel() != t.numel():
                    raise ValueError(f"swnerf.batching.multires_loss: {name}[{l}] is {tuple(r.shape)}, its target patch {tuple(t.shape)}")
            out.append(r)
    if full.shape != targets[0].shape:
        raise ValueError(f"swnerf.batching.multires_loss: full_patch is {tuple(full.shape)}, the level-0 patch {tuple(targets[0].shape)}")
    loss, losses, recon = _MultiresLoss.apply(bool(add_global), n, full, *targets, *rs, *r0s)
    L = PATCH_MAX_LEVELS
    per_level = [losses[3 + l] for l in range(n)]
    per_level0 = [None if r0s[l] is None else losses[3 + L + l] for l in range(n)]
    return loss, per_level, per_level0, losses[1], losses[2], recon
