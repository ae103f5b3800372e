"""LPIPS v0.1 (AlexNet / VGG16 trunks) restated with torch CPU ops - the reference of tests/test_lpips_host.py and
tests/test_gpu_lpips.py.  float64 by default; fp32=True evaluates the same graph in float32, which is the arithmetic of the
`lpips` package itself (the package is not installed here, so this restatement cannot be run against it: DESIGN.md 6f).

The definition: scaling layer (x - shift) / scale; the trunk's five ReLU taps; per tap unit-normalise over the channels
(f / (|f|_2 + 1e-10)), squared difference, a bias-free 1x1 convolution `lin`, spatial mean; the sum over the taps.

Also the seeded stand-ins for the two weight files (torchvision's trunk checkpoint and the package's lin layers), in their
key layout: He-normal trunk weights, biases of about 0.1, non-negative lin weights."""
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
# (features index, cin, cout, kernel, stride, pad)
ALEX = [(0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1)]
VGG = [(i, ci, co, 3, 1, 1) for i, ci, co in ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256),
                                               (14, 256, 256), (17, 256, 512), (19, 512, 512), (21, 512, 512), (24, 512, 512),
                                               (26, 512, 512), (28, 512, 512))]
CONVS = {"alex": ALEX, "vgg": VGG}
# what happens after the ReLU of each convolution, by position: "tap" and / or a pooling window
AFTER = {"alex": [("tap", 3), ("tap", 3), ("tap", 0), ("tap", 0), ("tap", 0)],
         "vgg": [("", 0), ("tap", 2), ("", 0), ("tap", 2), ("", 0), ("", 0), ("tap", 2), ("", 0), ("", 0), ("tap", 2), ("", 0), ("", 0),
                 ("tap", 0)]}
CHANNELS = {"alex": [64, 192, 384, 256, 256], "vgg": [64, 128, 256, 512, 512]}
E2E_SIZES = {"alex": [(35, 47), (64, 64)], "vgg": [(18, 21), (32, 32)]}    # the end-to-end image sizes of the tests
IMG_SEED = 5
SEEDS = {"alex": 13, "vgg": 12}          # checked by test_lpips_host.py: no tap of the float64 reference is more than half dead


def seeded_weights(net, seed=None):
    """-> (trunk state dict with torchvision's keys, lin state dict with the package's keys), float32"""
    g = torch.Generator().manual_seed(SEEDS[net] if seed is None else seed)
    trunk, lin = {}, {}
    for i, ci, co, k, _, _ in CONVS[net]:
        trunk[f"features.{i}.weight"] = (torch.randn(co, ci, k, k, generator=g, dtype=torch.float64) * (2.0 / (ci * k * k)) ** 0.5).float()
        trunk[f"features.{i}.bias"] = (0.1 + 0.02 * torch.randn(co, generator=g, dtype=torch.float64)).float()
    trunk["classifier.1.weight"] = torch.zeros(2, 2)                        # present in the real file, ignored by the metric
    for j, c in enumerate(CHANNELS[net]):
        lin[f"lin{j}.model.1.weight"] = torch.rand(1, c, 1, 1, generator=g, dtype=torch.float64).float()
    return trunk, lin


def _spec(net):
    """'alex' / 'vgg', or a toy net as (convs, after) in the form of CONVS / AFTER"""
    return (CONVS[net], AFTER[net]) if isinstance(net, str) else net


def taps(net, trunk, x):
    """x [N,3,H,W] (already through the scaling layer), in x's dtype -> the tap feature maps [N,C,h,w]"""
    out = []
    for (i, _, _, _, s, p), (tap, pool) in zip(*_spec(net)):
        x = F.relu(F.conv2d(x, trunk[f"features.{i}.weight"].to(x.dtype), trunk[f"features.{i}.bias"].to(x.dtype), stride=s, padding=p))
        if tap:
            out.append(x)
        if pool:
            x = F.max_pool2d(x, kernel_size=pool, stride=2)
    return out


def layer(f0, f1, lin):
    """one tap: f0, f1 [N,C,h,w], lin [C] (same dtype) -> [N]"""
    n0 = f0 / (torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True)) + 1e-10)
    n1 = f1 / (torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True)) + 1e-10)
    d = (n0 - n1) ** 2
    return F.conv2d(d, lin.reshape(1, -1, 1, 1)).mean(dim=(2, 3)).reshape(-1)


def scaling(x):
    return (x - torch.tensor(SHIFT, dtype=x.dtype).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=x.dtype).view(1, 3, 1, 1)


def lpips_ref(net, trunk, lin, in0, in1, normalize=False, fp32=False):
    """in0, in1 [N,3,H,W] -> [N] float64 (computed in float32 throughout with fp32=True, then widened)"""
    dt = torch.float32 if fp32 else torch.float64
    in0, in1 = torch.as_tensor(in0).to(dt), torch.as_tensor(in1).to(dt)
    if normalize:
        in0, in1 = 2 * in0 - 1, 2 * in1 - 1
    t0, t1 = taps(net, trunk, scaling(in0)), taps(net, trunk, scaling(in1))
    val = None
    for j, (a, b) in enumerate(zip(t0, t1)):
        v = layer(a, b, lin[f"lin{j}.model.1.weight"].to(dt).reshape(-1))
        val = v if val is None else val + v
    return val.double()


def seeded_images(n, h, w, seed):
    """-> (gt, pred) [n,3,h,w] float32 in [0, 1]: uniform noise and a perturbed, clipped copy of it"""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(n, 3, h, w, generator=g)
    pred = (gt + 0.1 * torch.randn(n, 3, h, w, generator=g)).clamp(0, 1)
    return gt, pred


def dead_fractions(net, trunk, x):
    """per tap, the share of units that are exactly zero (float64)"""
    return [float((t == 0).double().mean()) for t in taps(net, trunk, scaling(torch.as_tensor(x).double()))]
