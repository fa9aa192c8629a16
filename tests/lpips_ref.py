"""The seeded recipe the LPIPS tests share, and a dtype-generic torch restatement of the definition
[REF lpipsPyTorch/modules/networks.py:36-63, lpips.py:30-36, utils.py:6-8].  Test infrastructure: the package never imports it.

Pretrained weights are not shipped, so the arithmetic is pinned with SEEDED weights: numpy.random.RandomState(seed) is a frozen
stream.  In layer order, per convolution: weight = standard_normal * sqrt(2 / (Cin k k)), bias = 0.05 * standard_normal; then the
five lin vectors |standard_normal|; everything cast to float32.  tests/golden/lpips.npz holds what the reference's OWN classes
return on these weights and images (tests/golden/make_lpips_vectors.py)."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

# torchvision's `features` of alexnet and vgg16 (configuration D), restated: ("conv", Cin, Cout, k, stride, pad) | ("relu",) | ("pool", k, stride)
ALEX = [("conv", 3, 64, 11, 4, 2), ("relu",), ("pool", 3, 2), ("conv", 64, 192, 5, 1, 2), ("relu",), ("pool", 3, 2),
        ("conv", 192, 384, 3, 1, 1), ("relu",), ("conv", 384, 256, 3, 1, 1), ("relu",), ("conv", 256, 256, 3, 1, 1), ("relu",), ("pool", 3, 2)]


def _vgg():
    out, c = [], 3
    for v in (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"):
        if v == "M":
            out.append(("pool", 2, 2))
        else:
            out += [("conv", c, v, 3, 1, 1), ("relu",)]
            c = v
    return out


FEATURES = {"alex": ALEX, "vgg": _vgg()}
# [REF networks.py:82-83, 93-94] (the fixture holds the reference's own lists, read with ast; test_lpips_host.py compares)
TARGET_LAYERS = {"alex": [2, 5, 8, 10, 12], "vgg": [4, 9, 16, 23, 30]}
N_CHANNELS = {"alex": [64, 192, 384, 256, 256], "vgg": [64, 128, 256, 512, 512]}
MEAN, STD = (-.030, -.088, -.188), (.458, .448, .450)
SEEDS = {"alex": 11, "vgg": 12}
SIZES = ((67, 83), (31, 50), (163, 178))          # the fixture's cases, both nets


def seeded_weights(net_type, seed=None):
    """{"backbone": {"{i}.weight" / "{i}.bias": float32 tensor}, "lin": {"{k}.1.weight": [1,C,1,1]}}, i the position in `features`."""
    rs = np.random.RandomState(SEEDS[net_type] if seed is None else seed)
    bb, lin = {}, {}
    for i, e in enumerate(FEATURES[net_type]):
        if e[0] == "conv":
            _, cin, cout, k, _, _ = e
            bb[f"{i}.weight"] = torch.from_numpy((rs.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32))
            bb[f"{i}.bias"] = torch.from_numpy((0.05 * rs.standard_normal(cout)).astype(np.float32))
    for k, c in enumerate(N_CHANNELS[net_type]):
        lin[f"{k}.1.weight"] = torch.from_numpy(np.abs(rs.standard_normal((1, c, 1, 1))).astype(np.float32))
    return {"backbone": bb, "lin": lin}


def weights_checksum(w):
    return float(sum(float(t.double().sum()) for t in w["backbone"].values()) + sum(float(t.double().sum()) for t in w["lin"].values()))


def sequential(net_type, w, dtype=torch.float64):
    """The recipe's nn.Sequential, laid out as torchvision's `features`."""
    mods = []
    for i, e in enumerate(FEATURES[net_type]):
        if e[0] == "conv":
            m = nn.Conv2d(e[1], e[2], e[3], e[4], e[5])
            m.weight.data = w["backbone"][f"{i}.weight"].clone()
            m.bias.data = w["backbone"][f"{i}.bias"].clone()
            mods.append(m)
        elif e[0] == "relu":
            mods.append(nn.ReLU(inplace=False))
        else:
            mods.append(nn.MaxPool2d(kernel_size=e[1], stride=e[2]))
    return nn.Sequential(*mods).to(dtype).requires_grad_(False)


def image_pair(H, W, seed):
    """(render, gt) float32 [3,H,W] with values k / 255: a smooth pattern plus noise, clipped and rounded to 8 bits."""
    rs = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    gt = np.stack([0.5 + 0.4 * np.sin(6.0 * xx + 2.0 * c) * np.cos(5.0 * yy - c) for c in range(3)]) + 0.05 * rs.standard_normal((3, H, W))
    render = gt + 0.08 * rs.standard_normal((3, H, W)) + 0.06 * np.sin(9.0 * (xx + yy))[None]
    q = lambda a: (np.round(np.clip(a, 0.0, 1.0) * 255.0) / 255.0).astype(np.float32)      # noqa: E731
    return q(render), q(gt)


def case_pair(k):
    H, W = SIZES[k]
    return image_pair(H, W, 100 + k)


def lpips_terms(x, y, net_type, w, dtype=torch.float64):
    """x, y: [B,3,H,W].  Returns [B,6] of `dtype`: column 0 = LPIPS, 1..5 = the layer terms, every operation in `dtype`."""
    x, y = x.to(dtype), y.to(dtype)
    mean = torch.tensor(MEAN, dtype=torch.float32).to(x.device, dtype)[None, :, None, None]       # (the float32 values of the buffers)
    std = torch.tensor(STD, dtype=torch.float32).to(x.device, dtype)[None, :, None, None]
    taps = {t - 1 for t in TARGET_LAYERS[net_type]}

    def feats(z):
        z = (z - mean) / std
        out = []
        for i, e in enumerate(FEATURES[net_type]):
            if e[0] == "conv":
                z = F.conv2d(z, w["backbone"][f"{i}.weight"].to(dtype), w["backbone"][f"{i}.bias"].to(dtype), stride=e[4], padding=e[5])
            elif e[0] == "relu":
                z = F.relu(z)
            else:
                z = F.max_pool2d(z, e[1], e[2])
            if i in taps:
                out.append(z / (torch.sqrt(torch.sum(z ** 2, dim=1, keepdim=True)) + 1e-10))
            if len(out) == len(taps):
                break
        return out

    terms = []
    for k, (fx, fy) in enumerate(zip(feats(x), feats(y))):
        d = (fx - fy) ** 2
        terms.append((d * w["lin"][f"{k}.1.weight"].to(dtype)).sum(1).mean((1, 2)))
    t = torch.stack(terms, dim=1)
    return torch.cat([t.sum(1, keepdim=True), t], dim=1)


def pooled_bar(cases, margin=8.0):
    """The bar of a GPU comparison with float64: `margin` x the largest relative distance, over ALL of `cases` (pairs of
    (float32 result, float64 result) tensors of the same restatement on the CPU), so that one lucky case cannot shrink it."""
    worst = 0.0
    for r32, r64 in cases:
        worst = max(worst, float(((r32.double() - r64).abs() / r64.abs().clamp_min(1e-300)).max()))
    return margin * worst, worst
