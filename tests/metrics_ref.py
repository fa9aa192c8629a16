"""Test helper: a plain torch restatement of the image metrics gaussianprediction_amd.metrics computes on the device, in whatever
dtype the inputs have (float64 is the yardstick, float32 measures the format's own error).  Definitions: L1 / SSIM as
[REF utils/loss_utils.py:54-98], PSNR in the two call shapes of [REF utils/image_utils.py:18-20] (`[1,3,H,W]` at metrics.py:141,
`[3,H,W]` + .mean() at train.py:107), MS-SSIM as pytorch_msssim.ms_ssim(X, Y, data_range=1, size_average=True) publishes it (the
package is absent: parity with it is unpinned).  Never imported by the package."""
import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
C1, C2 = 0.01 ** 2, 0.03 ** 2
NAMES = ("L1", "MSE", "PSNR", "PSNR_CH", "SSIM", "MS_SSIM", "D_SSIM")


def window_1d(dtype, device="cpu"):
    x = torch.arange(11, dtype=torch.float32) - 5
    g = torch.exp(-(x ** 2) / (2 * 1.5 ** 2))
    return (g / g.sum()).to(dtype=dtype, device=device)


def _filter(x, pad):
    """x [B,3,H,W] -> the 11 x 11 Gaussian-window mean, zero padded (pad=5) or valid (pad=0)."""
    g = window_1d(x.dtype, x.device)
    w2 = (g[:, None] * g[None, :]).expand(3, 1, 11, 11).contiguous()
    return F.conv2d(x, w2, padding=pad, groups=3)


def _ssim_maps(a, b, pad):
    mu1, mu2 = _filter(a, pad), _filter(b, pad)
    s11 = _filter(a * a, pad) - mu1 * mu1
    s22 = _filter(b * b, pad) - mu2 * mu2
    s12 = _filter(a * b, pad) - mu1 * mu2
    cs = (2 * s12 + C2) / (s11 + s22 + C2)
    ssim = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs
    return ssim, cs


def quantize8(x):
    return torch.floor(x * 255 + 0.5).clamp(0, 255) / 255


def l1(a, b):
    return (a - b).abs().flatten(1).mean(1)


def mse(a, b):
    return ((a - b) ** 2).flatten(1).mean(1)


def psnr(a, b):
    """[B,3,H,W] -> [B]: over all three channels (metrics.py's call shape)."""
    return 20 * torch.log10(1.0 / torch.sqrt(mse(a, b)))


def psnr_ch(a, b):
    """[B,3,H,W] -> [B]: the mean of the per-channel PSNR (train.py's call shape)."""
    m = ((a - b) ** 2).flatten(2).mean(2)
    return (20 * torch.log10(1.0 / torch.sqrt(m))).mean(1)


def ssim(a, b):
    return _ssim_maps(a, b, 5)[0].flatten(1).mean(1)


def ms_ssim_levels(a, b):
    """[B,5,3]: mean cs of scales 1-4 and mean ssim of scale 5 per channel, before the ReLU."""
    assert min(a.shape[-2:]) > 160
    rows = []
    for l in range(5):
        s, cs = _ssim_maps(a, b, 0)
        rows.append((s if l == 4 else cs).flatten(2).mean(2))
        if l < 4:
            pad = [n % 2 for n in a.shape[-2:]]
            a = F.avg_pool2d(a, kernel_size=2, padding=pad)
            b = F.avg_pool2d(b, kernel_size=2, padding=pad)
    return torch.stack(rows, dim=1)


def ms_ssim(a, b):
    lv = torch.relu(ms_ssim_levels(a, b))
    w = torch.tensor(WEIGHTS, dtype=a.dtype, device=a.device)
    return torch.prod(lv ** w[None, :, None], dim=1).mean(1)


def all_metrics(a, b, with_ms=True):
    """{name: [B] tensor} (+ "levels" [B,5,3]) for a, b [B,3,H,W]."""
    r = {"L1": l1(a, b), "MSE": mse(a, b), "PSNR": psnr(a, b), "PSNR_CH": psnr_ch(a, b), "SSIM": ssim(a, b)}
    if with_ms:
        r["levels"] = ms_ssim_levels(a, b)
        r["MS_SSIM"] = ms_ssim(a, b)
        r["D_SSIM"] = (1 - r["MS_SSIM"]) / 2
    return r


def probe_pair(H=163, W=178, B=2, seed=0):
    """The smooth test images: gt = a coarse uniform grid upsampled bicubically, clamped, rounded to 8 bits;
    render = gt + 0.05 * noise, clamped.  float32 [B,3,H,W] on the CPU."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(B, 3, 12, 13, generator=g)
    gt = F.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=False).clamp(0, 1)
    gt = torch.round(gt * 255) / 255
    render = (gt + 0.05 * torch.randn(B, 3, H, W, generator=g)).clamp(0, 1)
    return render.contiguous(), gt.contiguous()


GOLDEN_SIZES = ((37, 45), (64, 64))


def golden_pair(k):
    """Image pair k of tests/golden/metrics.npz (numpy PCG64 streams are stable across versions; the file holds a checksum of
    each image to prove it): float32 numpy [3,H,W] render, gt."""
    import numpy as np
    H, W = GOLDEN_SIZES[k]
    rng = np.random.default_rng(100 + k)
    gt = rng.uniform(0.0, 1.0, size=(3, H, W)).astype(np.float32)
    img = np.clip(gt + rng.normal(0.0, 0.1, size=(3, H, W)), 0.0, 1.0).astype(np.float32)
    return img, gt
