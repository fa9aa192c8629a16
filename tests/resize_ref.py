"""Pillow's 8-bit resampler restated in numpy, independent of csrc/resize_core.h: the coefficient tables in float64 (`coeffs`), one
integer pass along an axis (`resample_axis`), the premultiplied-alpha round trip, and `resize` = what Image.resize returns for the
modes L, RGB and RGBA.  tests/test_resize_host.py holds it against Pillow itself; the GPU tests use Pillow directly."""
import math

import numpy as np

FILTERS = {"box": 4, "bilinear": 2, "hamming": 5, "bicubic": 3, "lanczos": 1}      # name -> Pillow's Image.Resampling value
SUPPORT = {"box": 0.5, "bilinear": 1.0, "hamming": 1.0, "bicubic": 2.0, "lanczos": 3.0}
PRECISION_BITS = 22
ALPHAS = (0, 1, 77, 200, 255)


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def weight(name, x):
    if name == "box":
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if name == "lanczos":
        return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0
    x = abs(x)
    if name == "bilinear":
        return 1.0 - x if x < 1.0 else 0.0
    if name == "hamming":
        if x == 0.0:
            return 1.0
        if x >= 1.0:
            return 0.0
        x = x * math.pi
        return math.sin(x) / x * (float(np.float32(0.54)) + float(np.float32(0.46)) * math.cos(x))     # (the two constants are floats)
    a = -0.5
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def ksize(n_in, n_out, name):
    return int(math.ceil(SUPPORT[name] * max(n_in / n_out, 1.0))) * 2 + 1


def coeffs(n_in, n_out, name):
    """(bounds int32 [n_out, 2] = (xmin, n), k int32 [n_out, ksize], zero beyond n)."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT[name] * fs
    ks = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / fs
    bounds, k = np.zeros((n_out, 2), np.int32), np.zeros((n_out, ks), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - xmin
        w = [weight(name, (x + xmin - center + 0.5) * inv) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            k[xx, x] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
        bounds[xx] = (xmin, n)
    return bounds, k


def resample_axis(planes, n_out, name, axis):
    """uint8 [..., H, W] resampled along `axis` (-1: horizontal, -2: vertical) to n_out samples."""
    src = np.moveaxis(planes, axis, -1).astype(np.int64)
    bounds, k = coeffs(src.shape[-1], n_out, name)
    out = np.empty(src.shape[:-1] + (n_out,), np.uint8)
    for xx, (xmin, n) in enumerate(bounds):
        ss = (1 << (PRECISION_BITS - 1)) + (src[..., xmin:xmin + n] * k[xx, :n].astype(np.int64)).sum(axis=-1)
        assert np.abs(ss).max() < (1 << 31) - (1 << 21)
        out[..., xx] = np.clip(ss >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, -1, axis)


def premultiply(planes):
    """[4, H, W] -> the colours times alpha, Pillow's MULDIV255; alpha as it is."""
    a = planes[3].astype(np.int32)
    out = planes.copy()
    t = planes[:3].astype(np.int32) * a + 128
    out[:3] = ((t >> 8) + t) >> 8
    return out


def unpremultiply(planes):
    a = planes[3].astype(np.int32)
    out = planes.copy()
    c = planes[:3].astype(np.int32)
    q = np.minimum(255, (255 * c) // np.maximum(a, 1))
    out[:3] = np.where((a == 0) | (a == 255), c, q)
    return out


def resize(planes, size, name="bicubic", alpha=None):
    """planes: uint8 [C, H, W]; size = (width, height).  What Image.resize(size, filter) gives for L / RGB / RGBA, planar."""
    C, H, W = planes.shape
    Wo, Ho = size
    alpha = (C == 4) if alpha is None else alpha
    if (Wo, Ho) == (W, H):
        return planes.copy()
    x = premultiply(planes) if alpha else planes
    if Wo != W:
        x = resample_axis(x, Wo, name, -1)
    if Ho != H:
        x = resample_axis(x, Ho, name, -2)
    return unpremultiply(x) if alpha else x


def noise(C, H, W, seed, alphas=ALPHAS):
    """Test planes: noise with some flat and some saturated runs; the alpha plane of C = 4 drawn from `alphas`."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(C, H, W), dtype=np.uint8)
    img[:, : H // 3, : W // 2] = rng.choice(np.array([0, 255], np.uint8), size=(C, H // 3, W // 2))
    if C == 4:
        img[3] = rng.choice(np.array(alphas, np.uint8), size=(H, W))
    return img


def pillow(planes, size, name="bicubic"):
    """Image.resize itself, planar in and out."""
    from PIL import Image
    C = planes.shape[0]
    im = Image.fromarray(planes[0] if C == 1 else np.ascontiguousarray(planes.transpose(1, 2, 0)), {1: "L", 3: "RGB", 4: "RGBA"}[C])
    out = np.array(im.resize(size, FILTERS[name]))
    return out[None] if C == 1 else np.ascontiguousarray(out.transpose(2, 0, 1))
