"""Image resizing on the device, byte for byte what Pillow's Image.resize returns (include/gp_resize.h, csrc/resize_kernels.hip):
the step between decoding an image file and scoring or training on it at a reduced resolution.

  [REF metrics.py readImages]              Image.open(f).resize((int(w * ratio), int(h * ratio))), then to_tensor and [:, :3]
  [REF utils/general_utils.py:21-27]       PILtoTorch: resize, / 255.0, permute

Pillow's 8-bit resampler is integer arithmetic once its coefficient tables exist: two separable passes with 22-bit fixed-point weights
and an 8-bit rounding between them.  The tables are built on the host in double (gp_resize_coeffs) and cached on the device per
(device, in, out, filter); the passes run in one fused launch with the intermediate in LDS, or in two launches through a scratch
buffer where a tile's window does not fit (gp_resize_path tells which).  RGBA goes through premultiplied alpha as Image.resize sends
it.  HIP only: CPU tensors raise."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

GP_RESIZE_ABI_VERSION = 1           # include/gp_resize.h
LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = 1, 2, 3, 4, 5      # Pillow's Image.Resampling values
FILTERS = {"lanczos": LANCZOS, "bilinear": BILINEAR, "bicubic": BICUBIC, "box": BOX, "hamming": HAMMING}
DST_U8, DST_F32 = 0, 1
PATH_COPY, PATH_FUSED, PATH_TWO_LAUNCH, PATH_HORIZONTAL, PATH_VERTICAL = range(5)
TILE_W, TILE_H = 64, 32
MAX_PLANES = 65535                  # B * C of one call (the planes are one grid dimension)
TABLE_CACHE = 64                    # axes kept on the device


def _prototypes():
    i32, i64, P = C.c_int32, C.c_int64, _lib.Ptr
    return {   # name: (restype, argtypes), as include/gp_resize.h declares them (tests/test_resize_host.py compares the two)
        "gp_resize_abi_version": (i32, []),
        "gp_resize_ksize": (i32, [i32, i32, i32]),
        "gp_resize_coeffs": (i32, [i32, i32, i32, P, P]),
        "gp_resize_scratch_bytes": (i64, [i32, i32, i32, i32, i32, i32, i32]),
        "gp_resize_path": (i32, [i32, i32, i32, i32, i32]),
        "gp_resize_u8": (i32, [i32, i32, i32, i32, i32, i32, i32, P, i64, P, P, i32, P, P, i32, i32, i32, P, i64, P, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi("gp_resize.h", "gp_resize_abi_version", GP_RESIZE_ABI_VERSION, PROTOTYPES)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)

_tables: dict = {}


def filter_id(resample):
    """A filter's name or Pillow's integer constant -> GP_RESIZE_*.  NEAREST is not a convolution and is not offered."""
    if isinstance(resample, str):
        f = FILTERS.get(resample.lower())
    else:
        f = int(resample) if int(resample) in FILTERS.values() else None
    if f is None:
        raise RuntimeError(f"resize: resample = {resample!r} is not one of {sorted(FILTERS)} (or Pillow's constants 1 .. 5)")
    return f


def coeffs(n_in, n_out, resample="bicubic"):
    """The tables of one axis on the host: (bounds int32 [n_out, 2] = (xmin, n), coeffs int32 [n_out, ksize]).  No device is touched."""
    f, l = filter_id(resample), lib()
    taps = int(l.gp_resize_ksize(n_in, n_out, f))
    if taps < 0:
        raise _lib.GpHipError(f"gp_resize_ksize: {_lib.last_error()}")
    bounds, k = np.empty((n_out, 2), np.int32), np.empty((n_out, taps), np.int32)
    _lib.check(l.gp_resize_coeffs(n_in, n_out, f, bounds.ctypes.data, k.ctypes.data), "gp_resize_coeffs")
    return bounds, k


def path(size_in, size_out, resample="bicubic"):
    """GP_RESIZE_PATH_* of (width, height) -> (width, height)."""
    (W, H), (Wo, Ho) = size_in, size_out
    r = int(lib().gp_resize_path(H, W, Ho, Wo, filter_id(resample)))
    if r < 0:
        raise _lib.GpHipError(f"gp_resize_path: {_lib.last_error()}")
    return r


def axis_tables(device, n_in, n_out, f):
    """(bounds, coeffs, taps) of one axis on `device`, cached per (device, in, out, filter); (None, None, 0) where the size stays."""
    if n_in == n_out:
        return None, None, 0
    key = (device.index, n_in, n_out, f)
    hit = _tables.get(key)
    if hit is None:
        bounds, k = coeffs(n_in, n_out, f)
        both = torch.from_numpy(np.concatenate([bounds.reshape(-1), k.reshape(-1)])).to(device)      # (one copy per axis, once)
        hit = (both[:2 * n_out], both[2 * n_out:], k.shape[1])
        if len(_tables) >= TABLE_CACHE:
            _tables.pop(next(iter(_tables)))
        _tables[key] = hit
    return hit


def target_size(size, w, h, name="<image>"):
    """`size` of the decoders' and the loops' resize= : (width, height), or a callable (w, h) -> (width, height).  A side below 1
    raises, naming the file."""
    Wo, Ho = size(w, h) if callable(size) else size
    Wo, Ho = int(Wo), int(Ho)
    if Wo < 1 or Ho < 1:
        raise ValueError(f"resize: {name}: {w} x {h} -> {Wo} x {Ho}: a target size of 0")
    return Wo, Ho


def resize(images, size, resample="bicubic", *, dtype=torch.uint8, alpha=None, out=None):
    """images: uint8 [B, C, H, W] or [C, H, W] on the device, C = 1, 3 or 4 (Pillow's L, RGB, RGBA), each image contiguous (the
    batch stride is free).  size = (width, height), as Image.resize takes it.  resample: "box", "bilinear", "hamming", "bicubic",
    "lanczos" or Pillow's constant.  Returns [B, C, height, width] (or [C, height, width]) of `dtype`: torch.uint8, Pillow's bytes,
    or torch.float32 = byte / 255 (bit-equal to uint8.to(float32) / 255.0).  alpha: premultiply the colours by plane 3 before and
    divide after, as Image.resize does for RGBA (default: C == 4).  out: the tensor to write, of the result's shape and dtype, each
    image contiguous.  Nothing is read from the device."""
    if not torch.is_tensor(images):
        raise RuntimeError("resize: images must be a tensor")
    if not images.is_cuda:
        raise RuntimeError(f"resize: images are on {images.device} -- HIP kernels only (no CPU fallback)")
    if images.dtype != torch.uint8:
        raise RuntimeError(f"resize: images must be torch.uint8 (got {images.dtype}); the resampler is Pillow's 8-bit one")
    if dtype not in (torch.uint8, torch.float32):
        raise RuntimeError(f"resize: dtype must be torch.uint8 or torch.float32 (got {dtype})")
    single = images.dim() == 3
    x = images.detach()[None] if single else images.detach()
    if x.dim() != 4 or x.shape[1] not in (1, 3, 4):
        raise RuntimeError(f"resize: images must be [B, C, H, W] or [C, H, W] with C = 1, 3 or 4 (got {tuple(images.shape)})")
    B, Cn, H, W = x.shape
    f = filter_id(resample)
    Wo, Ho = target_size(size, W, H)
    alpha = Cn == 4 if alpha is None else bool(alpha)
    if alpha and Cn != 4:
        raise RuntimeError(f"resize: alpha needs four planes (got C = {Cn})")
    if B < 1:
        raise RuntimeError("resize: an empty batch")
    if B > 1 and x.stride(0) < Cn * H * W or x[0].numel() and not x[0].is_contiguous():
        x = x.contiguous()
    device = x.device
    if out is None:
        dst = torch.empty(B, Cn, Ho, Wo, dtype=dtype, device=device)
    else:
        dst = out[None] if single else out
        if dst.dtype != dtype or dst.device != device or tuple(dst.shape) != (B, Cn, Ho, Wo) or not dst[0].is_contiguous() \
                or (B > 1 and dst.stride(0) < Cn * Ho * Wo):
            raise RuntimeError(f"resize: out must be {dtype} [{B}, {Cn}, {Ho}, {Wo}] on {device}, each image contiguous")
    l = lib()
    with _lib.on_device(device):
        xb, xk, xt = axis_tables(device, W, Wo, f)
        yb, yk, yt = axis_tables(device, H, Ho, f)
        for lo in range(0, B, MAX_PLANES // Cn):
            n = min(B - lo, MAX_PLANES // Cn)
            scratch = _lib.scratch(l.gp_resize_scratch_bytes, n, Cn, H, W, Ho, Wo, f, device=device)
            _lib.check(l.gp_resize_u8(n, Cn, H, W, Ho, Wo, f, x[lo:], x.stride(0) if B > 1 else Cn * H * W, xb, xk, xt, yb, yk, yt, int(alpha),
                                      DST_U8 if dtype == torch.uint8 else DST_F32, dst[lo:],
                                      (dst.stride(0) if B > 1 else Cn * Ho * Wo) * dst.element_size(), scratch if scratch.numel() else None,
                                      _lib.stream_ptr(device)), "gp_resize_u8")
    return out if out is not None else dst[0] if single else dst


def as_batch(images):
    """A list of equal-shaped [C, H, W] tensors as one [B, C, H, W] tensor: a view where they are the slots of one buffer, evenly
    spaced (what the decoders return for a shape group), else a stacked copy."""
    first = images[0]
    if len(images) == 1:
        return first[None]
    step = images[1].data_ptr() - first.data_ptr()
    same = all(im.untyped_storage().data_ptr() == first.untyped_storage().data_ptr() and im.is_contiguous()
               and im.data_ptr() - first.data_ptr() == k * step for k, im in enumerate(images))
    if same and step >= first.numel() * first.element_size() and step % first.element_size() == 0:
        return first.as_strided((len(images),) + tuple(first.shape), (step // first.element_size(),) + tuple(first.stride()))
    return torch.stack(images)


def resize_each(images, size, resample="bicubic", *, dtype=torch.uint8, names=None):
    """A list of uint8 [C, H, W] device tensors of any shapes -> the list resized, one batched `resize` call per run of equal
    shapes and equal targets.  size: (width, height) or a callable (w, h) -> (width, height)."""
    by_shape = {}
    for i, im in enumerate(images):
        Wo, Ho = target_size(size, im.shape[2], im.shape[1], names[i] if names is not None else f"<image {i}>")
        by_shape.setdefault((tuple(im.shape), Wo, Ho), []).append(i)
    out = [None] * len(images)
    for (_, Wo, Ho), idx in by_shape.items():
        got = resize(as_batch([images[i] for i in idx]), (Wo, Ho), resample, dtype=dtype)
        for k, i in enumerate(idx):
            out[i] = got[k]
    return out
