"""Depth renders on the device (csrc/gp_depth.h, csrc/depth_kernels.hip): the depth map of a view, its picture, its normals, the
visible surface as a point cloud, and the standard depth errors against a ground truth.

render() returns "depth" = sum z_i alpha_i T_i and nothing used it ([REF eval.py:109] unwraps the value and drops it; metrics.evaluate_dirs
skips files whose name contains "depth", as [REF metrics.py:36]).  render_depth is ONE ordinary render with an override colour of ones
over a zero background of its own: the image's channel 0 is then alpha = sum alpha_i T_i and the returned "depth" the accumulated z; resolve
divides.  colorize is depth or disparity through a 256-row table (default feature_vis.jet_lut) with the range found on the device when
none is given; normals are the cross product of central differences of the unprojected pixels, in camera space, facing the camera;
unproject is the ordered compaction of the valid pixels to world points (with colours and pixel numbers); depth_metrics gives AbsRel,
SqRel, RMSE, RMSE-log, the three delta shares, SIlog and the least-squares scale in float64, bit-reproducible.  write_pfm / read_pfm are
PFM files (host only).  The header states every definition in full, tests/depth_ref.py restates them in numpy and the tests pin that.

The depth is the rasterizer's z-depth (not the ray distance), alpha-weighted: where surfaces at different depths overlap in a pixel it
is their weighted mean, not the first surface.

HIP only: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
import math
import os
import re
from collections import namedtuple

import numpy as np
import torch

from . import _lib

GP_DEPTH_ABI_VERSION = 1            # csrc/gp_depth.h
TILE, SUMS, COLUMNS, LUT = 1024, 12, 12, 256
METRIC_NAMES = ("count", "abs_rel", "sq_rel", "rmse", "rmse_log", "delta1", "delta2", "delta3", "silog", "scale", "gt_mean", "reserved")
MODES = {"depth": 0, "disparity": 1}
HEADER = "../gaussianprediction_amd/csrc/gp_depth.h"     # relative to include/: the header is not one of include/ 


class DepthViewC(C.Structure):
    """gp_depth_view."""
    _fields_ = [("cam2world", C.c_void_p), ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("W", C.c_int32), ("H", C.c_int32)]


def _prototypes():
    i32, i64, f32, P, V = C.c_int32, C.c_int64, C.c_float, _lib.Ptr, C.POINTER(DepthViewC)
    return {   # name: (restype, argtypes), as csrc/gp_depth.h declares them (tests/test_depth_host.py compares the two)
        "gp_depth_abi_version": (i32, []),
        "gp_depth_resolve": (i32, [P, P, f32, P, P, i32, i32, P]),
        "gp_depth_colorize": (i32, [P, P, i32, f32, f32, P, f32, f32, f32, P, P, i32, i32, P]),
        "gp_depth_normals": (i32, [P, P, V, P, P, i32, i32, P]),
        "gp_depth_normals_image": (i32, [P, P, f32, f32, f32, P, i32, i32, P]),
        "gp_depth_unproject_scratch_bytes": (i64, [i32, i32]),
        "gp_depth_unproject": (i32, [P, P, P, V, P, P, P, P, P, i32, i32, P]),
        "gp_depth_metrics_scratch_bytes": (i64, [i32, i32, i32]),
        "gp_depth_metrics": (i32, [P, P, P, P, f32, f32, i32, i32, i32, P, P, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi(HEADER, "gp_depth_abi_version", GP_DEPTH_ABI_VERSION, PROTOTYPES, register=False)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)

DepthResult = namedtuple("DepthResult", "depth alpha valid")                 # [H, W] float32, [H, W] float32, [H, W] bool
DepthView = namedtuple("DepthView", "cam2world tanfovx tanfovy W H c")       # the [4, 4] tensor (kept alive), the constants, the gp_depth_view


# ---- refusals that need no device, as the library words them (None: accepted) ----
def check_plane(H, W):
    H, W = int(H), int(W)
    if H <= 0 or W <= 0:
        return "H and W must be > 0"
    if H * W >= 2 ** 31:
        return "H*W must be below 2^31"
    return None


def check_batch(B, H, W):
    if int(B) <= 0:
        return "B must be > 0"
    why = check_plane(H, W)
    if why:
        return why
    return "B must be at most 65535" if int(B) > 65535 else None


def _refuse(what, why, **sizes):
    if why:
        raise _lib.GpHipError(f"{what}: {why} ({', '.join(f'{k} = {v}' for k, v in sizes.items())})")


def _scalar(what, name, v):
    v = float(v)
    if v != v:
        raise _lib.GpHipError(f"{what}: {name} must not be NaN")
    return v


def _device_f32(what, *args):
    """Each (name, tensor, shape text, shape test) as a contiguous float32 tensor on a HIP device, or the refusal: the shapes and
    types of all of them first, then where they are."""
    for name, t, shape_text, ok in args:
        if not torch.is_tensor(t) or t.dtype != torch.float32 or not ok(t):
            raise RuntimeError(f"{what}: {name} must be a {shape_text} float32 tensor")
    for name, t, _, _ in args:
        if not t.is_cuda:
            raise RuntimeError(f"{what}: {name} is on {t.device} -- HIP kernels only (no CPU fallback)")
    return [t.detach().contiguous() for _, t, _, _ in args]


def _like(what, name, t, first):
    if t.shape != first.shape or t.device != first.device:
        raise RuntimeError(f"{what}: {name} must be a {list(first.shape)} tensor on {first.device}")


def _mask_u8(what, name, m, shape, device):
    if m is None:
        return None
    if not torch.is_tensor(m) or m.dtype not in (torch.bool, torch.uint8) or tuple(m.shape) != tuple(shape):
        raise RuntimeError(f"{what}: {name} must be a {list(shape)} bool or uint8 tensor")
    if m.device != device:
        raise RuntimeError(f"{what}: {name} is on {m.device}, the depth on {device} -- HIP kernels only (no CPU fallback)")
    m = m.detach().contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def _background(what, background):
    bg = [float(v) for v in background]
    if len(bg) != 3:
        raise RuntimeError(f"{what}: background must hold three numbers")
    return bg


_plane = lambda t: t.dim() == 2               # noqa: E731


# ---- views ----
def view_constants(view):
    """The gp_depth_view of a camera: cam2world, the inverse of its world_view_transform -- formed in float64 on the host and cast,
    once per camera: the matrix is read from the device that one time and the result is kept on the camera object -- plus
    tan(FoVx / 2), tan(FoVy / 2), image_width and image_height, as renderer._settings hands them to the rasterizer."""
    if isinstance(view, DepthView):
        return view
    vm = view.world_view_transform
    if not torch.is_tensor(vm) or vm.dtype != torch.float32 or tuple(vm.shape) != (4, 4):
        raise RuntimeError("view_constants: world_view_transform must be a [4, 4] float32 tensor")
    if not vm.is_cuda:
        raise RuntimeError(f"view_constants: world_view_transform is on {vm.device} -- HIP kernels only (no CPU fallback)")
    W, H = int(view.image_width), int(view.image_height)
    _refuse("view_constants", check_plane(H, W), H=H, W=W)
    tx, ty = math.tan(float(view.FoVx) * 0.5), math.tan(float(view.FoVy) * 0.5)
    if tx != tx or ty != ty:
        raise _lib.GpHipError("view_constants: tanfovx and tanfovy must not be NaN")
    kept = getattr(view, "_gp_depth_view", None)
    key = (vm.data_ptr(), vm._version, tx, ty, W, H)
    if kept is not None and kept[0] == key:
        return kept[1]
    inv = np.linalg.inv(vm.detach().cpu().numpy().astype(np.float64)).astype(np.float32)       # (the one read of this camera)
    c2w = torch.from_numpy(np.ascontiguousarray(inv)).to(vm.device)
    out = DepthView(c2w, tx, ty, W, H, DepthViewC(c2w.data_ptr(), tx, ty, W, H))
    try:
        view._gp_depth_view = (key, out)
    except AttributeError:                        # (a view that takes no attributes is converted every time)
        pass
    return out


def _view_for(what, view, H, W, device):
    v = view_constants(view)
    if (v.H, v.W) != (H, W) or v.cam2world.device != device:
        raise RuntimeError(f"{what}: the view is {v.H} x {v.W} on {v.cam2world.device}, the depth {H} x {W} on {device}")
    return v


# ---- the entries ----
def resolve(accum, alpha, alpha_min=1e-3):
    """DepthResult of the composite's two planes [H, W]: depth = accum / alpha where alpha >= alpha_min and the quotient is finite and
    > 0 (valid), else 0; alpha as it came."""
    what = "resolve"
    accum, alpha = _device_f32(what, ("accum", accum, "[H, W]", _plane), ("alpha", alpha, "[H, W]", _plane))
    _like(what, "alpha", alpha, accum)
    H, W = accum.shape
    _refuse(what, check_plane(H, W), H=H, W=W)
    alpha_min = _scalar(what, "alpha_min", alpha_min)
    dev = accum.device
    depth = torch.empty(H, W, dtype=torch.float32, device=dev)
    valid = torch.empty(H, W, dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.check(lib().gp_depth_resolve(accum, alpha, alpha_min, depth, valid, H, W, _lib.stream_ptr(dev)), "gp_depth_resolve")
    return DepthResult(depth, alpha, valid.view(torch.bool))


def render_depth(view, gaussians, pipeline, iteration, time=None, alpha_min=1e-3):
    """The depth map of `view` (at `time`, for a model that takes one) as a DepthResult.  Under no_grad: ONE render() with
    override_color = ones [N, 3] over a zero background of its own, whatever the scene's is; alpha is channel 0 of its image
    (unclamped), accum its "depth"; then resolve."""
    from .renderer import render
    view = view["cam"] if isinstance(view, dict) else view
    vm = view.world_view_transform
    if not torch.is_tensor(vm) or not vm.is_cuda:
        raise RuntimeError(f"render_depth: the view is on {getattr(vm, 'device', None)} -- HIP kernels only (no CPU fallback)")
    dev = vm.device
    H, W = int(view.image_height), int(view.image_width)
    alpha_min = _scalar("render_depth", "alpha_min", alpha_min)
    with torch.no_grad():
        ones = torch.ones(gaussians.get_xyz.shape[0], 3, dtype=torch.float32, device=dev)
        if time is not None:
            time = torch.as_tensor(time, dtype=torch.float32).reshape(-1)[:1].to(dev)
        out = render(view, gaussians, pipeline, torch.zeros(3, dtype=torch.float32, device=dev), time=time, it=iteration, override_color=ones)
        return resolve(out["depth"].reshape(H, W), out["render"][0], alpha_min)


def colorize(depth, valid=None, mode="disparity", near=None, far=None, lut=None, background=(0, 0, 0), return_range=False):
    """[3, H, W] float32: depth [H, W] through a 256-row colour table.  mode "depth" colours the depth, "disparity" 1 / depth.  valid
    [H, W] bool or uint8: the other pixels, and those whose value is not finite or not > 0, take `background`.  near / far: the
    values (of the coloured quantity) mapped to the table's first and last row, both or neither; neither (or near >= far) takes the
    smallest and the largest value over the coloured pixels, found on the device in the same call ((0, 1) where there are none) --
    nothing is read.  lut: [256, 3] float32 on the device (default feature_vis.jet_lut), read by feature_vis.colormap's rule.
    return_range: also the [2] float32 device tensor of the pair used."""
    what = "colorize"
    depth, = _device_f32(what, ("depth", depth, "[H, W]", _plane))
    H, W = depth.shape
    _refuse(what, check_plane(H, W), H=H, W=W)
    if mode not in MODES:
        raise RuntimeError(f"{what}: mode = {mode!r} must be 'disparity' or 'depth'")
    if (near is None) != (far is None):
        raise RuntimeError(f"{what}: near and far go together (both or neither)")
    lo, hi = (0.0, 0.0) if near is None else (_scalar(what, "near", near), _scalar(what, "far", far))
    bg = _background(what, background)
    valid = _mask_u8(what, "valid", valid, (H, W), depth.device)
    dev = depth.device
    if lut is None:
        from .feature_vis import jet_lut
        lut = jet_lut(dev)
    else:
        lut, = _device_f32(what, ("lut", lut, "[256, 3]", lambda t: tuple(t.shape) == (LUT, 3)))
        if lut.device != dev:
            raise RuntimeError(f"{what}: lut must be [256, 3] on {dev}")
    out = torch.empty(3, H, W, dtype=torch.float32, device=dev)
    rng = torch.empty(2, dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        _lib.check(lib().gp_depth_colorize(depth, valid, MODES[mode], lo, hi, lut, bg[0], bg[1], bg[2], rng, out, H, W, _lib.stream_ptr(dev)),
                   "gp_depth_colorize")
    return (out, rng) if return_range else out


def normals(depth, valid, view):
    """(normals [3, H, W] float32, nvalid [H, W] bool): the camera-space unit normal of every pixel whose four neighbours are inside the
    image and valid -- the cross product of the central differences of the unprojected pixels, turned to face the camera (+z looks
    away from it: a fronto-parallel surface has n_z = -1) -- and zeros elsewhere.  valid: [H, W] bool or uint8, or None for all."""
    what = "normals"
    depth, = _device_f32(what, ("depth", depth, "[H, W]", _plane))
    H, W = depth.shape
    _refuse(what, check_plane(H, W), H=H, W=W)
    valid = _mask_u8(what, "valid", valid, (H, W), depth.device)
    v = _view_for(what, view, H, W, depth.device)
    dev = depth.device
    out = torch.empty(3, H, W, dtype=torch.float32, device=dev)
    nvalid = torch.empty(H, W, dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.check(lib().gp_depth_normals(depth, valid, C.byref(v.c), out, nvalid, H, W, _lib.stream_ptr(dev)), "gp_depth_normals")
    return out, nvalid.view(torch.bool)


def normals_image(normals, nvalid, background=(0, 0, 0)):
    """[3, H, W] float32 in [0, 1]: n * 0.5 + 0.5 where nvalid, `background` elsewhere."""
    what = "normals_image"
    normals, = _device_f32(what, ("normals", normals, "[3, H, W]", lambda t: t.dim() == 3 and t.shape[0] == 3))
    H, W = normals.shape[1:]
    _refuse(what, check_plane(H, W), H=H, W=W)
    if nvalid is None:
        raise RuntimeError(f"{what}: nvalid must be a {[H, W]} bool or uint8 tensor")
    nvalid = _mask_u8(what, "nvalid", nvalid, (H, W), normals.device)
    bg = _background(what, background)
    dev = normals.device
    out = torch.empty(3, H, W, dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        _lib.check(lib().gp_depth_normals_image(normals, nvalid, bg[0], bg[1], bg[2], out, H, W, _lib.stream_ptr(dev)), "gp_depth_normals_image")
    return out


def unproject(depth, valid, view, image=None, return_index=False):
    """The valid pixels as world points, in row-major pixel order: points [K, 3] float32 -- and colors [K, 3] gathered from image
    [3, H, W] where one is given, and with return_index the pixel numbers y * W + x [K] int32 -- as a tuple in that order (points alone
    where nothing else is asked for).  valid: [H, W] bool or uint8, or None for every pixel.  K is counted on the device by an ordered
    stream compaction; this function reads `count` once to slice its results -- the only host read of the module besides
    view_constants' one read of a camera's matrix."""
    what = "unproject"
    depth, = _device_f32(what, ("depth", depth, "[H, W]", _plane))
    H, W = depth.shape
    _refuse(what, check_plane(H, W), H=H, W=W)
    dev = depth.device
    if image is not None:
        image, = _device_f32(what, ("image", image, f"[3, {H}, {W}]", lambda t: tuple(t.shape) == (3, H, W)))
        if image.device != dev:
            raise RuntimeError(f"{what}: image is on {image.device}, the depth on {dev}")
    valid = _mask_u8(what, "valid", valid, (H, W), dev)
    v = _view_for(what, view, H, W, dev)
    points = torch.empty(H * W, 3, dtype=torch.float32, device=dev)
    colors = torch.empty(H * W, 3, dtype=torch.float32, device=dev) if image is not None else None
    index = torch.empty(H * W, dtype=torch.int32, device=dev) if return_index else None
    count = torch.empty(1, dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        scratch = _lib.scratch(lib().gp_depth_unproject_scratch_bytes, H, W, device=dev)
        _lib.check(lib().gp_depth_unproject(depth, valid, image, C.byref(v.c), points, colors, index, count, scratch, H, W, _lib.stream_ptr(dev)),
                   "gp_depth_unproject")
    K = int(count.item())                         # (the one read)
    out = [points[:K]] + ([colors[:K]] if colors is not None else []) + ([index[:K]] if index is not None else [])
    return out[0] if len(out) == 1 else tuple(out)


def depth_metrics(pred, gt, mask=None, align=None, gt_min=0.0, gt_max=float("inf")):
    """[B, 12] float64 on the device (METRIC_NAMES): per image the count of pixels where mask != 0, both depths are finite and > 0 and
    gt_min <= gt <= gt_max; AbsRel, SqRel, RMSE, RMSE-log, the shares with max(d/g, g/d) below 1.25, 1.25^2 and 1.25^3, SIlog =
    mean(l^2) - mean(l)^2 with l = log d - log g, the least-squares scale sum(d g) / sum(d d), the mean gt, and 0.  A count of 0 gives a
    row of NaN.  pred, gt: [B, H, W] float32, or [H, W] as B = 1; mask: [B, H, W] ([H, W]) bool or uint8.  align="scale": the errors of
    scale * pred, with the first pass's scale column cast to float32 on the device -- two passes, nothing is read; the scale column
    of the result is then that of the scaled prediction (1 up to rounding).  Two calls give equal bytes, and row b of a batch is the
    B = 1 row."""
    what = "depth_metrics"
    ok = lambda t: t.dim() in (2, 3)              # noqa: E731
    pred, gt = _device_f32(what, ("pred", pred, "[B, H, W]", ok), ("gt", gt, "[B, H, W]", ok))
    if pred.dim() == 2:
        pred = pred[None]
        gt = gt[None] if gt.dim() == 2 else gt
        mask = mask[None] if torch.is_tensor(mask) and mask.dim() == 2 else mask
    _like(what, "gt", gt, pred)
    if align not in (None, "scale"):
        raise RuntimeError(f"{what}: align = {align!r} must be None or 'scale'")
    B, H, W = pred.shape
    _refuse(what, check_batch(B, H, W), B=B, H=H, W=W)
    gt_min, gt_max = _scalar(what, "gt_min", gt_min), _scalar(what, "gt_max", gt_max)
    mask = _mask_u8(what, "mask", mask, (B, H, W), pred.device)
    dev = pred.device
    with _lib.on_device(dev):
        scratch = _lib.scratch(lib().gp_depth_metrics_scratch_bytes, B, H, W, device=dev)
        scale = None
        for _ in range(2 if align == "scale" else 1):
            table = torch.empty(B, COLUMNS, dtype=torch.float64, device=dev)
            _lib.check(lib().gp_depth_metrics(pred, gt, mask, scale, gt_min, gt_max, B, H, W, scratch, table, _lib.stream_ptr(dev)), "gp_depth_metrics")
            scale = table[:, 9].to(torch.float32).contiguous()
    return table


# ---- PFM files (host only) ----
def write_pfm(path, depth):
    """depth [H, W] (a tensor anywhere, or an array) -> a one-channel PFM file: the text `Pf\\n<W> <H>\\n-1.0\\n`, then the rows from the
    bottom one to the top one as little-endian float32.  A device tensor is read once."""
    a = depth.detach().cpu().numpy() if torch.is_tensor(depth) else np.asarray(depth)
    if a.ndim != 2:
        raise RuntimeError(f"write_pfm: depth must be [H, W] (got {list(a.shape)})")
    H, W = a.shape
    with open(os.fspath(path), "wb") as fp:
        fp.write(f"Pf\n{W} {H}\n-1.0\n".encode("ascii"))
        fp.write(np.ascontiguousarray(a[::-1], dtype="<f4").tobytes())


def read_pfm(path):
    """The [H, W] float32 CPU tensor of a one-channel PFM file, of either byte order (the sign of its scale).  Another tag, sizes that
    are not positive, a scale of 0 or a length that is not the header's are refused."""
    raw = open(os.fspath(path), "rb").read()
    m = re.match(rb"Pf\s+(-?\d+)\s+(-?\d+)\s+([-+0-9.eE]+)[ \t\r]?\n", raw)
    if not m:
        raise RuntimeError(f"read_pfm: {path} does not begin with a one-channel PFM header (Pf, width height, scale)")
    W, H = int(m.group(1)), int(m.group(2))
    try:
        scale = float(m.group(3))
    except ValueError:
        scale = 0.0
    if W <= 0 or H <= 0 or scale == 0.0 or scale != scale or len(raw) - m.end() != 4 * W * H:
        raise RuntimeError(f"read_pfm: {path} holds {len(raw) - m.end()} bytes of depth, its header says {W} x {H} with scale {m.group(3).decode()}")
    a = np.frombuffer(raw, "<f4" if scale < 0 else ">f4", W * H, m.end()).reshape(H, W)[::-1]
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
