"""Optical flow rendered on the device (csrc/gp_flow.h, csrc/flow_kernels.hip): where does every pixel go between two times or two
views?  The dense counterpart of eval_render.project_trajectory, the standard comparison of a dynamic reconstruction with an external
flow estimate, and the check on a GCN rollout.

The reference carries the plumbing and never uses it ([REF scene/cameras.py] fwd_flow / bwd_flow and their masks, the "optical flow"
view dicts its render loops unwrap); nothing there renders a flow.  Here every Gaussian's screen displacement between its two
positions (screen_flow: the projection kernel's own pixel centre and depth test) goes through the composite as an unclamped override
colour with a third channel of ones, over a zero background, and the quotient of the composite is the flow (resolve).  colorize is
the Middlebury colour wheel, restated: no flow package is installed where this was written, so PARITY WITH flow_vis / cv2 IS UNPINNED;
the header states every definition in full, tests/flow_ref.py restates them in numpy and the tests pin that.  flow_metrics gives the
end-point error, the > 1 / 3 / 5 px shares and KITTI's Fl against a given flow, in float64 and bit-reproducible; warp is the backward
bilinear warp; write_flo / read_flo are Middlebury's .flo files (host only).

Compositions left to the caller: the photometric check is warp(frame1, flow01) against frame0; a forward-backward occlusion mask is
|flow01 + warp(flow10, flow01)| above a threshold, where both flows are valid.

HIP only: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
import os
import struct
from collections import namedtuple

import numpy as np
import torch

from . import _lib

GP_FLOW_ABI_VERSION = 1             # csrc/gp_flow.h
TILE, SUMS, COLUMNS, WHEEL = 1024, 7, 8, 55
METRIC_NAMES = ("count", "epe", "px1", "px3", "px5", "fl", "gt_magnitude", "reserved")
FLO_TAG = b"PIEH"
HEADER = "../gaussianprediction_amd/csrc/gp_flow.h"      # relative to include/: the header is not one of include/ 


class FlowViewC(C.Structure):
    """gp_flow_view."""
    _fields_ = [("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p), ("W", C.c_int32), ("H", C.c_int32)]


def _prototypes():
    i32, i64, f32, P, V = C.c_int32, C.c_int64, C.c_float, _lib.Ptr, C.POINTER(FlowViewC)
    return {   # name: (restype, argtypes), as csrc/gp_flow.h declares them (tests/test_flow_host.py compares the two)
        "gp_flow_abi_version": (i32, []),
        "gp_flow_project": (i32, [V, V, P, P, i64, P, P]),
        "gp_flow_resolve": (i32, [P, f32, P, P, P, i32, i32, P]),
        "gp_flow_colorize": (i32, [P, P, f32, f32, f32, f32, P, P, i32, i32, P]),
        "gp_flow_metrics_scratch_bytes": (i64, [i32, i32, i32]),
        "gp_flow_metrics": (i32, [P, P, P, i32, i32, i32, P, P, P]),
        "gp_flow_warp": (i32, [P, P, P, i32, i32, i32, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi(HEADER, "gp_flow_abi_version", GP_FLOW_ABI_VERSION, PROTOTYPES, register=False)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)

FlowResult = namedtuple("FlowResult", "flow alpha valid")          # [2, H, W] float32, [H, W] float32, [H, W] bool
FlowView = namedtuple("FlowView", "viewmatrix projmatrix W H c")   # the two [4, 4] tensors (kept alive), the sizes, the gp_flow_view


# ---- refusals that need no device, as the library words them (None: accepted) ----
def check_plane(H, W):
    H, W = int(H), int(W)
    if H <= 0 or W <= 0:
        return "H and W must be > 0"
    if H * W >= 2 ** 31:
        return "H*W must be below 2^31"
    return None


def check_points(N):
    return None if 0 <= int(N) < 2 ** 31 else "N must be >= 0 and below 2^31"


def check_batch(B, H, W):
    if int(B) <= 0:
        return "B must be > 0"
    why = check_plane(H, W)
    if why:
        return why
    return "B must be at most 65535" if int(B) > 65535 else None


def check_warp(Cn, H, W):
    if int(Cn) <= 0:
        return "C must be > 0"
    why = check_plane(H, W)
    if why:
        return why
    return "C*H*W must be below 2^31" if int(Cn) * int(H) * int(W) >= 2 ** 31 else None


def _refuse(what, why, **sizes):
    if why:
        raise _lib.GpHipError(f"{what}: {why} ({', '.join(f'{k} = {v}' for k, v in sizes.items())})")


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


def _mask_u8(what, name, m, shape, device):
    if m is None:
        return None
    if not torch.is_tensor(m) or m.dtype not in (torch.bool, torch.uint8) or tuple(m.shape) != tuple(shape):
        raise RuntimeError(f"{what}: {name} must be a {list(shape)} bool or uint8 tensor")
    if m.device != device:
        raise RuntimeError(f"{what}: {name} is on {m.device}, the flow on {device} -- HIP kernels only (no CPU fallback)")
    m = m.detach().contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


# ---- views ----
def view_constants(view):
    """The gp_flow_view of a camera: its world_view_transform and full_proj_transform [4, 4] float32 on the device and its image_width
    and image_height -- what renderer._settings hands the rasterizer, by pointer: nothing is copied or read."""
    if isinstance(view, FlowView):
        return view
    vm, pm = view.world_view_transform, view.full_proj_transform
    for name, m in (("world_view_transform", vm), ("full_proj_transform", pm)):
        if not torch.is_tensor(m) or m.dtype != torch.float32 or tuple(m.shape) != (4, 4):
            raise RuntimeError(f"view_constants: {name} must be a [4, 4] float32 tensor")
        if not m.is_cuda:
            raise RuntimeError(f"view_constants: {name} is on {m.device} -- HIP kernels only (no CPU fallback)")
    W, H = int(view.image_width), int(view.image_height)
    _refuse("view_constants", check_plane(H, W), H=H, W=W)
    vm, pm = vm.detach().contiguous(), pm.detach().contiguous()
    return FlowView(vm, pm, W, H, FlowViewC(vm.data_ptr(), pm.data_ptr(), W, H))


def screen_flow(xyz0, xyz1, view0, view1=None):
    """[N, 3] float32: per Gaussian (pix1.x - pix0.x, pix1.y - pix0.y, 1) between its position xyz0 seen in view0 and xyz1 seen in
    view1 (default view0: pure scene motion), and (0, 0, 0) where either is at or behind the rasterizer's depth limit or a coordinate is
    not finite -- the rows render() takes as override_color."""
    what = "screen_flow"
    rows = lambda t: t.dim() == 2 and t.shape[1] == 3               # noqa: E731
    xyz0, xyz1 = _device_f32(what, ("xyz0", xyz0, "[N, 3]", rows), ("xyz1", xyz1, "[N, 3]", rows))
    if xyz1.shape != xyz0.shape or xyz1.device != xyz0.device:
        raise RuntimeError(f"{what}: xyz1 must be a {list(xyz0.shape)} tensor on {xyz0.device}")
    N = xyz0.shape[0]
    _refuse(what, check_points(N), N=N)
    v0 = view_constants(view0)
    v1 = v0 if view1 is None else view_constants(view1)
    for v in (v0, v1):
        if v.viewmatrix.device != xyz0.device:
            raise RuntimeError(f"{what}: the view is on {v.viewmatrix.device}, xyz0 on {xyz0.device}")
    out = torch.empty(N, 3, dtype=torch.float32, device=xyz0.device)
    with _lib.on_device(xyz0.device):
        _lib.check(lib().gp_flow_project(C.byref(v0.c), C.byref(v1.c), xyz0, xyz1, N, out, _lib.stream_ptr(xyz0.device)), "gp_flow_project")
    return out


def resolve(composite, alpha_min=1e-3):
    """FlowResult of a composite [3, H, W] rendered from screen_flow's rows over a zero background: alpha = composite[2], flow =
    composite[0:2] / alpha where alpha >= alpha_min and both quotients are finite (valid), else 0."""
    what = "resolve"
    composite, = _device_f32(what, ("composite", composite, "[3, H, W]", lambda t: t.dim() == 3 and t.shape[0] == 3))
    H, W = composite.shape[1:]
    _refuse(what, check_plane(H, W), H=H, W=W)
    alpha_min = float(alpha_min)
    if alpha_min != alpha_min:
        raise _lib.GpHipError(f"{what}: alpha_min must not be NaN")
    dev = composite.device
    flow = torch.empty(2, H, W, dtype=torch.float32, device=dev)
    alpha = torch.empty(H, W, dtype=torch.float32, device=dev)
    valid = torch.empty(H, W, dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.check(lib().gp_flow_resolve(composite, alpha_min, flow, alpha, valid, H, W, _lib.stream_ptr(dev)), "gp_flow_resolve")
    return FlowResult(flow, alpha, valid.view(torch.bool))


def render_flow(view, gaussians, pipeline, iteration, time0, time1, view1=None, alpha_min=1e-3):
    """The flow of `view` from time0 to time1 -- and, with view1, into that camera at time1 (camera motion, as between render_video's
    interpolated poses) -- as a FlowResult.  Under no_grad: gaussians.forward at both times for the positions (_last_xyz_t, cloned),
    screen_flow, ONE render(view, ..., time=time0, override_color=rows) over a zero background of its own, whatever the scene's is,
    then resolve.  That is three deformation passes per frame (two here, one inside render()); they are not shared."""
    from .renderer import render
    view = view["cam"] if isinstance(view, dict) else view
    if view1 is not None:
        view1 = view1["cam"] if isinstance(view1, dict) else view1
    v0 = view_constants(view)
    dev = v0.viewmatrix.device
    t0 = torch.as_tensor(time0, dtype=torch.float32).reshape(-1)[:1].to(dev)
    t1 = torch.as_tensor(time1, dtype=torch.float32).reshape(-1)[:1].to(dev)
    with torch.no_grad():
        gaussians.forward(t0, iteration)
        xyz0 = gaussians._last_xyz_t.clone()
        gaussians.forward(t1, iteration)
        xyz1 = gaussians._last_xyz_t.clone()
        rows = screen_flow(xyz0, xyz1, v0, view1)
        out = render(view, gaussians, pipeline, torch.zeros(3, dtype=torch.float32, device=dev), time=t0, it=iteration, override_color=rows)
        return resolve(out["render"], alpha_min)


def colorize(flow, valid=None, max_flow=None, background=(0, 0, 0), return_scale=False):
    """[3, H, W] float32 in [0, 1]: the Middlebury colour wheel of flow [2, H, W] -- the hue is the direction, white is no motion, the
    saturation grows to the scale and magnitudes beyond it are dimmed by 0.75.  valid [H, W] bool or uint8: the other pixels, and
    those whose flow is not finite, take `background`.  max_flow: the scale; None or <= 0 takes the largest finite magnitude over the
    coloured pixels (1 where there is none or it is 0), found on the device in the same call -- nothing is read.  return_scale: also
    the [1] float32 device tensor of max_flow, or of that largest magnitude."""
    what = "colorize"
    flow, = _device_f32(what, ("flow", flow, "[2, H, W]", lambda t: t.dim() == 3 and t.shape[0] == 2))
    H, W = flow.shape[1:]
    _refuse(what, check_plane(H, W), H=H, W=W)
    valid = _mask_u8(what, "valid", valid, (H, W), flow.device)
    max_flow = 0.0 if max_flow is None else float(max_flow)
    if max_flow != max_flow:
        raise _lib.GpHipError(f"{what}: max_flow must not be NaN")
    bg = [float(v) for v in background]
    if len(bg) != 3:
        raise RuntimeError(f"{what}: background must hold three numbers")
    dev = flow.device
    out = torch.empty(3, H, W, dtype=torch.float32, device=dev)
    scale = torch.empty(1, dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        _lib.check(lib().gp_flow_colorize(flow, valid, max_flow, bg[0], bg[1], bg[2], scale, out, H, W, _lib.stream_ptr(dev)), "gp_flow_colorize")
    return (out, scale) if return_scale else out


def flow_metrics(flow, gt, mask=None):
    """[B, 8] float64 on the device (METRIC_NAMES): per image the count of pixels where mask != 0 and all four values are finite, their
    mean end-point error, the shares with an error above 1, 3 and 5 px, KITTI's Fl (above 3 px and above 5 % of |gt|), the mean |gt|,
    and 0.  A count of 0 gives a row of NaN.  flow, gt: [B, 2, H, W] float32, or [2, H, W] as B = 1; mask: [B, H, W] ([H, W]) bool or
    uint8.  Two calls give equal bytes, and row b of a batch is the B = 1 row."""
    what = "flow_metrics"
    ok = lambda t: t.dim() in (3, 4) and t.shape[-3] == 2           # noqa: E731
    flow, gt = _device_f32(what, ("flow", flow, "[B, 2, H, W]", ok), ("gt", gt, "[B, 2, H, W]", ok))
    if flow.dim() == 3:
        flow = flow[None]
        gt = gt[None] if gt.dim() == 3 else gt
        mask = mask[None] if torch.is_tensor(mask) and mask.dim() == 2 else mask
    if gt.shape != flow.shape or gt.device != flow.device:
        raise RuntimeError(f"{what}: gt must be a {list(flow.shape)} tensor on {flow.device}")
    B, _, H, W = flow.shape
    _refuse(what, check_batch(B, H, W), B=B, H=H, W=W)
    mask = _mask_u8(what, "mask", mask, (B, H, W), flow.device)
    dev = flow.device
    table = torch.empty(B, COLUMNS, dtype=torch.float64, device=dev)
    with _lib.on_device(dev):
        scratch = _lib.scratch(lib().gp_flow_metrics_scratch_bytes, B, H, W, device=dev)
        _lib.check(lib().gp_flow_metrics(flow, gt, mask, B, H, W, scratch, table, _lib.stream_ptr(dev)), "gp_flow_metrics")
    return table


def warp(image, flow):
    """out(p) = bilinear(image, p + flow(p)), taps outside the image contributing 0 and a sample position that is not finite giving 0:
    the backward warp of frame 1 into frame 0 by the flow 0 -> 1.  image [C, H, W] float32, flow [2, H, W]."""
    what = "warp"
    image, flow = _device_f32(what, ("image", image, "[C, H, W]", lambda t: t.dim() == 3),
                              ("flow", flow, "[2, H, W]", lambda t: t.dim() == 3 and t.shape[0] == 2))
    Cn, H, W = image.shape
    if tuple(flow.shape[1:]) != (H, W) or flow.device != image.device:
        raise RuntimeError(f"{what}: flow must be a [2, {H}, {W}] tensor on {image.device}")
    _refuse(what, check_warp(Cn, H, W), C=Cn, H=H, W=W)
    out = torch.empty_like(image)
    with _lib.on_device(image.device):
        _lib.check(lib().gp_flow_warp(image, flow, out, Cn, H, W, _lib.stream_ptr(image.device)), "gp_flow_warp")
    return out


# ---- Middlebury .flo files (host only) ----
def write_flo(path, flow):
    """flow [2, H, W] (a tensor anywhere, or an array) -> the bytes PIEH, int32 width, int32 height, then rows of interleaved
    little-endian float32 u, v.  A device tensor is read once."""
    a = flow.detach().cpu().numpy() if torch.is_tensor(flow) else np.asarray(flow)
    if a.ndim != 3 or a.shape[0] != 2:
        raise RuntimeError(f"write_flo: flow must be [2, H, W] (got {list(a.shape)})")
    H, W = a.shape[1:]
    with open(os.fspath(path), "wb") as fp:
        fp.write(FLO_TAG + struct.pack("<ii", W, H))
        fp.write(np.ascontiguousarray(a.transpose(1, 2, 0), dtype="<f4").tobytes())


def read_flo(path):
    """The [2, H, W] float32 CPU tensor of a .flo file; a wrong tag, sizes that are not positive or a length that is not the
    header's are refused."""
    raw = open(os.fspath(path), "rb").read()
    if len(raw) < 12 or raw[:4] != FLO_TAG:
        raise RuntimeError(f"read_flo: {path} does not begin with {FLO_TAG!r}")
    W, H = struct.unpack("<ii", raw[4:12])
    if W <= 0 or H <= 0 or len(raw) != 12 + 8 * W * H:
        raise RuntimeError(f"read_flo: {path} holds {len(raw) - 12} bytes of flow, its header says {W} x {H}")
    a = np.frombuffer(raw, "<f4", 2 * W * H, 12).reshape(H, W, 2).transpose(2, 0, 1)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
