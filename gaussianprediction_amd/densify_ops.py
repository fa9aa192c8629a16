"""Densify (clone + split), opacity reset and prune on the device (include/gp_densify.h, csrc/densify_kernels.hip): the per-view
statistics in one launch, one plan over the state before any of the three operations, one apply that writes every output tensor.

  [REF train.py:166-167, scene/gaussian_model.py:755-760]    stats()
  [REF scene/gaussian_model.py:663-718, 745-753]              plan()
  [REF scene/gaussian_model.py:547-661]                       apply()

Nothing here reads the device; the caller reads the status block when it needs the row count.  HIP only: CPU tensors raise."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

GP_DENSIFY_ABI_VERSION = 1          # include/gp_densify.h
BLOCK = 256                         # rows per workgroup of the plan and the apply
MAX_TENSORS = 8
MAX_ROWS = 1 << 30
DENSIFY, RESET, PRUNE, SCREEN = 1, 2, 4, 8
STATUS_WORDS = 8
ST_CLONED, ST_SPLIT, ST_PRUNED, ST_ROWS, ST_BASE = 0, 1, 2, 3, 4
ROLE_NONE, ROLE_XYZ, ROLE_SCALING, ROLE_ROTATION, ROLE_OPACITY = 0, 1, 2, 3, 4
ROLES = {"xyz": ROLE_XYZ, "scaling": ROLE_SCALING, "rotation": ROLE_ROTATION, "opacity": ROLE_OPACITY}


class DensifyTensorC(C.Structure):
    """gp_densify_tensor."""
    _fields_ = [("in_", C.c_void_p), ("in_exp_avg", C.c_void_p), ("in_exp_avg_sq", C.c_void_p),
                ("out", C.c_void_p), ("out_exp_avg", C.c_void_p), ("out_exp_avg_sq", C.c_void_p),
                ("width", C.c_int32), ("role", C.c_int32)]


def _prototypes():
    i32, i64, u32, f32, P = C.c_int32, C.c_int64, C.c_uint32, C.c_float, _lib.Ptr
    return {   # name: (restype, argtypes), as include/gp_densify.h declares them (tests/test_densify_plan_host.py compares the two)
        "gp_densify_abi_version": (i32, []),
        "gp_densify_stats": (i32, [i64, P, P, P, P, P, P, P, P]),
        "gp_densify_scratch_bytes": (i64, [i64]),
        "gp_densify_plan": (i32, [i64, P, P, P, P, P, f32, f32, f32, f32, f32, u32, P, P, P]),
        "gp_densify_apply": (i32, [i64, i32, P, P, P, P, i64, u32, P, P, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi("gp_densify.h", "gp_densify_abi_version", GP_DENSIFY_ABI_VERSION, PROTOTYPES)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)


def _device_f32(t, name, shape=None, dtype=torch.float32):
    if not torch.is_tensor(t):
        raise TypeError(f"densify_ops: {name} must be a tensor (got {type(t).__name__})")
    if not t.is_cuda:
        raise RuntimeError(f"densify_ops: {name} is on {t.device} -- HIP kernels only (no CPU fallback)")
    if t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError(f"densify_ops: {name} must be a contiguous {dtype} tensor (got {t.dtype}, contiguous={t.is_contiguous()})")
    if shape is not None and t.numel() != shape:
        raise RuntimeError(f"densify_ops: {name} must hold {shape} elements (got {tuple(t.shape)})")
    return t


def flags_of(do_densify, do_reset, do_prune, max_screen_size):
    return (DENSIFY if do_densify else 0) | (RESET if do_reset else 0) | (PRUNE if do_prune else 0) | (SCREEN if max_screen_size else 0)


def stats(visible, radii, grad, max_radii2D, accum, denom, accum_max):
    """The statistics of one view, in place, for the rows with visible != 0.  visible: [N] bool or uint8; radii: [N] int32; grad: [N,3]
    (the screen-space gradient); the four statistics: N floats each.  One launch, nothing read back."""
    n = radii.numel()
    vis = visible.view(torch.uint8) if torch.is_tensor(visible) and visible.dtype == torch.bool else visible
    _device_f32(vis, "visible", n, torch.uint8)
    _device_f32(radii, "radii", n, torch.int32)
    _device_f32(grad, "grad", 3 * n)
    for name, t in (("max_radii2D", max_radii2D), ("accum", accum), ("denom", denom), ("accum_max", accum_max)):
        _device_f32(t, name, n)
    dev = radii.device
    with _lib.on_device(dev):
        _lib.check(lib().gp_densify_stats(n, vis, radii, grad, max_radii2D, accum, denom, accum_max, _lib.stream_ptr(dev)), "gp_densify_stats")


def plan(accum, denom, max_radii2D, scaling, opacity, grad_threshold, dense_extent, min_opacity, max_screen_size, world_extent, *,
         do_densify, do_reset, do_prune=True):
    """-> (scratch, status, flags): the keep bytes and scanned block counts (opaque, for apply()) and the status block, 8 int32 words
    on the device: rows selected for cloning, split sources, pruned rows, output rows, the four segment bases.  max_screen_size None
    (or 0) switches the screen- and world-size tests off, as in prune()."""
    if not float(grad_threshold) > 0:
        raise ValueError(f"densify plan: grad_threshold must be > 0 (got {grad_threshold}): the split pass relies on the zero-padded "
                         "gradient of cloned rows failing `>= grad_threshold`")
    n = opacity.numel()
    for name, t, k in (("accum", accum, 1), ("denom", denom, 1), ("max_radii2D", max_radii2D, 1), ("scaling", scaling, 3), ("opacity", opacity, 1)):
        _device_f32(t, name, k * n)
    dev, l = opacity.device, lib()
    scratch = _lib.scratch(l.gp_densify_scratch_bytes, n, device=dev)
    status = torch.empty(STATUS_WORDS, dtype=torch.int32, device=dev)
    flags = flags_of(do_densify, do_reset, do_prune, max_screen_size)
    with _lib.on_device(dev):
        _lib.check(l.gp_densify_plan(n, accum, denom, max_radii2D, scaling, opacity, float(grad_threshold), float(dense_extent),
                                     float(min_opacity), float(max_screen_size or 0.0), float(world_extent), flags, scratch, status,
                                     _lib.stream_ptr(dev)), "gp_densify_plan")
    return scratch, status, flags


def apply(n, entries, normals, stats_in, stats_out, out_rows, flags, scratch, status):
    """entries: up to eight (name, tensor in, (exp_avg, exp_avg_sq) in or None, tensor out, (exp_avg, exp_avg_sq) out or None); the
    name gives the role (ROLES).  stats_in / stats_out: (accum, denom, accum_max, max_radii2D).  One launch."""
    if len(entries) > MAX_TENSORS:
        raise ValueError(f"densify apply: at most {MAX_TENSORS} per-Gaussian tensors (got {len(entries)})")
    table = (DensifyTensorC * len(entries))()
    for e, (name, t_in, mom_in, t_out, mom_out) in zip(table, entries):
        if t_in.numel() % n:
            raise RuntimeError(f"densify apply: {name} holds {t_in.numel()} elements, no multiple of {n} rows")
        w = t_in.numel() // n
        _device_f32(t_in, name)
        _device_f32(t_out, name + " (out)", out_rows * w)
        e.in_, e.out, e.width, e.role = t_in.data_ptr(), t_out.data_ptr(), w, ROLES.get(name, ROLE_NONE)
        if (mom_in is None) != (mom_out is None):
            raise ValueError(f"densify apply: {name} needs its moments on both sides or on neither")
        if mom_in is not None:
            for k, (a, b) in enumerate(zip(mom_in, mom_out)):
                _device_f32(a, f"{name} moment {k}", n * w)
                _device_f32(b, f"{name} moment {k} (out)", out_rows * w)
            e.in_exp_avg, e.in_exp_avg_sq = mom_in[0].data_ptr(), mom_in[1].data_ptr()
            e.out_exp_avg, e.out_exp_avg_sq = mom_out[0].data_ptr(), mom_out[1].data_ptr()
    if normals is not None:
        _device_f32(normals, "normals", 6 * n)
    for k, (a, b) in enumerate(zip(stats_in, stats_out)):
        _device_f32(a, f"statistic {k}", n)
        _device_f32(b, f"statistic {k} (out)", out_rows)
    arr = lambda ts: (C.c_void_p * 4)(*[t.data_ptr() for t in ts])      # noqa: E731
    dev = scratch.device
    with _lib.on_device(dev):
        _lib.check(lib().gp_densify_apply(n, len(entries), table, normals, arr(stats_in), arr(stats_out), out_rows, flags, scratch, status,
                                          _lib.stream_ptr(dev)), "gp_densify_apply")
