"""TSDF fusion of depth renders and mesh extraction on the device (csrc/gp_tsdf.h, csrc/tsdf_kernels.hip): the views of one instant
fused into one truncated signed distance volume, and its zero surface as a watertight, coloured triangle mesh.

depth_ops stops at one loose point cloud per view.  TsdfVolume holds tsdf, weight and (optionally) colour on a regular grid of points;
integrate folds up to 16 views into it per launch (the volume is read and written once for all of them), extract runs marching
tetrahedra on the Kuhn split of every cell: one vertex per crossing lattice edge, numbered by an ordered scan, so that every triangle
sharing a vertex sees the same bits and two runs give equal bytes.  fuse renders the depth of every view at one time
(depth_ops.render_depth) and its colour (one ordinary render), integrates and extracts.  The header states every definition in full,
tests/tsdf_ref.py restates them in numpy and the tests pin that.

The depth is the rasterizer's alpha-weighted z-depth: the fused surface is where those depths agree, not a density level set.

HIP only: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import torch

from . import _lib, depth_ops

GP_TSDF_ABI_VERSION = 1             # csrc/gp_tsdf.h
MAX_VIEWS, TILE, EDGES = 16, 1024, 7
HEADER = "../gaussianprediction_amd/csrc/gp_tsdf.h"      # relative to include/: the header is not one of include/ 


class TsdfVolumeC(C.Structure):
    """gp_tsdf_volume."""
    _fields_ = [("tsdf", C.c_void_p), ("weight", C.c_void_p), ("color", C.c_void_p), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32),
                ("origin_x", C.c_float), ("origin_y", C.c_float), ("origin_z", C.c_float), ("voxel", C.c_float), ("trunc", C.c_float)]


class TsdfViewC(C.Structure):
    """gp_tsdf_view."""
    _fields_ = [("world_view", C.c_void_p), ("tanfovx", C.c_float), ("tanfovy", C.c_float)]


def _prototypes():
    i32, i64, f32, P, VOL, VIEW = C.c_int32, C.c_int64, C.c_float, _lib.Ptr, C.POINTER(TsdfVolumeC), C.POINTER(TsdfViewC)
    return {   # name: (restype, argtypes), as csrc/gp_tsdf.h declares them (tests/test_tsdf_host.py compares the two)
        "gp_tsdf_abi_version": (i32, []),
        "gp_tsdf_integrate": (i32, [VOL, P, P, P, VIEW, i32, i32, i32, f32, f32, f32, P]),
        "gp_tsdf_extract_scratch_bytes": (i64, [i32, i32, i32]),
        "gp_tsdf_extract_count": (i32, [VOL, f32, f32, P, P, P]),
        "gp_tsdf_extract_fill": (i32, [VOL, f32, P, P, P, P, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi(HEADER, "gp_tsdf_abi_version", GP_TSDF_ABI_VERSION, PROTOTYPES, register=False)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)

Mesh = namedtuple("Mesh", "vertices faces colors")           # [Nv, 3] float32, [Nf, 3] int32, [Nv, 3] float32 or None
View = namedtuple("View", "world_view tanfovx tanfovy")      # the [4, 4] tensor as a camera stores it, and the tangents of its half angles


# ---- refusals that need no device, as the library words them (None: accepted) ----
def check_dims(nx, ny, nz):
    nx, ny, nz = int(nx), int(ny), int(nz)
    if nx < 1 or ny < 1 or nz < 1:
        return "nx, ny and nz must be >= 1"
    if EDGES * nx * ny * nz >= 2 ** 31:
        return "7*nx*ny*nz must be below 2^31"
    return None


def check_grid(origin, voxel, trunc):
    vals = [float(v) for v in origin] + [float(voxel), float(trunc)]
    if not all(abs(v) < float("inf") for v in vals):
        return "origin, voxel and trunc must be finite"
    if not (vals[3] > 0 and vals[4] > 0):
        return "voxel and trunc must be > 0"
    return None


def _positive(what, **scalars):
    out = []
    for name, v in scalars.items():
        v = float(v)
        if not (0 < v < float("inf")):
            raise _lib.GpHipError(f"{what}: {', '.join(scalars)} must be finite and > 0 ({name} = {v})")
        out.append(v)
    return out


class TsdfVolume:
    """A truncated signed distance volume of dims = (nx, ny, nz) grid POINTS on a HIP device: point (i, j, k) lies at origin +
    (i, j, k) * voxel_size; .tsdf and .weight are [nz, ny, nx] float32, .color [3, nz, ny, nx] or None, all zeros at first.  trunc (the
    truncation distance, default 4 * voxel_size) scales the stored distance to [-1, 1]."""

    def __init__(self, origin, voxel_size, dims, trunc=None, color=True, device="cuda"):
        what = "TsdfVolume"
        origin = [float(v) for v in origin]
        dims = [int(v) for v in dims]
        if len(origin) != 3 or len(dims) != 3:
            raise RuntimeError(f"{what}: origin and dims must hold three numbers each")
        trunc = 4.0 * float(voxel_size) if trunc is None else float(trunc)
        for why in (check_dims(*dims), check_grid(origin, voxel_size, trunc)):
            if why:
                raise _lib.GpHipError(f"{what}: {why} (dims = {dims}, voxel_size = {voxel_size}, trunc = {trunc})")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"{what}: device is {device} -- HIP kernels only (no CPU fallback)")
        self.origin, self.voxel_size, self.dims, self.trunc, self.device = tuple(origin), float(voxel_size), tuple(dims), trunc, device
        nx, ny, nz = dims
        self.tsdf = torch.zeros(nz, ny, nx, dtype=torch.float32, device=device)
        self.weight = torch.zeros(nz, ny, nx, dtype=torch.float32, device=device)
        self.color = torch.zeros(3, nz, ny, nx, dtype=torch.float32, device=device) if color else None
        self.device = self.tsdf.device

    def _c(self):
        nx, ny, nz = self.dims
        return TsdfVolumeC(self.tsdf.data_ptr(), self.weight.data_ptr(), self.color.data_ptr() if self.color is not None else None, nx, ny, nz,
                           self.origin[0], self.origin[1], self.origin[2], self.voxel_size, self.trunc)

    def reset(self):
        """All zeros again: nothing seen."""
        self.tsdf.zero_()
        self.weight.zero_()
        if self.color is not None:
            self.color.zero_()

    def integrate(self, depth, valid, views, image=None, weight=1.0, weight_max=64.0, z_min=1e-3):
        """Fold views into the volume, in their order.  views: one camera (anything depth_ops.view_constants takes) or a list of V;
        depth: [V, H, W] float32 ([H, W] for one view), the z-depth of every pixel; valid: the same shape, bool or uint8, or None for
        every pixel; image: [V, 3, H, W] ([3, H, W]) float32, required iff the volume has colour.  A grid point in front of a view
        (z > z_min) that projects into a valid pixel of finite depth d > 0 and lies no more than trunc behind it takes
        min(1, (d - z) / trunc) into its running mean with `weight`; its own weight grows by `weight` up to weight_max.  More than 16
        views go in groups of 16, one launch each; nothing is read."""
        what = "TsdfVolume.integrate"
        views = list(views) if isinstance(views, (list, tuple)) and not isinstance(views, View) else [views]
        V = len(views)
        if V < 1:
            raise _lib.GpHipError(f"{what}: V must be >= 1 (V = 0)")
        if not torch.is_tensor(depth) or depth.dtype != torch.float32 or depth.dim() not in (2, 3):
            raise RuntimeError(f"{what}: depth must be a [V, H, W] float32 tensor")
        if depth.dim() == 2:
            depth = depth[None]
            valid = valid[None] if torch.is_tensor(valid) and valid.dim() == 2 else valid
            image = image[None] if torch.is_tensor(image) and image.dim() == 3 else image
        if not depth.is_cuda:
            raise RuntimeError(f"{what}: depth is on {depth.device} -- HIP kernels only (no CPU fallback)")
        if depth.shape[0] != V or depth.device != self.device:
            raise RuntimeError(f"{what}: depth must be [{V}, H, W] on {self.device} (got {list(depth.shape)} on {depth.device})")
        _, H, W = depth.shape
        depth_ops._refuse(what, depth_ops.check_plane(H, W), H=H, W=W)
        if (image is None) != (self.color is None):
            raise _lib.GpHipError(f"{what}: an image and a colour volume go together (both or neither)")
        if image is not None:
            if not torch.is_tensor(image) or image.dtype != torch.float32 or tuple(image.shape) != (V, 3, H, W) or image.device != self.device:
                raise RuntimeError(f"{what}: image must be a [{V}, 3, {H}, {W}] float32 tensor on {self.device}")
            image = image.detach().contiguous()
        valid = depth_ops._mask_u8(what, "valid", valid, (V, H, W), self.device)
        z_min, weight, weight_max = _positive(what, z_min=z_min, view_weight=weight, weight_max=weight_max)
        depth = depth.detach().contiguous()
        views = [_view(what, v["cam"] if isinstance(v, dict) else v, H, W, self.device) for v in views]
        vol = self._c()
        with _lib.on_device(self.device):
            for a in range(0, V, MAX_VIEWS):
                b = min(V, a + MAX_VIEWS)
                arr = (TsdfViewC * (b - a))(*[TsdfViewC(v.world_view.data_ptr(), v.tanfovx, v.tanfovy) for v in views[a:b]])
                _lib.check(lib().gp_tsdf_integrate(C.byref(vol), depth[a:b], None if valid is None else valid[a:b], None if image is None else image[a:b],
                                                   arr, b - a, H, W, z_min, weight, weight_max, _lib.stream_ptr(self.device)), "gp_tsdf_integrate")
        return self

    def extract(self, iso=0.0, min_weight=1.0):
        """Mesh(vertices [Nv, 3] float32, faces [Nf, 3] int32, colors [Nv, 3] float32 or None): the surface tsdf = iso over the cells
        whose eight corners have weight >= min_weight, by marching tetrahedra: one vertex per crossing lattice edge in ascending edge
        order, the triangles in ascending cell order, wound so that their normals point towards larger tsdf (out of the surface).
        The sizes are counted on the device; this function reads `counts` once per mesh -- the only read."""
        what = "TsdfVolume.extract"
        iso, min_weight = float(iso), float(min_weight)
        if not abs(iso) < float("inf"):
            raise _lib.GpHipError(f"{what}: iso must be finite")
        if min_weight != min_weight:
            raise _lib.GpHipError(f"{what}: min_weight must not be NaN")
        dev, vol = self.device, self._c()
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        with _lib.on_device(dev):
            scratch = _lib.scratch(lib().gp_tsdf_extract_scratch_bytes, *self.dims, device=dev)
            _lib.check(lib().gp_tsdf_extract_count(C.byref(vol), iso, min_weight, scratch, counts, _lib.stream_ptr(dev)), "gp_tsdf_extract_count")
            nv, nf = (int(v) for v in counts.tolist())          # (the one read)
            if nv < 0 or nf < 0:
                raise _lib.GpHipError(f"{what}: more than 2^31 - 1 vertices or triangles")
            vertices = torch.empty(nv, 3, dtype=torch.float32, device=dev)
            faces = torch.empty(nf, 3, dtype=torch.int32, device=dev)
            colors = torch.empty(nv, 3, dtype=torch.float32, device=dev) if self.color is not None else None
            if nv > 0 and nf > 0:                               # (a crossing edge lies in an active cell, which has a triangle on it)
                _lib.check(lib().gp_tsdf_extract_fill(C.byref(vol), iso, scratch, vertices, colors, faces, _lib.stream_ptr(dev)), "gp_tsdf_extract_fill")
        return Mesh(vertices, faces, colors)


def _view(what, view, H, W, device):
    """The View of a camera: its world_view_transform as it lies in memory ([4, 4] float32, contiguous, on the volume's device) and
    depth_ops.view_constants' tangents; a View passes as it is."""
    if isinstance(view, View):
        vm, tx, ty = view
    else:
        consts = depth_ops._view_for(what, view, H, W, device)
        vm, tx, ty = view.world_view_transform, consts.tanfovx, consts.tanfovy
    if not torch.is_tensor(vm) or vm.dtype != torch.float32 or tuple(vm.shape) != (4, 4):
        raise RuntimeError(f"{what}: world_view_transform must be a [4, 4] float32 tensor")
    if vm.device != device:
        raise RuntimeError(f"{what}: world_view_transform is on {vm.device}, the volume on {device} -- HIP kernels only (no CPU fallback)")
    tx, ty = float(tx), float(ty)
    if not (abs(tx) < float("inf") and abs(ty) < float("inf")):
        raise _lib.GpHipError(f"{what}: tanfovx and tanfovy must be finite")
    return View(vm.detach().contiguous(), tx, ty)


def fuse(views, gaussians, pipeline, iteration, time=None, bounds=None, voxel_size=None, resolution=256, alpha_min=0.5, trunc=None,
         background=None, color=True, weight=1.0, weight_max=64.0, iso=0.0, min_weight=1.0):
    """The Mesh of the scene at one time, fused from `views` (cameras, or dicts with "cam"): per view ONE depth_ops.render_depth at
    `time` (the view's own time where time is None) with alpha_min -- a pixel counts where the composite's alpha reaches it -- and,
    with color, one ordinary render() over `background` (default zeros) for the colours; the views go into a TsdfVolume in batches of
    16 and the mesh is extracted.  bounds: ((x0, y0, z0), (x1, y1, z1)); default the smallest and largest position of the Gaussians at
    that time (the first view's where time is None), padded by trunc: one read of six floats.  voxel_size: default the longest side
    of the bounds over `resolution`.  trunc: default 4 * voxel_size."""
    from .renderer import render
    what = "fuse"
    cams = [v["cam"] if isinstance(v, dict) else v for v in (views if isinstance(views, (list, tuple)) else [views])]
    if not cams:
        raise _lib.GpHipError(f"{what}: V must be >= 1 (V = 0)")
    vm = cams[0].world_view_transform
    if not torch.is_tensor(vm) or not vm.is_cuda:
        raise RuntimeError(f"{what}: the view is on {getattr(vm, 'device', None)} -- HIP kernels only (no CPU fallback)")
    dev = vm.device

    def time_of(cam):
        t = cam.time if time is None else time
        return None if t is None else torch.as_tensor(t, dtype=torch.float32).reshape(-1)[:1].to(dev)

    with torch.no_grad():
        given = bounds is not None
        if bounds is None:
            t0 = time_of(cams[0])
            xyz = gaussians.get_xyz if t0 is None else gaussians(t0, iteration)[0]
            lo, hi = torch.stack([xyz.min(dim=0).values, xyz.max(dim=0).values]).tolist()          # (the one read of six floats)
        else:
            lo, hi = [float(v) for v in bounds[0]], [float(v) for v in bounds[1]]
        side = max(h - l for l, h in zip(lo, hi))
        if voxel_size is None:
            if int(resolution) < 1 or not side > 0:
                raise _lib.GpHipError(f"{what}: resolution must be >= 1 and the bounds must have a positive side")
            voxel_size = side / int(resolution)
        voxel_size = float(voxel_size)
        trunc = 4.0 * voxel_size if trunc is None else float(trunc)
        if not given:                                 # (the Gaussians' own box is padded by trunc; given bounds are taken as they are)
            lo, hi = [v - trunc for v in lo], [v + trunc for v in hi]
        dims = [max(1, int((h - l) / voxel_size) + 2) if voxel_size > 0 else 0 for l, h in zip(lo, hi)]
        volume = TsdfVolume(lo, voxel_size, dims, trunc=trunc, color=color, device=dev)
        bg = torch.zeros(3, dtype=torch.float32, device=dev) if background is None else background
        for a in range(0, len(cams), MAX_VIEWS):
            group = cams[a:a + MAX_VIEWS]
            depths, valids, images = [], [], []
            for cam in group:
                t = time_of(cam)
                res = depth_ops.render_depth(cam, gaussians, pipeline, iteration, time=t, alpha_min=alpha_min)
                depths.append(res.depth)
                valids.append(res.valid)
                if color:
                    images.append(render(cam, gaussians, pipeline, bg, time=t, it=iteration)["render"].detach())
            volume.integrate(torch.stack(depths), torch.stack(valids), group, image=torch.stack(images) if color else None, weight=weight,
                             weight_max=weight_max)
        return volume.extract(iso=iso, min_weight=min_weight)
