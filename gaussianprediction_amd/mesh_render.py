"""A triangle rasterizer on the device (csrc/gp_mesh_render.h, csrc/mesh_render_kernels.hip): the meshes of tsdf_ops, mesh_ops and
mesh_simplify as pictures -- the winning face, the depth, the barycentrics, interpolated attributes, face normals and a
headlight-shaded view -- and, through depth_ops.depth_metrics, their agreement with the depth render they were fused from.

A lane per vertex snaps it to 8 sub-pixel bits once per view; a lane per face decides coverage in 64-bit integers and sends
(depth bits << 32 | face) through a 64-bit atomic minimum, so the nearest surface wins, ties go to the smaller face number, and no
result depends on the order of the triangles; a lane per pixel resolves.  There is no clipping: a triangle with a corner at or
behind z_near, or beyond the guard band of 2^15 pixels, is dropped whole and counted.  The header states every definition in full,
tests/mesh_render_ref.py restates them in numpy and the tests pin that, bit for bit.

HIP only: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib, depth_ops
from .mesh_ops import _faces, _rows
from .tsdf_ops import View

GP_MESH_RENDER_ABI_VERSION = 1      # csrc/gp_mesh_render.h
NARROW_MAX, SPLIT, MAX_SIZE, MAX_CHANNELS, SUBPIXEL, GUARD = 64, 16, 16384, 8, 256, 2 ** 23
CULL = {"none": 0, "back": 1, "front": 2}
STATUS, DRAWN, NEAR, OUT_OF_RANGE, DEGENERATE, CULLED, WIDE, COUNT_WORDS = 0, 1, 2, 3, 4, 5, 6, 8
STAT_NAMES = ("status", "drawn", "near", "out_of_range", "degenerate", "culled", "wide")
MODES = ("shaded", "color", "normals", "depth")
GREY = 0.7                           # the colour of a mesh without colours
HEADER = "../gaussianprediction_amd/csrc/gp_mesh_render.h"        # relative to include/: the header is not one of include/ 


def _prototypes():
    i32, i64, f32, P = C.c_int32, C.c_int64, C.c_float, _lib.Ptr
    return {   # name: (restype, argtypes), as csrc/gp_mesh_render.h declares them (tests/test_mesh_render_host.py compares the two)
        "gp_mesh_render_abi_version": (i32, []),
        "gp_mesh_render_scratch_bytes": (i64, [i64, i64, i32, i32]),
        "gp_mesh_render_rasterize": (i32, [P, P, i64, i64, P, f32, f32, i32, i32, f32, i32, P, P, P, P]),
        "gp_mesh_render_resolve": (i32, [P, i64, i64, i32, i32, P, P, P, P, P, P]),
        "gp_mesh_render_interpolate": (i32, [P, i32, P, i64, i64, i32, i32, P, P, P, P, P, P, P]),
        "gp_mesh_render_normals": (i32, [P, P, i64, i64, P, f32, f32, i32, i32, P, P, P, P, P, P]),
        "gp_mesh_render_shade": (i32, [P, P, P, P, f32, f32, i32, i32, f32, f32, f32, f32, P, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi(HEADER, "gp_mesh_render_abi_version", GP_MESH_RENDER_ABI_VERSION, PROTOTYPES, register=False)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)


class MeshRaster:
    """What rasterize leaves, all [H, W] on the device: face int32 (-1: none), depth float32 (0: none), valid bool, bary [3, H, W]
    float32 in the face's stored corner order, coverage int32 (the counting samples of every pixel) or None.  stats: {"status",
    "drawn", "near", "out_of_range", "degenerate", "culled", "wide"} -- the ONE read of the device, made when stats is first asked for
    and never otherwise."""
    __slots__ = ("face", "depth", "valid", "bary", "coverage", "_counts", "_stats", "_scratch", "_faces", "_nv")

    def __init__(self, face, depth, valid, bary, coverage, counts, scratch, faces, nv):
        self.face, self.depth, self.valid, self.bary, self.coverage = face, depth, valid, bary, coverage
        self._counts, self._stats, self._scratch, self._faces, self._nv = counts, None, scratch, faces, nv

    @property
    def stats(self):
        if self._stats is None:
            self._stats = dict(zip(STAT_NAMES, (int(v) for v in self._counts.tolist())))          # (the one read)
        return self._stats


def check_size(H, W):
    """The library's refusal of an image size, as it words it (None: accepted)."""
    if int(H) <= 0 or int(W) <= 0:
        return "H and W must be > 0"
    if int(H) > MAX_SIZE or int(W) > MAX_SIZE:
        return "H and W must be <= 16384"
    return None


def _view(what, view, size, device):
    """(world_view [4, 4] on `device`, tanfovx, tanfovy, H, W) of a camera, or of a tsdf_ops.View with size = (H, W)."""
    view = view["cam"] if isinstance(view, dict) else view
    if isinstance(view, View):
        if size is None:
            raise RuntimeError(f"{what}: a tsdf_ops.View carries no image size: pass size=(H, W)")
        vm, tx, ty = view
        H, W = int(size[0]), int(size[1])
    else:
        vm = view.world_view_transform
        tx, ty = math.tan(float(view.FoVx) * 0.5), math.tan(float(view.FoVy) * 0.5)
        H, W = (int(view.image_height), int(view.image_width)) if size is None else (int(size[0]), int(size[1]))
    if not torch.is_tensor(vm) or vm.dtype != torch.float32 or tuple(vm.shape) != (4, 4):
        raise RuntimeError(f"{what}: world_view_transform must be a [4, 4] float32 tensor")
    if not vm.is_cuda or (device is not None and vm.device != device):
        raise RuntimeError(f"{what}: world_view_transform is on {vm.device}" + (f", the mesh on {device}" if device is not None else "") + " -- HIP kernels only (no CPU fallback)")
    tx, ty = float(tx), float(ty)
    if not (abs(tx) < math.inf and abs(ty) < math.inf):
        raise _lib.GpHipError(f"{what}: tanfovx and tanfovy must be finite")
    why = check_size(H, W)
    if why:
        raise _lib.GpHipError(f"{what}: {why} (H = {H}, W = {W})")
    return vm.detach().contiguous(), tx, ty, H, W


def _mesh(what, mesh):
    vertices, faces = mesh[0], mesh[1]
    if not torch.is_tensor(vertices) or vertices.dim() != 2:
        raise RuntimeError(f"{what}: vertices must be an [Nv, 3] float32 tensor")
    nv = vertices.shape[0]
    faces = _faces(what, faces, nv)
    return _rows(what, "vertices", vertices, nv, faces.device, 3), faces, nv


def _raster(what, raster, H=None, W=None):
    if not isinstance(raster, MeshRaster):
        raise RuntimeError(f"{what}: raster must be a MeshRaster (of rasterize)")
    if H is not None and tuple(raster.face.shape) != (H, W):
        raise RuntimeError(f"{what}: the raster is {list(raster.face.shape)}, the view {[H, W]}")
    return raster


def rasterize(mesh, view, z_near=0.01, cull="none", counts=False, size=None):
    """MeshRaster of `mesh` (a tsdf_ops.Mesh, or any (vertices [Nv, 3] float32, faces [Nf, 3] int32, ...)) seen from `view`: a camera
    (world_view_transform, FoVx, FoVy, image_width, image_height), or a tsdf_ops.View with size=(H, W).  z_near: a face with a corner
    at P_z <= z_near is dropped whole (no clipping), as is one with a corner more than 2^15 pixels from the origin.  cull: "none",
    "back" (drops the faces whose normal (b - a) x (c - a) points away from the camera) or "front".  counts: also the coverage plane,
    the number of counting samples per pixel.  An empty mesh gives an empty picture.  Nothing is read: a face index outside [0, Nv)
    drops that face and shows in stats["status"], which reads the device when first looked at."""
    what = "rasterize"
    z_near = float(z_near)
    if not (math.isfinite(z_near) and z_near > 0):
        raise _lib.GpHipError(f"{what}: z_near must be finite and > 0 (z_near = {z_near:g})")
    if cull not in CULL:
        raise _lib.GpHipError(f"{what}: cull must be \"none\", \"back\" or \"front\" (cull = {cull!r})")
    vertices, faces, nv = _mesh(what, mesh)
    dev = faces.device
    vm, tx, ty, H, W = _view(what, view, size, dev)
    nf = faces.shape[0]
    words = torch.empty(COUNT_WORDS, dtype=torch.int32, device=dev)
    face = torch.empty(H, W, dtype=torch.int32, device=dev)
    depth = torch.empty(H, W, dtype=torch.float32, device=dev)
    valid = torch.empty(H, W, dtype=torch.uint8, device=dev)
    bary = torch.empty(3, H, W, dtype=torch.float32, device=dev)
    coverage = torch.empty(H, W, dtype=torch.int32, device=dev) if counts else None
    with _lib.on_device(dev):
        st = _lib.stream_ptr(dev)
        scratch = _lib.scratch(lib().gp_mesh_render_scratch_bytes, nv, nf, H, W, device=dev)
        _lib.check(lib().gp_mesh_render_rasterize(vertices, faces, nv, nf, vm, tx, ty, H, W, z_near, CULL[cull], scratch, coverage, words, st), "gp_mesh_render_rasterize")
        _lib.check(lib().gp_mesh_render_resolve(faces, nv, nf, H, W, scratch, face, depth, valid, bary, st), "gp_mesh_render_resolve")
    return MeshRaster(face, depth, valid.view(torch.bool), bary, coverage, words, scratch, faces, nv)


def interpolate(raster, attributes, background=0):
    """[C, H, W] float32: the rows of attributes [Nv, C] float32, 1 <= C <= 8, interpolated over the winning face of every pixel,
    perspective-correct; `background` (a number, or C of them) where no face covers the pixel."""
    what = "interpolate"
    raster = _raster(what, raster)
    dev = raster.face.device
    attributes = _rows(what, "attributes", attributes, raster._nv, dev)
    k = attributes.shape[1]
    if not 1 <= k <= MAX_CHANNELS:
        raise _lib.GpHipError(f"{what}: C must be 1 .. {MAX_CHANNELS} (C = {k})")
    bg = [float(background)] * k if not hasattr(background, "__len__") else [float(v) for v in background]
    if len(bg) != k:
        raise RuntimeError(f"{what}: background must hold one number or {k}")
    H, W = raster.face.shape
    out = torch.empty(k, H, W, dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        _lib.check(lib().gp_mesh_render_interpolate(attributes, k, raster._faces, raster._nv, raster._faces.shape[0], H, W, raster._scratch, raster.face,
                                                    raster.valid.view(torch.uint8), raster.bary, (C.c_float * k)(*bg), out, _lib.stream_ptr(dev)),
                   "gp_mesh_render_interpolate")
    return out


def normals(raster, mesh, view, size=None):
    """(normals [3, H, W] float32, nvalid [H, W] bool): the unit normal of the winning face of every pixel in camera space, from the
    camera points of its corners, turned to face the camera as depth_ops.normals turns its own (a fronto-parallel surface has
    n_z = -1): depth_ops.normals_image colours it.  Zeros and False where no face covers the pixel or the face has no area."""
    what = "normals"
    vertices, faces, nv = _mesh(what, mesh)
    dev = faces.device
    vm, tx, ty, H, W = _view(what, view, size, dev)
    raster = _raster(what, raster, H, W)
    out = torch.empty(3, H, W, dtype=torch.float32, device=dev)
    nvalid = torch.empty(H, W, dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.check(lib().gp_mesh_render_normals(vertices, faces, nv, faces.shape[0], vm, tx, ty, H, W, raster.face, raster.depth, raster.valid.view(torch.uint8), out,
                                                nvalid, _lib.stream_ptr(dev)), "gp_mesh_render_normals")
    return out, nvalid.view(torch.bool)


def shade(color, normals, raster, view, ambient=0.3, background=(0, 0, 0), size=None):
    """[3, H, W] float32: color [3, H, W] lit by a headlight at the camera, L = ambient + (1 - ambient) * |n . P| / |P| with P the
    pixel's point at the mesh depth; `background` where there is no normal.  normals: what normals() returned -- the pair, or its
    [3, H, W] tensor alone (every covered pixel then counts as lit)."""
    what = "shade"
    raster = _raster(what, raster)
    dev = raster.face.device
    n, nvalid = normals if isinstance(normals, (tuple, list)) else (normals, raster.valid)
    _, tx, ty, H, W = _view(what, view, size, dev)
    _raster(what, raster, H, W)
    ok = lambda t: tuple(t.shape) == (3, H, W)          # noqa: E731
    color, n = depth_ops._device_f32(what, ("color", color, f"[3, {H}, {W}]", ok), ("normals", n, f"[3, {H}, {W}]", ok))
    nvalid = depth_ops._mask_u8(what, "nvalid", nvalid, (H, W), dev)
    bg = depth_ops._background(what, background)
    ambient = float(ambient)
    if not math.isfinite(ambient):
        raise _lib.GpHipError(f"{what}: ambient must be finite")
    if color.device != dev or n.device != dev:
        raise RuntimeError(f"{what}: color and normals must be on {dev}")
    out = torch.empty(3, H, W, dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        _lib.check(lib().gp_mesh_render_shade(color, n, nvalid, raster.depth, tx, ty, H, W, ambient, bg[0], bg[1], bg[2], out, _lib.stream_ptr(dev)), "gp_mesh_render_shade")
    return out


def render_mesh(mesh, view, mode="shaded", background=(0, 0, 0), z_near=0.01, cull="none", ambient=0.3, size=None, raster=None, **colorize):
    """[3, H, W] float32, the picture of `mesh` from `view`.  mode "shaded": the vertex colours under the headlight of shade();
    "color": the vertex colours alone; "normals": depth_ops.normals_image of the face normals; "depth": depth_ops.colorize of the
    mesh depth, with its options near, far, lut and return_range as keywords, and depth_mode= for its own `mode` ("disparity" or
    "depth").  A mesh without colours is grey.  `background` everywhere else.  raster: a MeshRaster of the same mesh and view, where the caller has one.  Nothing is read."""
    what = "render_mesh"
    if mode not in MODES:
        raise RuntimeError(f"{what}: mode = {mode!r} must be one of {', '.join(repr(m) for m in MODES)}")
    if mode != "depth" and colorize:
        raise RuntimeError(f"{what}: {sorted(colorize)} are options of mode 'depth'")
    bg = depth_ops._background(what, background)
    r = rasterize(mesh, view, z_near=z_near, cull=cull, size=size) if raster is None else _raster(what, raster)
    if mode == "depth":
        if "depth_mode" in colorize:
            colorize["mode"] = colorize.pop("depth_mode")
        return depth_ops.colorize(r.depth, r.valid, background=bg, **colorize)
    if mode == "normals":
        n, nvalid = normals(r, mesh, view, size=size)
        return depth_ops.normals_image(n, nvalid, background=bg)
    colors = mesh[2] if len(mesh) > 2 else None
    if colors is None:
        colors = torch.full((r._nv, 3), GREY, dtype=torch.float32, device=r.face.device)
    colour = interpolate(r, colors, background=bg)
    if mode == "color":
        return colour
    return shade(colour, normals(r, mesh, view, size=size), r, view, ambient=ambient, background=bg, size=size)


def agreement(raster, depth_result):
    """How the mesh agrees with a depth render of the same camera (a depth_ops.DepthResult): depth_ops.depth_metrics(pred = the mesh
    depth, gt = the render's depth, mask = both valid) as a dict by depth_ops.METRIC_NAMES, plus "iou", the intersection over the
    union of the two valid masks (NaN where both are empty), and "pixels", H * W.  One read of the device."""
    what = "agreement"
    raster = _raster(what, raster)
    depth, valid = depth_result.depth, depth_result.valid
    if not torch.is_tensor(depth) or tuple(depth.shape) != tuple(raster.depth.shape) or depth.device != raster.depth.device:
        raise RuntimeError(f"{what}: the depth render must be {list(raster.depth.shape)} on {raster.depth.device}")
    both, either = raster.valid & valid.bool(), raster.valid | valid.bool()
    table = depth_ops.depth_metrics(raster.depth, depth, mask=both)
    sums = torch.stack([both.sum(), either.sum()]).to(torch.float64)
    row = torch.cat([table[0], sums]).tolist()                                          # (the one read)
    out = dict(zip(depth_ops.METRIC_NAMES, row[:len(depth_ops.METRIC_NAMES)]))
    out["iou"] = row[-2] / row[-1] if row[-1] > 0 else float("nan")
    out["pixels"] = int(raster.depth.numel())
    return out
