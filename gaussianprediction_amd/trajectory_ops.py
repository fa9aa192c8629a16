"""Motion trajectories drawn on the device (csrc/gp_trajectory.h, csrc/trajectory_kernels.hip): the polyline each of P points walks over
S steps, projected into one view, later lines over earlier ones.

  [REF eval.py:38-73]                      project_trajectory: per step, up to H*W cv2.line calls in a Python loop
  [REF utils/camera_utils.py:195-267]      transpose and pi, the projection

cv2 is not installed where this was written, so PARITY WITH cv2.line IS UNPINNED: the rasterisation is this project's own definition
(the header states it in full; tests/trajectory_ref.py restates it in numpy and the tests pin that, bit for bit).  In short: float32
projection with the reference's operations in the reference's order and one focal length for both axes; a point is drawable where its
u and v are finite and below 2^20 in magnitude (the reference's cast of anything else is undefined in numpy), and its pixel is the
truncation; a segment is the 8-connected Bresenham line started at the EARLIER pixel, both ends included, clipped exactly to the image;
step s of point j claims pixels with key s*P + j + 1 and the largest key owns a pixel -- the reference's overwrite order -- so two runs
give equal bytes.  The reference has no depth test and neither has the default; `min_depth` adds one.

The work streams: a TrajectoryCanvas keeps the previous step's pixels [P, 2] and the owner image [H, W]; nothing of size S*P exists.
HIP only: CPU tensors raise."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .cameras import fov2focal

GP_TRAJ_ABI_VERSION = 1             # csrc/gp_trajectory.h
NOT_DRAWABLE = -2 ** 31             # both members of the stored pixel of a point that is not drawable
COORD_LIMIT = 2 ** 20
HEADER = "../gaussianprediction_amd/csrc/gp_trajectory.h"      # relative to include/: the header is not one of include/ 


class TrajViewC(C.Structure):
    """gp_traj_view."""
    _fields_ = [("R", C.c_float * 9), ("t", C.c_float * 3), ("f", C.c_float), ("cx", C.c_float), ("cy", C.c_float)]


def _prototypes():
    i32, i64, f32, P = C.c_int32, C.c_int64, C.c_float, _lib.Ptr
    return {   # name: (restype, argtypes), as csrc/gp_trajectory.h declares them (tests/test_trajectory_host.py compares the two)
        "gp_traj_abi_version": (i32, []),
        "gp_traj_step": (i32, [C.POINTER(TrajViewC), P, P, i64, i64, i64, P, P, i32, i32, f32, P]),
        "gp_traj_resolve": (i32, [P, P, i64, P, P, i32, i32, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi(HEADER, "gp_traj_abi_version", GP_TRAJ_ABI_VERSION, PROTOTYPES, register=False)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)


def view_constants(view, H, W):
    """The gp_traj_view of a camera [REF eval.py:48-56]: R = view.R.T and t = view.T as float32, f = fov2focal(view.FoVx, W) for both
    axes, cx = W / 2, cy = H / 2, each rounded to float32 once."""
    R = np.asarray(view.R, dtype=np.float64).T.astype(np.float32).reshape(9)
    t = np.asarray(view.T, dtype=np.float64).astype(np.float32).reshape(3)
    c = TrajViewC()
    c.R[:], c.t[:] = R.tolist(), t.tolist()
    c.f, c.cx, c.cy = (float(np.float32(v)) for v in (fov2focal(float(view.FoVx), W), W / 2, H / 2))
    return c


def default_colors(P, seed=0):
    """[P, 3] float32 on the host: torch.rand from a generator seeded with `seed` (the reference's are unseeded np.random.rand)."""
    return torch.rand(int(P), 3, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32)


def check_sizes(N, P, s, H, W, has_idx):
    """The refusals of gp_traj_step that need no device, as the library words them (None: accepted)."""
    N, P, s, H, W = int(N), int(P), int(s), int(H), int(W)
    if N < 0 or P < 0 or s < 0:
        return "N, P and s must be >= 0"
    if H <= 0 or W <= 0:
        return "H and W must be > 0"
    if H * W >= 2 ** 31:
        return "H*W must be below 2^31"
    if P >= 2 ** 31:
        return "P must be below 2^31"
    if (s + 1) * P >= 2 ** 32 - 1:
        return "S*P must be below 2^32 - 1 (the keys are 32 bits wide)"
    if not has_idx and N < P:
        return "without idx, xyz must hold at least P rows"
    if has_idx and P > 0 and N == 0:
        return "idx given but xyz holds no row"
    return None


class TrajectoryCanvas:
    """The drawing of P trajectories into one view.  view: a camera with R, T, FoVx (and image_height / image_width where H / W are not
    given).  colors: [P, 3] float32, default default_colors(P, seed).  min_depth: None for the reference's behaviour (no depth test), or
    the camera-space depth at or below which a point is not drawable.

      .step(xyz, idx=None)   xyz [N, 3] float32 on the device; idx [P] int32 rows of xyz (None: the first P rows).  Step 0 only stores
                             the pixels; every later step draws from the stored pixels to the new ones.  A row outside xyz is not drawable.
      .image(base=None, layout="hwc")   the owners' colours over `base` [3, H, W] (or over zero), as [H, W, 3] or [3, H, W] float32
      .owner                 [H, W] uint32: 0 where nothing was drawn, else s*P + j + 1 of the last claim (torch implements few
                             operators for uint32: compare it, or read it with .cpu().numpy())
      .px                    [P, 2] int32: the pixels of the last step (NOT_DRAWABLE twice for a point that is not drawable)
    P == 0, or fewer than two steps, gives the base (or zero) without a launch.  Nothing is read from the device."""

    def __init__(self, view, P, device, H=None, W=None, colors=None, seed=0, min_depth=None):
        self.H = int(view.image_height if H is None else H)
        self.W = int(view.image_width if W is None else W)
        self.P = int(P)
        why = check_sizes(self.P, self.P, 0, self.H, self.W, False)
        if why:
            raise _lib.GpHipError(f"TrajectoryCanvas: {why} (P = {self.P}, H = {self.H}, W = {self.W})")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"TrajectoryCanvas: device = {self.device} -- HIP kernels only (no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if colors is None:
            colors = default_colors(self.P, seed)
        if not torch.is_tensor(colors) or tuple(colors.shape) != (self.P, 3):
            raise RuntimeError(f"TrajectoryCanvas: colors must be a [{self.P}, 3] tensor")
        self.view = view_constants(view, self.H, self.W)
        self.min_depth = float("nan") if min_depth is None else float(min_depth)
        self.colors = colors.detach().to(self.device, torch.float32).contiguous()
        self.px = torch.full((self.P, 2), NOT_DRAWABLE, dtype=torch.int32, device=self.device)
        self._owner = torch.zeros(self.H, self.W, dtype=torch.int32, device=self.device)
        self.steps = 0

    @property
    def owner(self):
        return self._owner.view(torch.uint32)

    def step(self, xyz, idx=None):
        if not torch.is_tensor(xyz) or xyz.dtype != torch.float32 or xyz.dim() != 2 or xyz.shape[1] != 3:
            raise RuntimeError("TrajectoryCanvas.step: xyz must be a [N, 3] float32 tensor")
        if idx is not None and (not torch.is_tensor(idx) or idx.dtype != torch.int32 or tuple(idx.shape) != (self.P,)):
            raise RuntimeError(f"TrajectoryCanvas.step: idx must be a [{self.P}] int32 tensor")
        for name, t in (("xyz", xyz), ("idx", idx)):
            if t is not None and t.device != self.device:
                raise RuntimeError(f"TrajectoryCanvas.step: {name} is on {t.device}, the canvas on {self.device} -- HIP kernels only (no CPU fallback)")
        why = check_sizes(xyz.shape[0], self.P, self.steps, self.H, self.W, idx is not None)
        if why:
            raise _lib.GpHipError(f"TrajectoryCanvas.step: {why} (N = {xyz.shape[0]}, P = {self.P}, s = {self.steps})")
        if self.P > 0:
            xyz = xyz.detach().contiguous()
            idx = None if idx is None else idx.contiguous()
            with _lib.on_device(self.device):
                _lib.check(lib().gp_traj_step(C.byref(self.view), xyz, idx, xyz.shape[0], self.P, self.steps, self.px, self._owner, self.H, self.W,
                                              self.min_depth, _lib.stream_ptr(self.device)), "gp_traj_step")
        self.steps += 1

    def image(self, base=None, layout="hwc"):
        if layout not in ("hwc", "chw"):
            raise ValueError(f"TrajectoryCanvas.image: layout = {layout!r} must be 'hwc' or 'chw'")
        if base is not None:
            if not torch.is_tensor(base) or tuple(base.shape) != (3, self.H, self.W) or base.device != self.device:
                raise RuntimeError(f"TrajectoryCanvas.image: base must be a [3, {self.H}, {self.W}] tensor on {self.device}")
            base = base.detach().to(torch.float32).contiguous()
        if self.P == 0 or self.steps < 2:
            out = torch.zeros(3, self.H, self.W, dtype=torch.float32, device=self.device) if base is None else base.clone()
        else:
            out = torch.empty(3, self.H, self.W, dtype=torch.float32, device=self.device)
            with _lib.on_device(self.device):
                _lib.check(lib().gp_traj_resolve(self._owner, self.colors, self.P, base, out, self.H, self.W, _lib.stream_ptr(self.device)),
                           "gp_traj_resolve")
        return out.permute(1, 2, 0).contiguous() if layout == "hwc" else out
