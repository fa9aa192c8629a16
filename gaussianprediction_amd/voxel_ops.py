"""Voxel-grid downsampling of a point cloud on the device (include/gp_voxel.h, csrc/voxel_kernels.hip): the step that makes the
cloud a HyperNeRF scene starts from.

  [REF utils/prepare/downsample_points.py]   voxel_size = 0.02; while len(pcd.points) > 40000: pcd = pcd.voxel_down_sample(voxel_size);
                                             voxel_size += 0.01  -- Open3D, on the host, over the dense COLMAP cloud
  [REF scene/dataset_readers.py:294]         opens the points3D_downsample.ply that loop wrote

The semantics are those of Open3D's PointCloud::VoxelDownSample, restated from its published source: float64 throughout,
min_bound = min(points) - voxel_size / 2, index = floor((p - min_bound) / voxel_size) as int32, one output point per occupied voxel =
the sum of its points in ascending input order over double(count); colours and normals are averaged the same way and normals are
not re-normalised.  Open3D is not installed where this was written, so PARITY WITH ITS BINARY IS UNPINNED: the tests pin a numpy
restatement of the same formulae (tests/voxel_ref.py), bit for bit.  The output ascends in (ix, iy, iz), x most significant; Open3D's
own order is that of its hash map, so only the SET of points is Open3D's -- and because a later pass of the loop sums in the order
the previous pass wrote, its sums can differ from Open3D's in the last bit.

One pass: two launches for the bounds, then a read of 64 bytes (the refusals -- a coordinate that is not finite, "voxel_size is too
small" -- are raised on it before any coordinate is converted to an integer, and the sort key takes only the bits the largest index
needs); the index, the sort, the segment heads and the means are launched without another look at the device; then a read of M.
HIP only: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np
import torch

from . import _lib, io_formats

GP_VOXEL_ABI_VERSION = 1            # include/gp_voxel.h
RECORD_DOUBLES = 8                  # min x y z, max x y z, the non-finite flag, 0
MAX_N = 2 ** 31 - 1                 # n below this


def _prototypes():
    i32, i64, f64, P = C.c_int32, C.c_int64, C.c_double, _lib.Ptr
    return {   # name: (restype, argtypes), as include/gp_voxel.h declares them (tests/test_voxel_host.py compares the two)
        "gp_voxel_abi_version": (i32, []),
        "gp_voxel_scratch_bytes": (i64, [i64]),
        "gp_voxel_bounds": (i32, [i64, P, P, P, P]),
        "gp_voxel_downsample": (i32, [i64, P, P, P, f64, P, P, P, P, P, P, P, P]),
        "gp_voxel_downsample_host": (i32, [i64, P, P, P, f64, P, P, P, P, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi("gp_voxel.h", "gp_voxel_abi_version", GP_VOXEL_ABI_VERSION, PROTOTYPES)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)


def _voxel_size(voxel_size):
    voxel_size = float(voxel_size)
    if not voxel_size > 0.0:
        raise RuntimeError(f"voxel_down_sample: voxel_size = {voxel_size} <= 0")
    return voxel_size


def _device_rows(name, t, n=None, device=None):
    """`t` as a contiguous float64 [n, 3] tensor on the device: float32 widens exactly."""
    if not torch.is_tensor(t):
        raise RuntimeError(f"voxel_down_sample: {name} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"voxel_down_sample: {name} are on {t.device} -- HIP kernels only (no CPU fallback)")
    if t.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"voxel_down_sample: {name} must be float32 or float64 (got {t.dtype})")
    if t.dim() != 2 or t.shape[1] != 3 or (n is not None and t.shape[0] != n):
        raise RuntimeError(f"voxel_down_sample: {name} must be [{'N' if n is None else n}, 3] (got {tuple(t.shape)})")
    if device is not None and t.device != device:
        raise RuntimeError(f"voxel_down_sample: {name} are on {t.device}, the points on {device}")
    return t.detach().to(torch.float64).contiguous()


def voxel_down_sample(points, voxel_size, colors=None, normals=None, *, return_index=False):
    """points [N, 3], colors and normals [N, 3] or None: float32 or float64 tensors on the device.  Returns float64
    (points [M, 3], colors, normals), None where None came in, plus the int32 voxel indices [M, 3] with return_index=True, in ascending
    (ix, iy, iz).  The semantics are the module's; parity with Open3D's binary is unpinned.  Raises RuntimeError for voxel_size <= 0, a
    coordinate that is not finite, "voxel_size is too small" (voxel_size * INT32_MAX below the padded extent) and N >= 2^31.  Two
    reads of the device: the bounds record, then M."""
    pts = _device_rows("points", points)
    voxel_size = _voxel_size(voxel_size)
    n, device = pts.shape[0], pts.device
    col = None if colors is None else _device_rows("colors", colors, n, device)
    nrm = None if normals is None else _device_rows("normals", normals, n, device)
    if n >= MAX_N:
        raise RuntimeError(f"voxel_down_sample: N = {n} must be below 2^31")
    if n == 0:
        out = (pts, col, nrm)
        return out + (torch.empty(0, 3, dtype=torch.int32, device=device),) if return_index else out
    l = lib()
    with _lib.on_device(device):
        stream = _lib.stream_ptr(device)
        scratch = _lib.scratch(l.gp_voxel_scratch_bytes, n, device=device)
        record = torch.empty(RECORD_DOUBLES, dtype=torch.float64, device=device)
        _lib.check(l.gp_voxel_bounds(n, pts, scratch, record, stream), "gp_voxel_bounds")
        bounds = record.cpu().numpy()                                                  # (the first read of the pass)
        out_p = torch.empty(n, 3, dtype=torch.float64, device=device)
        out_c = None if col is None else torch.empty_like(out_p)
        out_n = None if nrm is None else torch.empty_like(out_p)
        out_i = torch.empty(n, 3, dtype=torch.int32, device=device)
        m = torch.empty(1, dtype=torch.int32, device=device)
        _lib.check(l.gp_voxel_downsample(n, pts, col, nrm, voxel_size, bounds.ctypes.data, out_p, out_c, out_n, out_i, m, scratch, stream),
                   "gp_voxel_downsample")                                              # (refuses on the record before it launches)
        M = int(m.item())                                                              # (the second and last)
    cut = lambda t: None if t is None else t[:M].clone()                               # noqa: E731  (the n-row buffers go back to the allocator)
    out = (cut(out_p), cut(out_c), cut(out_n))
    return out + (cut(out_i),) if return_index else out


def host_pass(points, voxel_size, colors=None, normals=None, *, return_index=False):
    """The same pass on numpy float64 arrays through gp_voxel_downsample_host -- the programs of csrc/voxel_core.h on the CPU.  For the
    tests that run without a device: the device API above never falls back to it."""
    arr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3)      # noqa: E731
    pts, col, nrm = arr(points), arr(colors), arr(normals)
    n = pts.shape[0]
    like = lambda a: None if a is None else np.empty((n, 3), np.float64)               # noqa: E731
    out_p, out_c, out_n, out_i, m = like(pts), like(col), like(nrm), np.empty((n, 3), np.int32), C.c_int64(0)
    p = lambda a: None if a is None else a.ctypes.data                                 # noqa: E731
    _lib.check(lib().gp_voxel_downsample_host(n, p(pts), p(col), p(nrm), float(voxel_size), p(out_p), p(out_c), p(out_n), p(out_i), C.byref(m)),
               "gp_voxel_downsample_host")
    cut = lambda a: None if a is None else a[:m.value].copy()                          # noqa: E731
    out = (cut(out_p), cut(out_c), cut(out_n))
    return out + (cut(out_i),) if return_index else out


def _loop(one_pass, cloud, max_points, voxel_size, step):
    if max_points < 1 or not step > 0.0:
        raise RuntimeError(f"downsample_until: max_points = {max_points} must be >= 1 and step = {step} > 0")
    voxel_size, passes = float(voxel_size), []
    while cloud[0].shape[0] > max_points:
        cloud = one_pass(cloud[0], voxel_size, cloud[1], cloud[2])
        passes.append((voxel_size, int(cloud[0].shape[0])))
        voxel_size += step
    return cloud, passes


def downsample_until(points, colors=None, normals=None, max_points=40000, voxel_size=0.02, step=0.01):
    """The reference's loop: while the cloud holds more than max_points, voxel_down_sample it and grow voxel_size by step.  voxel_size
    accumulates `+= step` in a Python float, as the script's does (the fifth is 0.060000000000000005, not 0.06).  Each pass takes the
    float64 output of the one before (colours are not quantised in between).  Returns ((points, colors, normals),
    [(voxel_size, count) per pass]); a cloud that is small enough comes back as it is, widened to float64."""
    cloud = (_device_rows("points", points),) + tuple(None if t is None else _device_rows(name, t, points.shape[0], points.device)
                                                      for name, t in (("colors", colors), ("normals", normals)))
    return _loop(voxel_down_sample, cloud, max_points, voxel_size, step)


def read_point_cloud_ply(path):
    """(points, colors, normals) float64 numpy arrays of a PLY's vertex element: x y z, nx ny nz where present, red green blue as
    uchar / 255 where present (else None)."""
    v = io_formats.read_ply_vertices(path)
    names = v.dtype.names or ()
    cols = lambda keys: np.stack([np.asarray(v[k], dtype=np.float64) for k in keys], axis=1)       # noqa: E731
    if not all(k in names for k in ("x", "y", "z")):
        raise ValueError(f"{path}: no x y z on the vertex element")
    colors = cols(("red", "green", "blue")) / 255.0 if all(k in names for k in ("red", "green", "blue")) else None
    normals = cols(("nx", "ny", "nz")) if all(k in names for k in ("nx", "ny", "nz")) else None
    return cols(("x", "y", "z")), colors, normals


def downsample_ply(input_path, output_path, *, device="cuda:0", **loop_args):
    """utils/prepare/downsample_points.py: read input_path, run downsample_until(**loop_args) on `device`, write output_path with
    io_formats.save_point_cloud_ply (the fields the reference's fetchPly reads).  Returns the passes."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"downsample_ply: device = {device} -- HIP kernels only (no CPU fallback)")
    to = lambda a: None if a is None else torch.from_numpy(a).to(device)               # noqa: E731
    cloud, passes = downsample_until(*(to(a) for a in read_point_cloud_ply(input_path)), **loop_args)
    io_formats.save_point_cloud_ply(output_path, *(None if t is None else t.cpu().numpy() for t in cloud))
    return passes


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 2:
        print("usage: python -m gaussianprediction_amd.voxel_ops INPUT.ply OUTPUT.ply", file=sys.stderr)
        return 2
    for voxel_size, count in downsample_ply(argv[0], argv[1]):
        print(f"voxel_size {voxel_size!r}: {count} points")
    return 0


if __name__ == "__main__":
    sys.exit(main())
