"""PCA colouring of per-Gaussian features and a jet colour map, on the device (csrc/gp_pca.h, csrc/pca_kernels.hip): which Gaussians
move TOGETHER, shown by the three leading principal components of their motion features.

  [REF utils/visualizer_utils.py:57-82]    PCA_vis: sklearn PCA, np.percentile over all of the transformed values, trimesh export
  [REF utils/visualizer_utils.py:46-54]    draw_motion_feature: one component through matplotlib's jet, np.savetxt
  [REF utils/visualizer_utils.py:95-102]   draw_weights: one keypoint's weights through jet, np.savetxt
  [REF utils/visualizer_utils.py:35-44]    cluster: sklearn KMeans or MeanShift labels -- here kmeans_ops.kmeans (deterministic; sklearn's
                                           randomly initialised KMeans labelling is unpinned by nature) or meanshift_ops.mean_shift
                                           (csrc/gp_meanshift.h, pinned against sklearn), and label_colors for the segment renders

The header states the definition in full: float64 mean and covariance summed in a fixed order, cyclic Jacobi in float64, eigenvalues
descending, each component signed so that its entry of largest magnitude is positive (sklearn 1.7's svd_flip on the components), a
float32 projection, exact percentiles by a radix select, and the reference's (y - q1) / (q99 - q1).  Two fits of one input give equal
bytes.  What is unpinned: trimesh is not installed where this was written, so PCA_vis writes its cloud through
io_formats.save_point_cloud_ply and THE FILE'S LAYOUT AGAINST trimesh's EXPORT IS UNPINNED; and the results on non-finite input (the
calls return, nothing outside the arrays is touched).  q99 == q1 gives the IEEE result (inf or NaN colours), as in the reference.

HIP only: CPU tensors, another dtype than float32 and non-contiguous tensors raise."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

GP_PCA_ABI_VERSION = 1              # csrc/gp_pca.h
MAX_D, MAX_DIM, MAX_Q, CHUNK_ROWS = 128, 8, 2, 1024
HEADER = "../gaussianprediction_amd/csrc/gp_pca.h"      # relative to include/: the header is not one of include/ 


def _prototypes():
    i32, i64, P = C.c_int32, C.c_int64, _lib.Ptr
    return {   # name: (restype, argtypes), as csrc/gp_pca.h declares them (tests/test_pca_host.py compares the two)
        "gp_pca_abi_version": (i32, []),
        "gp_pca_scratch_size": (i64, [i64, i64]),
        "gp_pca_fit": (i32, [P, i64, i64, i32, P, P, P, P, i64, P]),
        "gp_pca_project": (i32, [P, i64, i64, P, P, i32, P, P]),
        "gp_pca_percentiles": (i32, [P, i64, P, i32, P, P, P, i64, P]),
        "gp_pca_colorize": (i32, [P, i64, i32, P, P, P, P]),
        "gp_colormap_lut": (i32, [P, i64, P, P, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi(HEADER, "gp_pca_abi_version", GP_PCA_ABI_VERSION, PROTOTYPES, register=False)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)


# ---- the refusals that need no device, as the library words them (None: accepted) ----
def check_fit(N, D, dim):
    N, D, dim = int(N), int(D), int(dim)
    if N < 2:
        return "N must be >= 2"
    if D < 1 or D > MAX_D:
        return "D must be in 1 .. 128"
    if dim < 1 or dim > MAX_DIM or dim > D or dim > N:
        return "dim must be in 1 .. min(8, D, N)"
    if N * dim >= 2 ** 31:
        return "N*dim must be below 2^31"
    return None


def check_percentiles(M, qs):
    M = int(M)
    if M < 1 or M >= 2 ** 31:
        return "M must be in 1 .. 2^31 - 1"
    if len(qs) < 1 or len(qs) > MAX_Q:
        return "the number of percentiles must be 1 or 2"
    if any(not (0.0 <= float(q) <= 100.0) for q in qs):
        return "a percentile must be in 0 .. 100"
    return None


def check_colorize(N, dim):
    N, dim = int(N), int(dim)
    if N < 1:
        return "N must be >= 1"
    if dim not in (3, 5):
        return "colours need dim 3 or 5"
    if N * dim >= 2 ** 31:
        return "N*dim must be below 2^31"
    return None


def _device_f32(what, t, ndim):
    if not torch.is_tensor(t):
        raise RuntimeError(f"{what} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{what} is on {t.device} -- HIP kernels only (no CPU fallback)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what} must be float32 (got {t.dtype})")
    if t.dim() != ndim:
        raise RuntimeError(f"{what} must have {ndim} dimension(s) (got {tuple(t.shape)})")
    if not t.is_contiguous():
        raise RuntimeError(f"{what} must be contiguous")
    return t.detach()


def _refuse(what, why, **sizes):
    if why:
        raise _lib.GpHipError(f"{what}: {why} ({', '.join(f'{k} = {v}' for k, v in sizes.items())})")


def _project(what, x, mean, components):
    N, D = x.shape
    dim = components.shape[0]
    _refuse(what, "N must be >= 1" if N < 1 else check_fit(max(N, 8), D, dim), N=N, D=D, dim=dim)
    if components.shape[1] != D or tuple(mean.shape) != (D,):
        raise RuntimeError(f"{what}: features are [{N}, {D}], the basis is for D = {components.shape[1]}")
    y = torch.empty(N, dim, dtype=torch.float32, device=x.device)
    with _lib.on_device(x.device):
        _lib.check(lib().gp_pca_project(x, N, D, mean, components, dim, y, _lib.stream_ptr(x.device)), "gp_pca_project")
    return y


def _percentiles(what, values, qs, selected=False):
    values = _device_f32(f"{what}: values", values, values.dim() if torch.is_tensor(values) else 1)
    qs = [float(q) for q in qs]
    M = values.numel()
    _refuse(what, check_percentiles(M, qs), M=M, nq=len(qs))
    dev = values.device
    out = torch.empty(len(qs), dtype=torch.float32, device=dev)
    sel = torch.empty(len(qs), 2, dtype=torch.float32, device=dev) if selected else None
    with _lib.on_device(dev):
        l = lib()
        scratch = _lib.scratch(l.gp_pca_scratch_size, 2, 1, device=dev)
        _lib.check(l.gp_pca_percentiles(values, M, (C.c_double * len(qs))(*qs), len(qs), out, sel, scratch, scratch.numel(),
                                        _lib.stream_ptr(dev)), "gp_pca_percentiles")
    return (out, sel) if selected else out


def percentiles(values, qs, selected=False):
    """np.percentile(values, qs) with linear interpolation, over ALL values of a float32 device tensor, exact (a radix select, no
    sort, no scratch of the values' size): a [len(qs)] float32 device tensor, len(qs) 1 or 2.  selected=True also returns
    [len(qs), 2]: the two order statistics each percentile was interpolated from.  Nothing is read from the device."""
    return _percentiles("percentiles", values, qs, selected)


def _colorize(what, y, q):
    N, dim = y.shape
    _refuse(what, check_colorize(N, dim), N=N, dim=dim)
    colors = torch.empty(N, 3, dtype=torch.float32, device=y.device)
    positions = torch.empty(N, 3, dtype=torch.float32, device=y.device) if dim == 5 else None
    with _lib.on_device(y.device):
        _lib.check(lib().gp_pca_colorize(y, N, dim, q, positions, colors, _lib.stream_ptr(y.device)), "gp_pca_colorize")
    return positions, colors


@dataclass
class PcaModel:
    """A fitted basis, every field a device tensor: mean [D], components [dim, D], explained_variance [dim], q1 and q99 (0-d views of
    `q` [2]: the 1st and 99th percentile of all of the fit's transformed values).
      .transform(features)   [N, dim]: (features - mean) @ components.T in float32, the definition's summation order
      .colors(features)      dim 3: [N, 3] in [0, 1];  .positions_colors(features), dim 5: ([N, 3] = (vis_0, vis_1, 1), [N, 3])
    for any rows of width D -- the frozen basis, e.g. keypoint features coloured in the Gaussians' basis."""
    mean: torch.Tensor
    components: torch.Tensor
    explained_variance: torch.Tensor
    q: torch.Tensor

    @property
    def q1(self):
        return self.q[0]

    @property
    def q99(self):
        return self.q[1]

    @property
    def dim(self):
        return int(self.components.shape[0])

    def transform(self, features):
        return _project("PcaModel.transform", _device_f32("PcaModel.transform: features", features, 2), self.mean, self.components)

    def positions_colors(self, features):
        return _colorize("PcaModel.colors", self.transform(features), self.q)

    def colors(self, features):
        return self.positions_colors(features)[1]


def pca_fit(features, dim=3, transformed=False) -> PcaModel:
    """Fit `dim` principal components of features [N, D] (float32, on the device, contiguous) and the percentiles q1, q99 of the
    transformed values.  transformed=True returns (model, Y [N, dim]) -- the projection the percentiles were taken over."""
    x = _device_f32("pca_fit: features", features, 2)
    N, D = x.shape
    dim = int(dim)
    _refuse("pca_fit", check_fit(N, D, dim), N=N, D=D, dim=dim)
    dev = x.device
    mean = torch.empty(D, dtype=torch.float32, device=dev)
    components = torch.empty(dim, D, dtype=torch.float32, device=dev)
    variance = torch.empty(dim, dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        l = lib()
        scratch = _lib.scratch(l.gp_pca_scratch_size, N, D, device=dev)
        _lib.check(l.gp_pca_fit(x, N, D, dim, mean, components, variance, scratch, scratch.numel(), _lib.stream_ptr(dev)), "gp_pca_fit")
    y = _project("pca_fit", x, mean, components)
    model = PcaModel(mean, components, variance, _percentiles("pca_fit", y, (1.0, 99.0)))
    return (model, y) if transformed else model


# ---- the jet colour map ----------------------------------------------------------------------------------------------------------
# matplotlib's segment data for `jet`: per channel the knots (x, y below, y above), y linear between knots
JET_SEGMENTS = {
    "red": ((0.00, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.00, 0.5, 0.5)),
    "green": ((0.000, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.640, 1, 1), (0.910, 0, 0), (1.000, 0, 0)),
    "blue": ((0.00, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.00, 0, 0)),
}


def _segment_table(knots, n):
    """The n samples of one channel, as matplotlib samples a segmented map: at x = k / (n - 1), linear between the enclosing knots."""
    a = np.asarray(knots, dtype=np.float64)
    x, y0, y1 = a[:, 0] * (n - 1), a[:, 1], a[:, 2]
    at = (n - 1) * np.linspace(0, 1, n)
    ind = np.searchsorted(x, at)[1:-1]
    t = (at[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
    return np.clip(np.concatenate([[y1[0]], t * (y0[ind] - y1[ind - 1]) + y1[ind - 1], [y0[-1]]]), 0.0, 1.0)


_JET = {}


def jet_table():
    """[256, 3] float32 on the host."""
    return np.stack([_segment_table(JET_SEGMENTS[c], 256) for c in ("red", "green", "blue")], axis=1).astype(np.float32)


def jet_lut(device="cuda"):
    """The [256, 3] float32 table of `jet` on `device` (built on the host once per device)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"jet_lut: device = {device} -- HIP kernels only (no CPU fallback)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _JET:
        _JET[device] = torch.from_numpy(jet_table()).to(device)
    return _JET[device]


def colormap(values, lut=None):
    """values [...] float32 on the device -> [..., 3]: row int(x * 256) of `lut` [256, 3] (default jet_lut) for 0 <= x < 1, row 255 for
    x >= 1, row 0 for x < 0, (0, 0, 0) for a NaN."""
    v = _device_f32("colormap: values", values, values.dim() if torch.is_tensor(values) else 1)
    lut = jet_lut(v.device) if lut is None else _device_f32("colormap: lut", lut, 2)
    if tuple(lut.shape) != (256, 3) or lut.device != v.device:
        raise RuntimeError(f"colormap: lut must be [256, 3] on {v.device}")
    out = torch.empty(*v.shape, 3, dtype=torch.float32, device=v.device)
    with _lib.on_device(v.device):
        _lib.check(lib().gp_colormap_lut(v, v.numel(), lut, out, _lib.stream_ptr(v.device)), "gp_colormap_lut")
    return out


# ---- the reference's functions ----------------------------------------------------------------------------------------------------
def PCA_vis(xyzs, features, output_path="default.ply", dim=3, return_only=False, finish_return=False):
    """[REF utils/visualizer_utils.py:57-82] on the device.  dim 3: the colours are the three leading components of `features`, the
    positions `xyzs`.  dim 5: the fit is over [xyzs, features]; the positions become (vis_0, vis_1, 1) and the colours components 2 .. 4.
    return_only: (positions, colours) as DEVICE tensors (the reference returns numpy arrays), nothing written.  Otherwise the cloud goes
    to `output_path` through io_formats.save_point_cloud_ply -- double x y z, uchar red green blue; trimesh is not installed where this
    was written, so the layout against trimesh's export is unpinned -- and with finish_return the pair is returned as well."""
    dim = int(dim)
    if dim not in (3, 5):
        raise RuntimeError(f"PCA_vis: dim = {dim} must be 3 or 5")
    xyzs = _device_f32("PCA_vis: xyzs", xyzs, 2)
    features = _device_f32("PCA_vis: features", features, 2)
    if xyzs.shape[1] != 3 or xyzs.shape[0] != features.shape[0] or xyzs.device != features.device:
        raise RuntimeError(f"PCA_vis: xyzs {tuple(xyzs.shape)} must be [N, 3] beside features {tuple(features.shape)}, on one device")
    samples = features if dim == 3 else torch.cat([xyzs, features], dim=-1)
    model, y = pca_fit(samples, dim, transformed=True)
    positions, colors = _colorize("PCA_vis", y, model.q)
    if dim == 3:
        positions = xyzs
    if return_only:
        return positions, colors
    from .io_formats import save_point_cloud_ply
    save_point_cloud_ply(output_path, positions.cpu().numpy(), colors.cpu().numpy())
    if finish_return:
        return positions, colors


def draw_motion_feature(points, features, output_path="vis_feature.txt", down_dim=1):
    """[REF utils/visualizer_utils.py:46-54]: the first of `down_dim` components of `features` through jet, UN-NORMALISED as in the
    reference (values outside [0, 1) take the table's end rows), written beside the points as text rows x y z r g b a (a = 1).
    Returns the [N, 3] colours on the device."""
    points = _device_f32("draw_motion_feature: points", points, 2)
    _, y = pca_fit(features, down_dim, transformed=True)
    colors = colormap(y[:, 0].contiguous())
    rgba = np.concatenate([colors.cpu().numpy(), np.ones((colors.shape[0], 1), np.float32)], axis=-1)
    np.savetxt(output_path, np.concatenate([points.cpu().numpy(), rgba], axis=-1))
    return colors


def draw_weights(weights_xyz, pcd, super_gaussians, idx, directory="visualize"):
    """[REF utils/visualizer_utils.py:95-102]: keypoint `idx`'s weights [N] through jet beside the points, to
    <directory>/weights_xyz_<idx>.txt (rows x y z r g b), and the keypoint's position three times to <directory>/kpts<idx>.txt.
    Returns the [N, 3] colours on the device."""
    weights_xyz = _device_f32("draw_weights: weights_xyz", weights_xyz, 2)
    pcd = _device_f32("draw_weights: pcd", pcd, 2)
    colors = colormap(weights_xyz[:, idx].contiguous())
    os.makedirs(directory, exist_ok=True)
    np.savetxt(os.path.join(directory, f"weights_xyz_{idx}.txt"), np.concatenate([pcd.cpu().numpy(), colors.cpu().numpy()], axis=-1))
    kpt = super_gaussians.detach().cpu().numpy()[..., :3][idx].reshape([1, 3]).repeat(3, axis=0)
    np.savetxt(os.path.join(directory, f"kpts{idx}.txt"), kpt)
    return colors


# ---- clusters -------------------------------------------------------------------------------------------------------------------------
def cluster(features, method="KMeans", k=4):
    """[REF utils/visualizer_utils.py:35-44] on the device: labels [N] int64 of features [N, D] (float32, on the device, contiguous).
    "KMeans": kmeans_ops.kmeans(features, k).ids -- deterministic Lloyd iterations from seeded rows, NOT sklearn's randomly initialised
    KMeans, whose labelling is unpinned by nature.  Anything else, as the reference's `else:`: meanshift_ops.mean_shift(features).labels,
    sklearn's MeanShift() with its estimated bandwidth, every row a seed (N * N pairs per step: subsample the seeds of a large cloud
    through meanshift_ops.mean_shift(features, seeds=...))."""
    features = _device_f32("cluster: features", features, 2)
    if method == "KMeans":
        from . import kmeans_ops
        return kmeans_ops.kmeans(features, k).ids
    from . import meanshift_ops
    return meanshift_ops.mean_shift(features).labels


def label_palette(count, seed=0):
    """[count, 3] float32 on the host: the seeded colours of labels 0 .. count - 1 (the first rows do not depend on count)."""
    return np.random.RandomState(seed).uniform(0.1, 1.0, size=(max(int(count), 1), 3)).astype(np.float32)


LABEL_GREY = (0.5, 0.5, 0.5)        # the colour of label -1 (an orphan of mean_shift(cluster_all=False))


def label_colors(labels, seed=0):
    """labels [N] int64 on the device -> [N, 3] float32: row `label` of label_palette(seed), mid-grey for -1.  One read of the largest
    label sizes the palette; the gather is torch indexing (plumbing, not a hot path)."""
    if not torch.is_tensor(labels) or not labels.is_cuda:
        raise RuntimeError(f"label_colors: labels is on {getattr(labels, 'device', 'the host')} -- HIP kernels only (no CPU fallback)")
    if labels.dim() != 1 or labels.dtype != torch.int64:
        raise RuntimeError(f"label_colors: labels must be [N] int64 (got {tuple(labels.shape)}, {labels.dtype})")
    count = int(labels.max()) + 1 if labels.numel() else 1
    table = torch.from_numpy(np.concatenate([label_palette(count, seed), np.array([LABEL_GREY], np.float32)])).to(labels.device)
    return table[torch.where(labels < 0, torch.full_like(labels, table.shape[0] - 1), labels)].contiguous()
