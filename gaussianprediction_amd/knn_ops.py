"""General k-nearest neighbours and batched furthest-point sampling (csrc/knn_kernels.hip), the kernels behind the import-name
shims of the reference's CUDA extensions:

* `pytorch3d.ops.knn_points` [REF scene/gaussian_model.py:208, utils/loss_utils.py:36,43]  ->  `knn_points`
* `frnn.frnn_grid_points` [REF scene/gaussian_model.py:113,117]                          ->  `knn_points(..., r2_max=r*r, pad=-1)`
* `pointops_cuda.knnquery_cuda` / `furthestsampling_cuda` [REF utils/fps.py:84]          ->  `knn_points`, `furthest_point_sampling_batched`

HIP only: there is no CPU fallback.
"""
from __future__ import annotations

import math

import torch

from . import _lib


def _need_cuda(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: HIP kernels only (no CPU fallback)")


def _lengths(lengths, B, P, device):
    if lengths is None:
        return None
    lengths = torch.as_tensor(lengths, device=device)
    if lengths.shape != (B,):
        raise ValueError(f"knn_points: lengths must have shape ({B},), got {tuple(lengths.shape)}")
    return lengths.to(torch.int64).clamp(0, P).contiguous()


def _forward(p1, p2, l1, l2, K, norm, r2_max, splits, pad_idx, pad_dist):
    B, P1, D = p1.shape
    P2 = p2.shape[1]
    dists = torch.empty(B, P1, K, device=p1.device)
    idx = torch.empty(B, P1, K, dtype=torch.int64, device=p1.device)
    with _lib.TorchAllocator(p1.device) as alloc:
        rc = _lib.lib().gp_knn_points(B, P1, P2, D, p1, p2, l1, l2, K, norm, r2_max, splits, pad_idx, pad_dist, dists, idx,
                                      alloc.cb, None, _lib.stream_ptr(p1.device))
        _lib.check(rc, "gp_knn_points")
    return dists, idx


class _KnnPoints(torch.autograd.Function):
    """dists is differentiable with respect to p1 and p2 (gp_knn_points_backward); idx is not."""

    @staticmethod
    def forward(ctx, p1, p2, l1, l2, K, norm, r2_max, splits, pad_idx, pad_dist):
        x1, x2 = p1.detach().contiguous(), p2.detach().contiguous()
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        # the backward tells padded slots by idx < 0: with a different padding index the kernel pads with -1 and the padding is
        # substituted afterwards
        dists, idx = _forward(x1, x2, l1, l2, K, norm, r2_max, splits, -1 if need else pad_idx, pad_dist)
        if need:
            ctx.save_for_backward(x1, x2, l1, l2, idx)
            ctx.norm = norm
            if pad_idx != -1:
                idx = idx.masked_fill(idx < 0, pad_idx)
        ctx.mark_non_differentiable(idx)
        return dists, idx

    @staticmethod
    def backward(ctx, g_dists, _g_idx):
        x1, x2, l1, l2, idx = ctx.saved_tensors
        B, P1, D = x1.shape
        g = g_dists.to(torch.float32).contiguous()
        g1 = torch.zeros_like(x1) if ctx.needs_input_grad[0] else None
        g2 = torch.zeros_like(x2) if ctx.needs_input_grad[1] else None
        with _lib.on_device(x1.device):
            _lib.check(_lib.lib().gp_knn_points_backward(B, P1, x2.shape[1], D, x1, x2, l1, l2, idx, idx.shape[2], ctx.norm, g,
                                                         g1, g2, _lib.stream_ptr(x1.device)), "gp_knn_points_backward")
        return g1, g2, None, None, None, None, None, None, None, None


def knn_points(p1, p2, lengths1=None, lengths2=None, K=1, norm=2, r2_max=math.inf, splits=0, pad_idx=0, pad_dist=0.0):
    """(dists [B,P1,K], idx [B,P1,K] int64): the K nearest points of p2[b] to every point of p1[b], ascending distance, ties to the
    lower index.  norm 2: squared Euclidean distance; norm 1: sum of absolute differences.  Rows beyond lengths1, slots beyond
    lengths2 and neighbours with distance > r2_max receive (pad_dist, pad_idx).  splits: 0 = automatic (the result does not depend
    on it).  `dists` is differentiable with respect to p1 and p2."""
    if p1.dim() != 3 or p2.dim() != 3 or p1.shape[0] != p2.shape[0] or p1.shape[2] != p2.shape[2]:
        raise ValueError(f"knn_points: p1 [B,P1,D] and p2 [B,P2,D] expected, got {tuple(p1.shape)} and {tuple(p2.shape)}")
    _need_cuda(p1, "knn_points")
    _need_cuda(p2, "knn_points")
    if p1.dtype != torch.float32 or p2.dtype != torch.float32:
        raise TypeError("knn_points: fp32 points expected")
    B, P1, D = p1.shape
    l1 = _lengths(lengths1, B, P1, p1.device)
    l2 = _lengths(lengths2, B, p2.shape[1], p1.device)
    return _KnnPoints.apply(p1, p2, l1, l2, int(K), int(norm), float(r2_max), int(splits), int(pad_idx), float(pad_dist))


def furthest_point_sampling_batched(xyz, offset, new_offset, tmp=None, idx=None):
    """pointops' furthestsampling_cuda: offset / new_offset (int32, cumulative ends) cut xyz[n,3] into batches; batch i receives
    new_offset[i] - new_offset[i-1] samples, starting at its first point.  Returns idx (int32 [new_offset[-1]], global indices),
    written into `idx` when given."""
    _need_cuda(xyz, "furthest_point_sampling_batched")
    x = xyz.detach().to(torch.float32).contiguous()
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError("furthest_point_sampling_batched: xyz [n,3] expected")
    off = offset.to(device=x.device, dtype=torch.int32).contiguous()
    noff = new_offset.to(device=x.device, dtype=torch.int32).contiguous()
    b = off.shape[0]
    if noff.shape[0] != b:
        raise ValueError("furthest_point_sampling_batched: offset and new_offset differ in length")
    if idx is None:
        idx = torch.zeros(int(noff[-1].item()) if b else 0, dtype=torch.int32, device=x.device)
    if idx.dtype != torch.int32 or not idx.is_contiguous() or idx.device != x.device:
        raise ValueError("furthest_point_sampling_batched: idx must be a contiguous int32 tensor on the points' device")
    if tmp is None or tmp.dtype != torch.float32 or tmp.numel() < x.shape[0] or not tmp.is_contiguous():
        tmp = torch.empty(x.shape[0], device=x.device)
    with _lib.on_device(x.device):
        _lib.check(_lib.lib().gp_furthest_point_sampling_batched(b, off, noff, x.shape[0], idx.numel(), x, tmp, idx,
                                                                 _lib.stream_ptr(x.device)), "gp_furthest_point_sampling_batched")
    return idx
