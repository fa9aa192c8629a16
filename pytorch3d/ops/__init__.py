"""Import-name shim: `from pytorch3d.ops import knn_points` [REF scene/gaussian_model.py:28, 208; utils/loss_utils.py:36, 43]
resolves to the HIP kNN (gp_knn_points through `gaussianprediction_amd.knn_ops.knn_points`).

pytorch3d's conventions: squared distances for norm 2, results sorted ascending, padded slots (beyond lengths2) hold idx 0 and
dist 0.  Ties go to the lower index.  Parity with the real pytorch3d is unpinned: the package is absent, so this follows its
documented contract and has never been compared against it."""
from collections import namedtuple

_KNN = namedtuple("KNN", "dists idx knn")


def knn_gather(x, idx, lengths=None):
    """x[B,P2,D] gathered at idx[B,P1,K] -> [B,P1,K,D]; slots k >= lengths[b] (the padded ones) are zero."""
    import torch
    B, P1, K = idx.shape
    D = x.shape[2]
    out = torch.gather(x[:, None].expand(B, P1, x.shape[1], D), 2, idx[..., None].clamp_min(0).expand(B, P1, K, D))
    if lengths is not None:
        pad = torch.arange(K, device=idx.device).view(1, 1, K) >= torch.as_tensor(lengths, device=idx.device).view(B, 1, 1)
        out = out.masked_fill(pad[..., None], 0.0)
    return out


def knn_points(p1, p2, lengths1=None, lengths2=None, norm=2, K=1, version=-1, return_nn=False, return_sorted=True):
    """(dists [B,P1,K], idx [B,P1,K], knn [B,P1,K,D] or None).  `version` is accepted and ignored (one kernel); the result is
    always sorted, which also satisfies return_sorted=False.  dists is differentiable with respect to p1 and p2."""
    from gaussianprediction_amd.knn_ops import knn_points as _knn
    dists, idx = _knn(p1, p2, lengths1=lengths1, lengths2=lengths2, K=K, norm=norm, pad_idx=0, pad_dist=0.0)
    nn = knn_gather(p2, idx, lengths2) if return_nn else None
    return _KNN(dists, idx, nn)
