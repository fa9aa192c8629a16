"""Import-name shim: `frnn.frnn_grid_points` [REF scene/gaussian_model.py:29, 113, 117] resolves to the HIP kNN (gp_knn_points
through `gaussianprediction_amd.knn_ops.knn_points`, exact brute force with the radius as a cutoff).

frnn's conventions: squared distances, neighbours farther than r and slots beyond lengths2 hold idx -1 and dist -1; the grid it
returns is an opaque token here (no grid is built) and is accepted back.  Parity with the real frnn is unpinned: the package is
absent, so this follows its documented contract and has never been compared against it."""


class _Grid:
    """What frnn_grid_points returns as `grid`: nothing is precomputed, so passing it back changes nothing."""

    def __init__(self, shape):
        self.shape = shape


def frnn_grid_points(points1, points2, lengths1=None, lengths2=None, K=-1, r=-1, grid=None, return_nn=False, return_sorted=True,
                     radius_cell_ratio=2):
    """(dists [B,P1,K], idxs [B,P1,K], nn [B,P1,K,D] or None, grid)."""
    import torch
    from gaussianprediction_amd.knn_ops import knn_points as _knn
    if K is None or int(K) < 1:
        raise ValueError("frnn_grid_points: K >= 1 required")
    if isinstance(r, torch.Tensor):
        if r.numel() != 1 and not bool((r == r.reshape(-1)[0]).all()):
            raise ValueError("frnn_grid_points: one radius for all batches is supported")
        r = float(r.reshape(-1)[0])
    r = float(r)
    if r <= 0:
        raise ValueError("frnn_grid_points: r > 0 required")
    dists, idxs = _knn(points1, points2, lengths1=lengths1, lengths2=lengths2, K=int(K), norm=2, r2_max=r * r, pad_idx=-1, pad_dist=-1.0)
    nn = None
    if return_nn:
        from pytorch3d.ops import knn_gather
        nn = knn_gather(points2, idxs, lengths2).masked_fill((idxs < 0)[..., None], 0.0)
    return dists, idxs, nn, grid if grid is not None else _Grid(tuple(points2.shape))
