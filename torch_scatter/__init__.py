"""Import-name shim: `torch_scatter.scatter` [REF utils/visualizer_utils.py:10, 86] resolves to the per-cluster mean of the device
k-means (gp_cluster_mean through `gaussianprediction_amd.kmeans_ops.cluster_mean`: double sums in a fixed order, no atomics).

Only what the reference calls is here: a 2-D float `src`, `dim=0`, a 1-D `index`, `reduce` "sum" or "mean"; everything else raises
NotImplementedError.  torch_scatter is a compiled CUDA extension that is absent here, so this follows its documented contract and
has never been compared against it: parity is unpinned."""


def scatter(src, index, dim=-1, out=None, dim_size=None, reduce='sum'):
    """[dim_size or index.max() + 1, C]: the sum or mean of the rows of `src` that share an index; rows nobody indexes are zero."""
    import torch
    from gaussianprediction_amd import kmeans_ops
    if out is not None:
        raise NotImplementedError("torch_scatter.scatter: out= is not implemented")
    if reduce not in ('sum', 'mean'):
        raise NotImplementedError(f"torch_scatter.scatter: reduce={reduce!r} (only 'sum' and 'mean' are implemented)")
    if not torch.is_tensor(src) or src.dim() != 2 or not src.is_floating_point():
        raise NotImplementedError(f"torch_scatter.scatter: src must be a 2-D float tensor (got {getattr(src, 'shape', type(src).__name__)})")
    if dim not in (0, -2):
        raise NotImplementedError(f"torch_scatter.scatter: dim={dim} (only dim=0 is implemented)")
    if index.dim() != 1 or index.shape[0] != src.shape[0]:
        raise NotImplementedError(f"torch_scatter.scatter: index must be [{src.shape[0]}] (got {tuple(index.shape)}; broadcasting is not implemented)")
    K = int(dim_size) if dim_size is not None else int(index.max()) + 1
    mean, counts = kmeans_ops.cluster_mean(src.float().contiguous(), index.contiguous(), K)
    res = mean if reduce == 'mean' else mean * counts[:, None].to(mean.dtype)
    return res.to(src.dtype)
