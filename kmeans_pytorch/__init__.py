"""Import-name shim: `kmeans_pytorch.kmeans` [REF utils/visualizer_utils.py:9, 85] resolves to the deterministic device k-means
(gp_kmeans_run through `gaussianprediction_amd.kmeans_ops.kmeans`).

The published package is absent here (it is not installed and cannot be fetched), so its behaviour is stated from its documentation
and has never been compared against: parity is unpinned.  Deliberate differences from what it documents: a cluster that loses all
its rows keeps its centre (the package draws a random row for it), and the ids returned are the assignment to the centres RETURNED
(the package returns the assignment made before the last update).  The stopping rule is the package's: the summed centre shift,
squared, against `tol`; `iter_limit = 0` (its "no limit") is capped at 1000 iterations."""


def kmeans(X, num_clusters, distance='euclidean', cluster_centers=[], tol=1e-4, tqdm_flag=True, iter_limit=0, device=None, seed=None):
    """(cluster_ids [N] int64, cluster_centers [K, D]), both on X's device."""
    import torch
    from gaussianprediction_amd import kmeans_ops
    if distance != 'euclidean':
        raise NotImplementedError(f"kmeans_pytorch.kmeans: distance={distance!r} (only 'euclidean' is implemented)")
    X = X.float().contiguous()
    if device is not None:
        X = X.to(device)
    init = None
    if torch.is_tensor(cluster_centers) or len(cluster_centers) > 0:
        init = torch.as_tensor(cluster_centers, dtype=torch.float32, device=X.device).contiguous()
    limit = int(iter_limit) if iter_limit and int(iter_limit) > 0 else kmeans_ops.MAX_ITERS
    res = kmeans_ops.kmeans(X, int(num_clusters), iters=min(limit, kmeans_ops.MAX_ITERS), tol=float(tol), seed=0 if seed is None else int(seed),
                            init=init)
    return res.ids, res.centres
