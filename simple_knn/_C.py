"""Import-name shim: `from simple_knn._C import distCUDA2` [REF scene/gaussian_model.py:21, 341] resolves to the MI355X
implementation (HIP kernel gp_knn3_mean_dist2 through `gaussianprediction_amd.weights_ops.dist_cuda2`).

Parity with the real simple_knn is unpinned: the package is absent from the reference tree, so this follows its published
contract (mean squared distance to the three nearest other points) and has never been compared against it."""


def distCUDA2(points):
    """[n] mean squared distance of every point of points[n,3] to its three nearest other points."""
    from gaussianprediction_amd.weights_ops import dist_cuda2
    return dist_cuda2(points)
