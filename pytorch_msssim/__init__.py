"""Import-name shim: `from pytorch_msssim import ms_ssim` [REF metrics.py:24] resolves to the MI355X image-metric kernels
(gaussianprediction_amd.metrics.image_metrics, gp_image_metrics).  The reference calls
`ms_ssim(render, gt, data_range=1, size_average=True)` on [1,3,H,W] images [REF metrics.py:75,143].

Only the published default form is implemented: five scales with the weights (0.0448, 0.2856, 0.3001, 0.2363, 0.1333), an 11-tap
Gaussian window of sigma 1.5, K = (0.01, 0.03), three channels, min(H, W) > 160.  Any other argument off its default raises
ValueError naming the key.  Parity with the real pytorch_msssim is unpinned: the package is absent, so this follows its published
definition (valid convolution, 2x2 average pooling padded by size % 2, ReLU on the terms before the powers) and has never been
compared against it.  The result is a float64 tensor on the images' device and carries no gradient."""

_DEFAULTS = {"win_size": 11, "win_sigma": 1.5, "win": None, "weights": None, "K": (0.01, 0.03)}


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, weights=None, K=(0.01, 0.03)):
    """MS-SSIM of X against Y ([B,3,H,W], values in [0, data_range]): a scalar tensor (size_average=True) or [B]."""
    given = {"win_size": win_size, "win_sigma": win_sigma, "win": win, "weights": weights, "K": K}
    for key, default in _DEFAULTS.items():
        value = given[key]
        same = value is None if default is None else (value is not None and (tuple(value) == default if key == "K" else value == default))
        if not same:
            raise ValueError(f"pytorch_msssim shim: {key!r} = {value!r} is not implemented (only the default {default!r})")
    if not float(data_range) > 0:
        raise ValueError(f"pytorch_msssim shim: 'data_range' = {data_range!r} must be positive")
    from gaussianprediction_amd.metrics import MS_SSIM, image_metrics
    if float(data_range) != 1.0:
        X, Y = X / data_range, Y / data_range
    col = image_metrics(X, Y, ms_ssim=True).table[:, MS_SSIM]
    return col.mean() if size_average else col
