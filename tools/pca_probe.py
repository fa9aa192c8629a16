"""The PCA colouring on the device (feature_vis / csrc/gp_pca.h) timed on the GPU: fit + colours of 1 M x 32 features, with the
library's brackets around each entry point, beside the reference's recipe on this host (sklearn's PCA, np.percentile, the projection
and the clip of [REF utils/visualizer_utils.py:57-75]) on the same array -- the host figure includes no copy off the device, which the
reference also pays.  The two colourings are first compared.  Informative only: no test depends on these numbers.  Writes
profiles/pca_probe.txt.

    python tools/pca_probe.py            (needs a GPU)
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pca_ref as ref  # noqa: E402
from gaussianprediction_amd import _lib, feature_vis as F  # noqa: E402

DEV = torch.device("cuda", 0)
N, D, DIM = 1_000_000, 32, 3
BRACKETS = ("pca_fit", "pca_project", "pca_percentiles", "pca_colorize")
WARM, REPS = 3, 20


def wall(fn):
    """Median wall ms of fn() between two synchronisations."""
    for _ in range(WARM):
        fn()
    out = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def host_recipe(X):
    from sklearn.decomposition import PCA
    pca = PCA(DIM, random_state=42)
    transformed = pca.fit_transform(X)
    q1, q99 = np.percentile(transformed, [1, 99])
    vis = (X - X.mean(0)[None, :]) @ pca.components_.T
    return ((vis - q1) / (q99 - q1)).clip(0.0, 1.0).astype(np.float32)


def main():
    X = ref.generate(N, D, 1)
    x = torch.from_numpy(X).to(DEV)

    def device():
        model = F.pca_fit(x, DIM)
        return model.colors(x)

    colors = device().cpu().numpy()
    whole = wall(device)
    fit_only = wall(lambda: F.pca_fit(x, DIM))
    _lib.profile_enable(2)
    for _ in range(REPS):
        device()
    torch.cuda.synchronize()
    brackets = _lib.profile_collect()
    _lib.profile_enable(0)
    ms = {k: brackets[k][1] / REPS for k in BRACKETS}

    lines = [f"feature_vis on {torch.cuda.get_device_name(DEV)}: pca_fit(dim = {DIM}) + colors of {N} x {D} float32 features (the generator of tests/pca_ref.py);",
             f"device: wall ms between two synchronisations, median of {REPS} after {WARM} warm-ups; brackets: hipEvent ms per call, mean of {REPS}, a run of its own.",
             "",
             f"pca_fit + colors:  {whole:8.3f} ms     pca_fit alone (mean, covariance, Jacobi, projection, percentiles):  {fit_only:8.3f} ms",
             "  brackets per pca_fit + colors: " + "  ".join(f"{k} {ms[k]:.4f}" for k in BRACKETS) + "   (pca_project runs twice: in the fit and in colors)",
             f"  input read at {N * D * 4 / 1e6:.0f} MB a pass: the fit reads it twice (mean, covariance), each projection once"]
    try:
        t0 = time.perf_counter()
        want = host_recipe(X)
        host = (time.perf_counter() - t0) * 1e3
        lines += [f"the reference's recipe on this host (sklearn PCA + np.percentile + projection, one run, no copy off the device counted):  {host:9.1f} ms",
                  f"  largest colour difference device - host: {np.abs(colors - want).max():.3e}   host / device: {host / whole:.1f}x (informative: another host gives another ratio)"]
    except ImportError:
        lines += ["sklearn is not installed on this host: no host figure"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "pca_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
