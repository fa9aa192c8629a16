"""Writes tests/golden/meanshift.npz: sklearn's MeanShift and estimate_bandwidth on the fixture cases of tests/test_meanshift_host.py,
run on the CPU with the installed sklearn (1.7.2 when the committed file was written).  Arrays only; the versions and the description
are strings.  Run from the repository root: python tests/golden/make_meanshift_vectors.py"""
import os
import sys

import numpy as np
import sklearn
from sklearn.cluster import MeanShift, estimate_bandwidth

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import meanshift_ref as ref  # noqa: E402


def fixture_runs():
    """(tag, X key, X, bandwidth or None for the estimate, max_iter) of every recorded run."""
    for N, D, k, seed in ref.BLOB_CASES:
        if D == 64:
            continue
        X = ref.blobs(N, D, k, seed)
        yield f"blobs_{N}_{D}_est", f"blobs_{N}_{D}", X, None, 300
        yield f"blobs_{N}_{D}_fix", f"blobs_{N}_{D}", X, 1.5 * np.sqrt(D), 300
    for n, (N, D, k, seed, bw) in enumerate(ref.LINE_CASES):
        if N == 1500:
            continue
        X = ref.lines(N, D, k, seed)
        for max_iter in (300, 3):
            yield f"lines{n}_{N}_{D}_{max_iter}", f"lines_{N}_{D}", X, bw, max_iter


def main():
    out, worst = {}, 0.0
    for tag, xkey, X, bw, max_iter in fixture_runs():
        out[f"X_{xkey}"] = X
        est = float(estimate_bandwidth(X))
        out[f"estimate_{xkey}"] = np.float64(est)
        ms = MeanShift(bandwidth=est if bw is None else bw, max_iter=max_iter).fit(X)
        assert ms.labels_.max() < 2 ** 15
        out[f"centers_{tag}"] = ms.cluster_centers_.astype(np.float32)
        assert (out[f"centers_{tag}"] == ms.cluster_centers_).all()
        out[f"labels_{tag}"] = ms.labels_.astype(np.int16)
        out[f"n_iter_{tag}"] = np.int32(ms.n_iter_)
        out[f"bandwidth_{tag}"] = np.float64(est if bw is None else bw)
        r = ref.mean_shift(X, out[f"bandwidth_{tag}"], max_iter=max_iter)
        assert r["cluster_centers"].shape == ms.cluster_centers_.shape and (r["labels"] == ms.labels_).all() and r["n_iter"] == ms.n_iter_, tag
        err = float(np.abs(r["cluster_centers"].astype(np.float64) - ms.cluster_centers_).max())
        worst = max(worst, err)
        print(f"{tag}: K = {len(ms.cluster_centers_)}, n_iter = {ms.n_iter_}, |restatement - sklearn| centres = {err:.3g}, "
              f"bandwidth rel = {abs(ref.estimate_bandwidth(X) / est - 1):.3g}", flush=True)
    out["sklearn_version"] = np.array(sklearn.__version__)
    out["numpy_version"] = np.array(np.__version__)
    out["restatement_to_sklearn_centres"] = np.float64(worst)
    out["description"] = np.array(
        "sklearn MeanShift (cluster_centers_, labels_ as int16, n_iter_) and estimate_bandwidth on the float32 inputs X_*; the numpy "
        f"restatement tests/meanshift_ref.py gave every label and n_iter equal and centres within {worst:.3g} absolute when this was written")
    np.savez_compressed(os.path.join(HERE, "meanshift.npz"), **out)
    print("largest |restatement - sklearn| over the centres:", worst)


if __name__ == "__main__":
    main()
