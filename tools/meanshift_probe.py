"""The mean-shift clustering on the device (meanshift_ops / csrc/gp_meanshift.h) timed on the GPU, per phase -- the bandwidth estimate,
the steps, the merge -- with the library's brackets around each entry point, beside sklearn's estimate_bandwidth and MeanShift on this
host where sklearn can still run (N = 2000 and 5000 at D = 32), and alone at N = 20000 and 200000 (all points as seeds, and 4096
seeds).  The inputs are the blobs of tests/meanshift_ref.py (k = 5) at bandwidth 1.5 * sqrt(D); where sklearn ran, K, the labels and
n_iter are first compared.  Informative only: no test depends on these numbers.  Writes profiles/meanshift_probe.txt.

    python tools/meanshift_probe.py [largest N]            (needs a GPU)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import meanshift_ref as ref  # noqa: E402
from gaussianprediction_amd import _lib, meanshift_ops as M  # noqa: E402

DEV = torch.device("cuda", 0)
D, K_BLOBS, SEEDS = 32, 5, 4096
HOST_NS, DEVICE_NS = (2000, 5000), (20000, 200000)
BRACKETS = ("meanshift_bandwidth", "meanshift_run", "meanshift_merge", "kmeans_assign")


def wall(fn):
    """(wall ms of one fn() between two synchronisations, its result)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def device_row(x, seeds, bandwidth, estimate):
    """One line: the estimate (optional), then mean_shift at the given bandwidth with the brackets of its phases."""
    N, S = len(x), len(x) if seeds is None else len(seeds)
    est = f"{wall(lambda: M.estimate_bandwidth(x))[0]:9.2f} ms" if estimate else "  (as above)"
    _lib.profile_enable(2)
    whole, r = wall(lambda: M.mean_shift(x, bandwidth, seeds))
    b = _lib.profile_collect()
    _lib.profile_enable(0)
    steps = r.n_iter + 1
    run = b["meanshift_run"][1]
    return r, (f"N = {N:6d}  S = {S:6d}   estimate_bandwidth {est}   mean_shift {whole:9.2f} ms  =  steps {run:9.2f} "
               f"({steps} with work, {run / steps:8.3f} ms each, {N * S / 1e6:9.1f} M pairs a step: {N * S * steps / run / 1e6:8.1f} G pairs/s)"
               f"  merge {b['meanshift_merge'][1]:7.2f}  labels {b['kmeans_assign'][1]:6.2f}   K = {len(r.cluster_centers)}  n_iter = {r.n_iter}")


def main():
    largest = int(sys.argv[1]) if len(sys.argv) > 1 else max(DEVICE_NS)
    bandwidth = 1.5 * np.sqrt(D)
    lines = [f"meanshift_ops on {torch.cuda.get_device_name(DEV)}: blobs(N, {D}, {K_BLOBS}, seed = 4) of tests/meanshift_ref.py, bandwidth 1.5 * sqrt(D) = {bandwidth:.4f}, max_iter 300;",
             "wall ms of ONE call between two synchronisations after a warm-up on 2000 rows; steps / merge / labels: the library's hipEvent brackets of that call",
             "(steps: all max_iter + 1 launches, those that return at once included).", ""]
    warm = torch.from_numpy(ref.blobs(2000, D, K_BLOBS, 4)).to(DEV)
    M.mean_shift(warm, bandwidth), M.estimate_bandwidth(warm)
    for N in HOST_NS + tuple(n for n in DEVICE_NS if n <= largest):
        X = ref.blobs(N, D, K_BLOBS, 4)
        x = torch.from_numpy(X).to(DEV)
        r, text = device_row(x, None, bandwidth, True)
        lines.append(text)
        if N in HOST_NS:
            try:
                from sklearn.cluster import MeanShift, estimate_bandwidth
                t0 = time.perf_counter()
                est = estimate_bandwidth(X)
                t1 = time.perf_counter()
                ms = MeanShift(bandwidth=bandwidth).fit(X)
                t2 = time.perf_counter()
                agree = len(ms.cluster_centers_) == len(r.cluster_centers) and np.array_equal(ms.labels_, r.labels.cpu().numpy()) and ms.n_iter_ == r.n_iter
                lines.append(f"    sklearn on this host: estimate_bandwidth {(t1 - t0) * 1e3:9.1f} ms   MeanShift {(t2 - t1) * 1e3:9.1f} ms   K, labels, n_iter equal: {agree}"
                             f"   estimate rel. difference {abs(float(M.estimate_bandwidth(x)) / est - 1):.1e}")
            except ImportError:
                lines.append("    sklearn is not installed on this host: no host figure")
        else:
            lines.append(device_row(x, x[::max(1, N // SEEDS)][:SEEDS].contiguous(), bandwidth, False)[1])
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "meanshift_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
