#!/usr/bin/env python
"""Time the k-means of the keypoint extraction on the device path (kmeans_ops.kmeans, include/gp_kmeans.h) and on the torch
composition (training.kmeans: chunked cdist, argmin, index_add_) at N = 200 k (the reference's max_gaussian_size) and N = 1 M, with
K = 150 clusters of D = 35 model-like rows (xyz in +-1.3, features +-1e-3), 20 iterations, tol = 0.

Both paths run in one process, alternated, after warm-ups, each timed with device events; the figure is the median.  The torch path
stops early when its centres stop moving (it reads the device every iteration to know), so its time is divided by the iterations it
ran; the device path enqueues all 20 and the final assignment + mean, and its time is divided by 21 row passes.  Launches are
counted with the profiler.  The algorithmic figures per iteration -- 2 * 3 * N * K * D flop (a subtract, a multiply and an add per
term, for the assignment; counted twice as the issue states it) and 4 * N * D bytes -- are set against the measured peaks
(peaks.measure).  Writes profiles/kmeans_probe.txt.

    python tools/kmeans_probe.py [--sizes 200000,1000000]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from gaussianprediction_amd import kmeans_ops as KM, peaks, training  # noqa: E402

DEV = torch.device("cuda", 0)
K, D, ITERS = 150, 35, 20
REPS, WARM = 7, 2


def median(v):
    return sorted(v)[len(v) // 2]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


def torch_iterations(X):
    """The iterations training.kmeans runs before its allclose stops it (same arithmetic, counted)."""
    n = 0
    orig = torch.allclose

    def counting(*a, **kw):
        nonlocal n
        n += 1
        return orig(*a, **kw)

    torch.allclose = counting
    try:
        training.kmeans(X, K, iters=ITERS, seed=0)
    finally:
        torch.allclose = orig
    return n


def probe(n, lines, pk):
    g = torch.Generator().manual_seed(n)
    X = torch.rand(n, D, generator=g) * 2 - 1
    X[:, :3] *= 1.3
    X[:, 3:] *= 1e-3
    X = X.to(DEV).contiguous()
    aux = X[:, :3].contiguous()
    dev_fn = lambda: KM.kmeans(X, K, iters=ITERS, tol=0.0, seed=0, aux=aux)       # noqa: E731
    torch_fn = lambda: training.kmeans(X, K, iters=ITERS, seed=0)                 # noqa: E731
    t_dev, t_torch = [], []
    for k in range(WARM + REPS):
        a, res = event_ms(dev_fn)
        b, _ = event_ms(torch_fn)
        if k >= WARM:
            t_dev.append(a)
            t_torch.append(b)
    ran_torch = torch_iterations(X)
    n_dev, n_torch = launches(dev_fn), launches(torch_fn)
    per_dev, per_torch = median(t_dev) / (ITERS + 1), median(t_torch) / ran_torch
    flop, nbytes = 2 * 3 * n * K * D, 4 * n * D
    lines.append("")
    lines.append(f"N = {n}, K = {K}, D = {D}, {ITERS} iterations, tol = 0 (median of {REPS} after {WARM} warm-ups, hipEvent)")
    lines.append(f"  device path  kmeans_ops.kmeans : {median(t_dev):9.3f} ms = {per_dev:7.3f} ms per row pass ({ITERS} iterations + the final pass; "
                 f"ran {res.iterations}, converged {res.converged}), {n_dev} launches")
    lines.append(f"  torch path   training.kmeans   : {median(t_torch):9.3f} ms = {per_torch:7.3f} ms per iteration ({ran_torch} iterations ran), "
                 f"{n_torch} launches = {n_torch / ran_torch:.1f} per iteration")
    lines.append(f"  ratio torch / device per iteration: {per_torch / per_dev:.2f}x")
    lines.append(f"  per iteration: {flop / 1e9:.2f} Gflop, {nbytes / 1e6:.1f} MB of X;  device path: {flop / per_dev / 1e9:.1f} Tflop/s = "
                 f"{100 * flop / per_dev / 1e9 / pk['mfma_f32_TFLOPs']:.1f} % of the measured fp32 matrix rate, which is the vector rate on this part ({pk['mfma_f32_TFLOPs']:.1f} Tflop/s), "
                 f"{nbytes / per_dev / 1e6:.0f} GB/s = {100 * nbytes / per_dev / 1e6 / pk['copy_GBps']:.1f} % of the measured copy peak "
                 f"({pk['copy_GBps']:.0f} GB/s): the bound is the arithmetic")
    b2 = KM.kmeans(X, K, iters=ITERS, tol=0.0, seed=0, aux=aux)
    same = all(torch.equal(x, y) for x, y in ((res.ids, b2.ids), (res.centres, b2.centres), (res.counts, b2.counts), (res.aux_mean, b2.aux_mean)))
    lines.append(f"  two device runs bit-identical: {same};  scratch {int(KM.lib().gp_kmeans_scratch_bytes(n, D, K)) / 1e6:.1f} MB")
    del X, aux
    torch.cuda.empty_cache()


def main():
    sizes = (200_000, 1_000_000)
    if "--sizes" in sys.argv:
        sizes = tuple(int(s) for s in sys.argv[sys.argv.index("--sizes") + 1].split(","))
    pk = peaks.measure(str(DEV), gib=0.25, reps=5)
    lines = [f"k-means probe on {torch.cuda.get_device_name(DEV)}: model-like rows, centres from the seeded row subset both paths share",
             f"measured peaks (peaks.measure): fp32 (MFMA) {pk['mfma_f32_TFLOPs']:.1f} Tflop/s, copy {pk['copy_GBps']:.0f} GB/s"]
    for n in sizes:
        probe(n, lines, pk)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "kmeans_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
