#!/usr/bin/env python
"""Time gp_knn_points (gaussianprediction_amd.knn_ops.knn_points) on the reference's three kNN shapes against the eager torch
search on the same device (torch.cdist + argmin / topk), hipEvent-timed, median of 20 runs after 3 warm-ups.  Writes
profiles/knn_probe.txt.

    python tools/knn_probe.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from gaussianprediction_amd.knn_ops import knn_points  # noqa: E402

DEV = torch.device("cuda", 0)


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def torch_knn(q, c, K, chunk):
    """the eager search: squared distances by torch.cdist in row chunks (bounded memory), then argmin (K = 1) or topk"""
    out = []
    for r0 in range(0, q.shape[0], chunk):
        d = torch.cdist(q[r0:r0 + chunk], c).square_()
        out.append(d.argmin(1, keepdim=True) if K == 1 else d.topk(K, dim=1, largest=False).indices)
    return torch.cat(out)


def main():
    g = torch.Generator(device=DEV).manual_seed(0)
    shapes = [("keypoint growth  [REF scene/gaussian_model.py:208]", 300, 1_000_000, 1, 300),
              ("iso_loss         [REF utils/loss_utils.py:36]", 20_000, 20_000, 21, 4096),
              ("nearest keypoints [REF scene/gaussian_model.py:113]", 1_000_000, 512, 8, 65536)]
    lines = [f"gp_knn_points vs torch.cdist + argmin/topk on {torch.cuda.get_device_name(DEV)}; D = 3, fp32, median of 20 (ms)",
             f"{'shape':56s} {'P1':>9s} {'P2':>9s} {'K':>3s} {'splits':>6s} {'hip ms':>8s} {'torch ms':>9s} {'speed-up':>8s}"]
    for name, P1, P2, K, chunk in shapes:
        c = torch.rand(1, P2, 3, device=DEV, generator=g) * 2 - 1
        q = torch.rand(1, P1, 3, device=DEV, generator=g) * 2 - 1 if P1 != P2 else c
        t_hip = timed(lambda: knn_points(q, c, K=K))
        t_t = timed(lambda: torch_knn(q[0], c[0], K, chunk), reps=5, warm=1)
        lines.append(f"{name:56s} {P1:9d} {P2:9d} {K:3d} {'auto':>6s} {t_hip:8.3f} {t_t:9.3f} {t_t / t_hip:7.1f}x")
        for s in (1, 7):
            lines.append(f"{'':56s} {P1:9d} {P2:9d} {K:3d} {s:6d} {timed(lambda: knn_points(q, c, K=K, splits=s)):8.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = os.path.join(ROOT, "profiles", "knn_probe.txt")
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
