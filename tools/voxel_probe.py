"""Voxel-grid downsampling on the device (voxel_ops / include/gp_voxel.h) measured on the GPU against the numpy restatement of the
same formulae (tests/voxel_ref.py) on this host -- not against Open3D, which is not installed: the reference's loop (voxel 0.02, + 0.01
a pass, until at most 40 000 points) on a synthetic surface cloud of 1 M coloured points, and the single pass at voxel 0.02, with the
library's brackets around each group of launches.  Both results are first compared bit for bit.  Writes profiles/voxel_probe.txt.

    python tools/voxel_probe.py            (needs a GPU)
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

import voxel_ref as ref  # noqa: E402
from gaussianprediction_amd import _lib, voxel_ops as V  # noqa: E402

DEV = torch.device("cuda", 0)
N = 1_000_000
BRACKETS = ("voxel_bounds", "voxel_index", "voxel_sort", "voxel_heads_scan", "voxel_mean")


def cloud(n, seed=0):
    """A wavy sheet over [-2, 2]^2 with a little thickness, float32 coordinates as a PLY of floats holds them, byte colours."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-2.0, 2.0, (n, 2))
    z = 0.3 * np.sin(3.0 * xy[:, 0]) * np.cos(2.0 * xy[:, 1]) + rng.normal(0.0, 0.004, n)
    pts = np.concatenate([xy, z[:, None]], axis=1).astype(np.float32).astype(np.float64)
    return pts, rng.integers(0, 256, (n, 3)).astype(np.float64) / 255.0


def wall(fn, warm=3, reps=30):
    """Median wall ms of fn(), which ends in a read of the device (so the clock stops after the work)."""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def same(t, a):
    return t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()


def main():
    pts, col = cloud(N)
    t0 = time.perf_counter()
    want_cloud, want_passes = ref.until(pts, col)
    host_loop = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    want_one = ref.down_sample(pts, 0.02, col)
    host_one = (time.perf_counter() - t0) * 1e3

    dp, dc = torch.from_numpy(pts).to(DEV), torch.from_numpy(col).to(DEV)
    got_cloud, got_passes = V.downsample_until(dp, dc)
    assert got_passes == want_passes and same(got_cloud[0], want_cloud[0]) and same(got_cloud[1], want_cloud[1])
    got_one = V.voxel_down_sample(dp, 0.02, dc)
    assert same(got_one[0], want_one[0]) and same(got_one[1], want_one[1])

    dev_loop = wall(lambda: V.downsample_until(dp, dc))
    dev_one = wall(lambda: V.voxel_down_sample(dp, 0.02, dc))
    _lib.profile_enable(2)
    reps = 20
    for _ in range(reps):
        V.voxel_down_sample(dp, 0.02, dc)
    torch.cuda.synchronize()
    brackets = _lib.profile_collect()
    _lib.profile_enable(0)
    ms = {k: brackets[k][1] / reps for k in BRACKETS}
    top = max(ms, key=ms.get)

    lines = [f"voxel_ops on {torch.cuda.get_device_name(DEV)}: a synthetic surface cloud of {N} points with colours (float64 on the device), against the numpy",
             "restatement tests/voxel_ref.py on this host (one thread; Open3D is not installed, so this is not a comparison with Open3D).  Both results were first",
             "compared bit for bit.  Device: wall ms, median of 30 after 3 warm-ups, host clock around a call that ends in its read of M.  numpy: one run.",
             "",
             f"the loop (voxel 0.02, + 0.01 a pass, until <= 40000): {len(want_passes)} passes, counts {[c for _, c in want_passes]}",
             f"  device {dev_loop:9.2f} ms    numpy {host_loop:9.1f} ms    numpy / device {host_loop / dev_loop:7.1f}x",
             f"the single pass at voxel 0.02: {N} -> {len(want_one[0])} points",
             f"  device {dev_one:9.2f} ms    numpy {host_one:9.1f} ms    numpy / device {host_one / dev_one:7.1f}x",
             "  library brackets, hipEvent ms per call (mean of 20, a run of its own): " + "  ".join(f"{k} {ms[k]:.4f}" for k in BRACKETS),
             f"  sum of the brackets {sum(ms.values()):.4f} ms of the {dev_one:.2f} ms wall; the largest is {top}",
             ("  the device loop is faster than the host restatement at this size" if dev_loop < host_loop else
              f"  the device loop is NOT faster than the host restatement at this size; the largest bracket is {top}")]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "voxel_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
