#!/usr/bin/env python
"""Time the loop-side densification calls on the existing (torch indexing) and the device (include/gp_densify.h) paths:

    densify.track_view          against  densify.track_view_device          (every iteration below densify_until_iter)
    densify.densification_step  against  densify.densification_step_device  (every densification_interval iterations)

at N = 200 k (the reference's max_gaussian_size) and 1 M, on bench.py's synthetic scene in stage 1 after three tracked TrainStep
steps.  Every figure is a median of 20 after 3 warm-ups: wall time with the device synchronised before and after, and hipEvent
time.  Both surgeries start from copies of ONE model state (restored before every repetition, outside the timed window), with a
gradient threshold at the 75th percentile of the tracked rows so that a quarter of them is cloned or split.  The apply kernel's own
time (the library's hipEvent bracket) is set against the bytes it must move and the measured copy peak (peaks.measure).
Writes profiles/densify_probe.txt.

    python tools/densify_probe.py [--sizes 200000,1000000]
"""
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from torch import nn  # noqa: E402

import bench  # noqa: E402
from gaussianprediction_amd import _lib, densify as dn, densify_ops as D, peaks  # noqa: E402
from gaussianprediction_amd.train_step import TrainStep  # noqa: E402
from gaussianprediction_amd.training import PER_GAUSSIAN, default_training_args  # noqa: E402

DEV = torch.device("cuda", 0)
ITERATION, SURGERY_ITERATION, EXTENT = 5000, 3100, 1.0
REPS, WARM = 20, 3


def median(v):
    return sorted(v)[len(v) // 2]


def timed(fn, before=None):
    """(median wall ms, median hipEvent ms) of fn(); `before` runs outside the timed window."""
    wall, dev = [], []
    for k in range(WARM + REPS):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if k >= WARM:
            wall.append((t1 - t0) * 1e3)
            dev.append(a.elapsed_time(b))
    return median(wall), median(dev)


def snapshot(pc):
    mom = pc.adam_moments()
    return SimpleNamespace(params={k: p.detach().clone() for k, p in pc._per_gaussian().items()},
                           moments={k: tuple(t.clone() for t in mom[id(p)]) for k, p in pc._per_gaussian().items() if id(p) in mom},
                           stats=tuple(t.clone() for t in (pc.xyz_gradient_accum, pc.denom, pc.xyz_gradient_accum_max, pc.max_radii2D)))


def restore(pc, snap):
    carried = {}
    for name, attr in PER_GAUSSIAN:
        if name in snap.params:
            q = nn.Parameter(snap.params[name].clone().requires_grad_(True))
            setattr(pc, attr, q)
            if name in snap.moments:
                carried[id(q)] = tuple(t.clone() for t in snap.moments[name])
    pc.xyz_gradient_accum, pc.denom, pc.xyz_gradient_accum_max, pc.max_radii2D = (t.clone() for t in snap.stats)
    pc._rebuild_optimizer(carried)


def apply_bytes(snap, n_out, kept):
    """Bytes the apply must move: survivors read parameter + both moments, new rows read the parameter; every output row is written
    in full; four statistics per output row."""
    floats = sum(t[0].numel() for t in snap.params.values())
    with_moments = sum(snap.params[k][0].numel() for k in snap.moments)
    read = kept * (floats + 2 * with_moments) + (n_out - kept) * floats
    written = n_out * (floats + 2 * with_moments + 4)
    return 4 * (read + written), floats, with_moments


def probe(n, lines, copy_peak):
    args = SimpleNamespace(gaussians=n, width=1352, height=1014, keypoints=250, nearest_num=6, time_freq=8, iteration=ITERATION,
                           scale_lo=0.003, scale_hi=0.012)
    pc, cams, gts, _ = bench.build_workload(args, DEV)
    ts = TrainStep(pc, cams, gts, ITERATION, schedule=True)
    for i in range(3):
        _, pkg = ts.step(i)
        dn.track_view(pc, pkg["viewspace_points"], pkg["visibility_filter"], pkg["radii"])
    torch.cuda.synchronize()
    snap = snapshot(pc)
    g = (pc.xyz_gradient_accum / pc.denom.clamp_min(1)).squeeze(-1)
    seen = g[g > 0]
    opt = default_training_args(densify_grad_threshold=float(seen.kthvalue(max(1, int(0.75 * seen.numel()))).values))
    visible = int(pkg["visibility_filter"].sum())

    rows = [("track_view", timed(lambda: dn.track_view(pc, pkg["viewspace_points"], pkg["visibility_filter"], pkg["radii"]))),
            ("track_view_device", timed(lambda: dn.track_view_device(pc, pkg)))]
    out = {}

    def surgery(fn, key):
        def run():
            out[key] = (fn(pc, SURGERY_ITERATION, opt, EXTENT, max_gaussian_size=10 ** 9), pc._xyz.shape[0])
        return run

    rows.append(("densification_step", timed(surgery(dn.densification_step, "old"), before=lambda: restore(pc, snap))))
    rows.append(("densification_step_device", timed(surgery(dn.densification_step_device, "new"), before=lambda: restore(pc, snap))))
    # the kernels' own times: the library's hipEvent brackets over ten device surgeries
    restore(pc, snap)
    _lib.profile_enable(2)
    _lib.profile_collect()
    for _ in range(10):
        restore(pc, snap)
        dn.track_view_device(pc, pkg)
        dn.densification_step_device(pc, SURGERY_ITERATION, opt, EXTENT, max_gaussian_size=10 ** 9)
    torch.cuda.synchronize()
    prof = _lib.profile_collect()
    _lib.profile_enable(0)
    per = {k: prof[k][1] / max(prof[k][0], 1) for k in ("densify_stats", "densify_plan", "densify_apply") if k in prof}
    (n_clone, n_src, n_pruned), n_out = out["new"]
    # survivors of segment 0, from a plan on the snapshot (the status block's first base after it)
    restore(pc, snap)
    P = pc._per_gaussian()
    _, status, _ = D.plan(pc.xyz_gradient_accum, pc.denom, pc.max_radii2D, P["scaling"].detach(), P["opacity"].detach(),
                          opt.densify_grad_threshold, pc.percent_dense * EXTENT, 0.005, 20, 0.1 * EXTENT, do_densify=True, do_reset=False)
    kept = int(status[D.ST_BASE + 1])
    nbytes, floats, with_moments = apply_bytes(snap, n_out, kept)
    lines.append("")
    lines.append(f"N = {n}: {visible} rows visible in the tracked view; surgery at iteration {SURGERY_ITERATION} (densify + prune), "
                 f"threshold {opt.densify_grad_threshold:.3e}")
    lines.append(f"  existing path: (cloned, split sources, pruned) = {out['old'][0]} -> {out['old'][1]} rows;  device path: {out['new'][0]} -> {n_out} rows")
    lines.append(f"  {'call':28s} {'wall ms':>10s} {'hipEvent ms':>12s}")
    for name, (w, d) in rows:
        lines.append(f"  {name:28s} {w:10.3f} {d:12.3f}")
    sp = lambda a, b: rows[a][1][0] / rows[b][1][0]      # noqa: E731
    lines.append(f"  wall-time ratio existing / device: track_view {sp(0, 1):.2f}x   densification_step {sp(2, 3):.2f}x")
    lines.append("  kernels (library brackets, ms per call): " + "  ".join(f"{k} {v:.4f}" for k, v in per.items()))
    if "densify_apply" in per:
        rate = nbytes / (per["densify_apply"] * 1e-3) / 1e9
        lines.append(f"  apply: {floats} floats per row, {with_moments} of them with two moments; {nbytes / 1e6:.1f} MB read + written in "
                     f"{per['densify_apply']:.4f} ms = {rate:.0f} GB/s = {100 * rate / copy_peak:.0f} % of the measured copy peak ({copy_peak:.0f} GB/s)")
    del ts, pc, snap
    torch.cuda.empty_cache()


def main():
    sizes = (200_000, 1_000_000)
    if "--sizes" in sys.argv:
        sizes = tuple(int(s) for s in sys.argv[sys.argv.index("--sizes") + 1].split(","))
    copy_peak = peaks.measure(str(DEV), gib=0.25, reps=5)["copy_GBps"]
    lines = [f"densify probe on {torch.cuda.get_device_name(DEV)}: bench.py's synthetic scene, stage 1, three tracked steps; median of {REPS} "
             f"after {WARM} warm-ups", f"measured copy peak (peaks.measure, read + written bytes): {copy_peak:.0f} GB/s"]
    for n in sizes:
        probe(n, lines, copy_peak)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "densify_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
