#!/usr/bin/env python
"""Time eval_render.project_trajectory at the workload's size -- bench.py's synthetic scene, 1352 x 1014, 1 M Gaussians, stage 3,
60 steps -- and split it:

    the whole call               wall time, the device synchronised before and after (median of REPS after one warm-up)
    the 60 model forwards        hipEvent time of gaussians.forward alone
    the 60 draw launches         hipEvent time of TrajectoryCanvas.step alone, on the positions the forwards produced
    the resolve                  hipEvent time of TrajectoryCanvas.image

The draw launches' time is set against the number of pixel claims (32-bit atomic maxima: per segment max(|dx|, |dy|) + 1, counted
from the stored pixels without the clipping, so a slight over-count).  The numpy restatement of the tests (tests/trajectory_ref.py:
a Python loop per pixel, the host form the reference's cv2 loop would take) runs on the first HOST_POINTS points, where it finishes.
No pass/fail threshold comes from here.  Writes profiles/trajectory_probe.txt.

    python tools/trajectory_probe.py [--gaussians 1000000] [--steps 60]
"""
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import trajectory_ref as ref  # noqa: E402
from gaussianprediction_amd import eval_render as ER  # noqa: E402
from gaussianprediction_amd.renderer import render  # noqa: E402
from gaussianprediction_amd.trajectory_ops import NOT_DRAWABLE, TrajectoryCanvas  # noqa: E402

DEV = torch.device("cuda", 0)
ITERATION, REPS, HOST_POINTS = 50000, 5, 5000


def median(v):
    return sorted(v)[len(v) // 2]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    n, steps = arg("--gaussians", 1_000_000), arg("--steps", 60)
    args = SimpleNamespace(gaussians=n, width=1352, height=1014, keypoints=250, nearest_num=6, time_freq=8, iteration=ITERATION,
                           scale_lo=0.003, scale_hi=0.012)
    pc, cams, _, _ = bench.build_workload(args, DEV)
    cam = cams[-1]
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    with torch.no_grad():
        out = render(cam, pc, pipe, torch.zeros(3, device=DEV), time=torch.from_numpy(cam.time).to(DEV), it=ITERATION)
    tidx, H, W = out["tidx"], args.height, args.width
    flat = tidx.reshape(-1)
    idx = flat[flat != -1].contiguous()
    P = idx.numel()

    wall = []
    for k in range(REPS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        image = ER.project_trajectory(pc, cam, tidx, None, ITERATION, steps=steps, base=out["render"])
        torch.cuda.synchronize()
        if k:
            wall.append((time.perf_counter() - t0) * 1e3)
    times = torch.linspace(0, float(cam.time[0]), steps).to(DEV)
    positions = []

    def forwards(keep):
        with torch.no_grad():
            for i in range(steps):
                pc.forward(times[i:i + 1], ITERATION)
                if keep:
                    positions.append(pc._last_xyz_t.clone())

    forwards(True)
    fwd = median([event_ms(lambda: forwards(False)) for _ in range(REPS)])
    # the canvas is made outside the timed windows: its default colours are drawn on the host (torch.rand, then one upload)
    t0 = time.perf_counter()
    canvas = TrajectoryCanvas(cam, P, DEV, H=H, W=W)
    torch.cuda.synchronize()
    make_ms = (time.perf_counter() - t0) * 1e3
    claims, prev = 0, None
    for xyz in positions:
        canvas.step(xyz, idx)
        now = canvas.px.to(torch.int64)
        if prev is not None:
            ok = (prev[:, 0] != NOT_DRAWABLE) & (now[:, 0] != NOT_DRAWABLE)
            claims += int(((now - prev).abs().amax(dim=1) + 1)[ok].sum())
        prev = now
    assert torch.equal(canvas.image(out["render"]), image)

    def draws():
        c = TrajectoryCanvas(cam, P, DEV, H=H, W=W, colors=canvas.colors)
        return event_ms(lambda: [c.step(xyz, idx) for xyz in positions])

    draw = median([draws() for _ in range(REPS)])
    resolve = median([event_ms(lambda: canvas.image(out["render"])) for _ in range(REPS)])
    touched = int((canvas.owner != 0).sum())

    # the host restatement, on the first HOST_POINTS points
    hp = min(HOST_POINTS, P)
    hidx = idx[:hp].cpu().numpy()
    hsteps = [p.cpu().numpy() for p in positions]
    t0 = time.perf_counter()
    _, howner = ref.run(cam, H, W, hsteps, hidx, hp)
    host_s = time.perf_counter() - t0
    small = TrajectoryCanvas(cam, hp, DEV, H=H, W=W)
    small_ms = event_ms(lambda: [small.step(p, idx[:hp]) for p in positions])
    assert np.array_equal(small.owner.cpu().numpy(), howner)

    seg = P * (steps - 1)
    lines = [f"trajectory probe on {torch.cuda.get_device_name(DEV)}: bench.py's synthetic scene, {n} Gaussians, {W}x{H}, iteration {ITERATION}, "
             f"{steps} steps; medians of {REPS}",
             f"points (valid pixels of tidx): {P} = {100 * P / (H * W):.1f} % of the image, {int(torch.unique(idx).numel())} distinct Gaussians; "
             f"{seg} segments, {claims} pixel claims ({claims / max(seg, 1):.2f} per segment), {touched} pixels owned at the end",
             f"project_trajectory, whole call (wall, synchronised): {median(wall):10.3f} ms",
             f"  {steps} x gaussians.forward (hipEvent):              {fwd:10.3f} ms  = {fwd / steps:.3f} ms each",
             f"  {steps} x TrajectoryCanvas.step (hipEvent):          {draw:10.3f} ms  = {draw / steps:.3f} ms each, "
             f"{claims / (draw * 1e-3) / 1e9:.2f} G claims/s (32-bit atomic maxima, scattered), {seg / (draw * 1e-3) / 1e9:.3f} G segments/s",
             f"  resolve (hipEvent):                               {resolve:10.3f} ms",
             f"  TrajectoryCanvas(...) with default colours (wall):  {make_ms:8.3f} ms  (torch.rand of [P, 3] on the host and its upload; inside the whole call)",
             f"host restatement (tests/trajectory_ref.py, Python loop per pixel) on the first {hp} points: {host_s:.2f} s "
             f"= {1e6 * host_s / max(hp * (steps - 1), 1):.2f} us per segment; the device draws the same {hp} points in {small_ms:.3f} ms "
             f"(equal owner images); scaled to {P} points the host loop would take {host_s * P / max(hp, 1):.0f} s"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "trajectory_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
