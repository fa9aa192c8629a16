#!/usr/bin/env python
"""Time the optical-flow entries (flow_ops) at the workload's size -- bench.py's synthetic scene, 1352 x 1014, 1 M Gaussians, stage 3:

    screen_flow, resolve, colorize (given and derived scale), flow_metrics, warp     hipEvent time of each call alone (median of REPS
                                                                                    after one warm-up), with the bytes it has to move
    render_flow                                                                     the whole call, and the ordinary render() of the
                                                                                    same view beside it

Informative only: no pass/fail threshold comes from here.  Prints one table and writes it to profiles/flow_probe.txt.

    python tools/flow_probe.py [--gaussians 1000000]
"""
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from gaussianprediction_amd import flow_ops as FO  # noqa: E402
from gaussianprediction_amd.renderer import render  # noqa: E402

DEV = torch.device("cuda", 0)
ITERATION, REPS = 50000, 7


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


def timed(fn):
    fn()
    return median([event_ms(fn) for _ in range(REPS)])


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    n = arg("--gaussians", 1_000_000)
    args = SimpleNamespace(gaussians=n, width=1352, height=1014, keypoints=250, nearest_num=6, time_freq=8, iteration=ITERATION,
                           scale_lo=0.003, scale_hi=0.012)
    pc, cams, _, _ = bench.build_workload(args, DEV)
    cam, nxt = cams[-2], cams[-1]
    H, W = args.height, args.width
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    bg = torch.zeros(3, device=DEV)
    t0, t1 = torch.from_numpy(cam.time).to(DEV), torch.from_numpy(nxt.time).to(DEV)
    with torch.no_grad():
        pc.forward(t0, ITERATION)
        xyz0 = pc._last_xyz_t.clone()
        pc.forward(t1, ITERATION)
        xyz1 = pc._last_xyz_t.clone()
    N = xyz0.shape[0]
    res = FO.render_flow(cam, pc, pipe, ITERATION, t0, t1, view1=nxt)
    rows = FO.screen_flow(xyz0, xyz1, cam, nxt)
    with torch.no_grad():
        comp = render(cam, pc, pipe, bg, time=t0, it=ITERATION, override_color=rows)["render"]
        frame = render(nxt, pc, pipe, bg, time=t1, it=ITERATION)["render"]
    assert torch.equal(FO.resolve(comp).flow, res.flow)
    gt = res.flow + 0.5 * torch.randn(res.flow.shape, generator=torch.Generator().manual_seed(0)).to(DEV)
    plane = H * W

    def with_no_grad(fn):
        def run():
            with torch.no_grad():
                fn()
        return run

    entries = [
        ("screen_flow (gp_flow_project)", lambda: FO.screen_flow(xyz0, xyz1, cam, nxt), 36 * N),
        ("resolve", lambda: FO.resolve(comp), 25 * plane),
        ("colorize, max_flow = 20", lambda: FO.colorize(res.flow, res.valid, 20.0), 21 * plane),
        ("colorize, derived max_flow", lambda: FO.colorize(res.flow, res.valid), 30 * plane),
        ("flow_metrics, B = 1, masked", lambda: FO.flow_metrics(res.flow, gt, res.valid), 17 * plane),
        ("warp, C = 3", lambda: FO.warp(frame, res.flow), 32 * plane),
        ("render_flow (3 deformations, project, render, resolve)", lambda: FO.render_flow(cam, pc, pipe, ITERATION, t0, t1, view1=nxt), 0),
        ("render() of the same view, for scale", with_no_grad(lambda: render(cam, pc, pipe, bg, time=t0, it=ITERATION)), 0),
        ("gaussians.forward alone", with_no_grad(lambda: pc.forward(t0, ITERATION)), 0),
    ]
    table = FO.flow_metrics(res.flow, gt, res.valid)[0].tolist()
    lines = [f"flow probe on {torch.cuda.get_device_name(DEV)}: bench.py's synthetic scene, {N} Gaussians, {W}x{H}, iteration {ITERATION}, the last two "
             f"cameras; hipEvent medians of {REPS} after one warm-up",
             f"valid pixels: {100 * float(res.valid.float().mean()):.1f} %; largest magnitude {float(FO.colorize(res.flow, res.valid, return_scale=True)[1]):.2f} px; "
             f"against flow + N(0, 0.5): EPE {table[1]:.4f}, > 1 px {100 * table[2]:.2f} %",
             f"{'entry':<58}{'ms':>10}{'MB moved':>12}{'GB/s':>10}"]
    for name, fn, nbytes in entries:
        ms = timed(fn)
        lines.append(f"{name:<58}{ms:>10.3f}" + (f"{nbytes / 1e6:>12.1f}{nbytes / (ms * 1e-3) / 1e9:>10.1f}" if nbytes else f"{'':>12}{'':>10}"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "flow_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
