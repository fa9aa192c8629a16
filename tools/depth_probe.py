#!/usr/bin/env python
"""Time the depth entries (depth_ops) at the workload's size -- bench.py's synthetic scene, 1352 x 1014, 1 M Gaussians, stage 3:

    resolve, colorize (given and derived range), normals, normals_image, unproject, depth_metrics     hipEvent time of each call alone
                                                                (median of REPS after one warm-up), with the bytes it has to move
    render_depth                                                the whole call, and the ordinary render() of the same view beside it

unproject's time includes its one read of the count.  Informative only: no pass/fail threshold comes from here.  Prints one table and
writes it to profiles/depth_probe.txt.

    python tools/depth_probe.py [--gaussians 1000000]
"""
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from gaussianprediction_amd import depth_ops as DO  # noqa: E402
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
    cam = cams[-1]
    H, W = args.height, args.width
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    bg = torch.zeros(3, device=DEV)
    t = torch.from_numpy(cam.time).to(DEV)
    res = DO.render_depth(cam, pc, pipe, ITERATION, time=t)
    with torch.no_grad():
        out = render(cam, pc, pipe, bg, time=t, it=ITERATION, override_color=torch.ones(pc.get_xyz.shape[0], 3, device=DEV))
        frame = render(cam, pc, pipe, bg, time=t, it=ITERATION)["render"]
    accum, alpha = out["depth"].reshape(H, W), out["render"][0].contiguous()
    assert torch.equal(DO.resolve(accum, alpha).depth, res.depth)
    normals, nvalid = DO.normals(res.depth, res.valid, cam)
    gt = res.depth * (1.0 + 0.05 * torch.randn(res.depth.shape, generator=torch.Generator().manual_seed(0)).to(DEV))
    plane, K = H * W, int(res.valid.sum())

    def with_no_grad(fn):
        def run():
            with torch.no_grad():
                fn()
        return run

    entries = [
        ("resolve", lambda: DO.resolve(accum, alpha), 13 * plane),
        ("colorize, near / far given", lambda: DO.colorize(res.depth, res.valid, "disparity", 0.05, 1.0), 17 * plane),
        ("colorize, derived range", lambda: DO.colorize(res.depth, res.valid), 22 * plane),
        ("normals", lambda: DO.normals(res.depth, res.valid, cam), 18 * plane),
        ("normals_image", lambda: DO.normals_image(normals, nvalid), 25 * plane),
        ("unproject with colours and index (+ the read of count)", lambda: DO.unproject(res.depth, res.valid, cam, image=frame, return_index=True), 2 * plane + 16 * K + 28 * K),
        ("depth_metrics, B = 1, masked", lambda: DO.depth_metrics(res.depth, gt, res.valid), 9 * plane),
        ("depth_metrics, align = scale (two passes)", lambda: DO.depth_metrics(res.depth, gt, res.valid, align="scale"), 18 * plane),
        ("render_depth (one render of ones, resolve)", lambda: DO.render_depth(cam, pc, pipe, ITERATION, time=t), 0),
        ("render() of the same view, for scale", with_no_grad(lambda: render(cam, pc, pipe, bg, time=t, it=ITERATION)), 0),
    ]
    table = DO.depth_metrics(res.depth, gt, res.valid)[0].tolist()
    rng = DO.colorize(res.depth, res.valid, "depth", return_range=True)[1].tolist()
    lines = [f"depth probe on {torch.cuda.get_device_name(DEV)}: bench.py's synthetic scene, {pc.get_xyz.shape[0]} Gaussians, {W}x{H}, iteration {ITERATION}, the last "
             f"camera; hipEvent medians of {REPS} after one warm-up",
             f"valid pixels: {100 * K / plane:.1f} % ({K}); depth from {rng[0]:.3f} to {rng[1]:.3f}; pixels with a normal: {100 * float(nvalid.float().mean()):.1f} %; "
             f"against depth * (1 + N(0, 0.05)): AbsRel {table[1]:.4f}, RMSE {table[3]:.4f}, delta_1 {100 * table[5]:.2f} %",
             f"{'entry':<58}{'ms':>10}{'MB moved':>12}{'GB/s':>10}"]
    for name, fn, nbytes in entries:
        ms = timed(fn)
        lines.append(f"{name:<58}{ms:>10.3f}" + (f"{nbytes / 1e6:>12.1f}{nbytes / (ms * 1e-3) / 1e9:>10.1f}" if nbytes else f"{'':>12}{'':>10}"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "depth_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
