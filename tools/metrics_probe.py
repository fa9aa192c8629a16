#!/usr/bin/env python
"""Time gaussianprediction_amd.metrics.image_metrics (gp_image_metrics) against the float32 torch composition of the same
definitions (tests/metrics_ref.py on the same device): 1352 x 1014 and 800 x 800, B = 1 and 8, with and without MS-SSIM --
hipEvent-timed, median of 20 calls after 3 warm-ups; per pyramid level from the library's own hipEvent brackets
(gp_profile_enable: metrics_level0 .. 4, metrics_finalize).  Then views/s of metrics.evaluate_views against the bare
SpeculativeRenderer loop on bench.py's scene, and the number of synchronising torch calls the loop makes.  Writes
profiles/metrics_probe.txt.

    python tools/metrics_probe.py                 (everything)
    python tools/metrics_probe.py --kernels-only  (ten calls per configuration and nothing else: the body of a
                                                   `rocprofv3 --kernel-trace --stats -- python tools/metrics_probe.py --kernels-only` run)
    python tools/metrics_probe.py --trace-summary DIR/s_kernel_trace.csv   (no GPU: that run's trace per launch shape -- a pyramid
                                                   level is a grid size -- appended to profiles/metrics_probe.txt)
    python tools/metrics_probe.py --lpips         (only the LPIPS section: both nets at both sizes, B = 1, with the seeded weights
                                                   of tests/lpips_ref.py -- the call, the library's brackets per kernel, lpips_conv's
                                                   TF/s against the measured f32 MFMA peak, every convolution against
                                                   torch.nn.functional.conv2d on the same device.  Writes profiles/lpips_probe.txt)
"""
import os
import sys
import time
import warnings
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import metrics_ref as R  # noqa: E402
from gaussianprediction_amd import _lib, metrics as M  # noqa: E402

DEV = torch.device("cuda", 0)
SIZES = ((1014, 1352), (800, 800))


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


def pair(B, H, W):
    g = torch.Generator().manual_seed(1)
    gt = torch.nn.functional.interpolate(torch.rand(B, 3, H // 16, W // 16, generator=g), size=(H, W), mode="bicubic").clamp(0, 1)
    return (gt + 0.05 * torch.randn(B, 3, H, W, generator=g)).clamp(0, 1).to(DEV), gt.to(DEV)


def torch_composition(a, b, ms):
    r = R.all_metrics(a, b, with_ms=ms)
    return torch.stack([r[k] for k in (R.NAMES if ms else R.NAMES[:5])], dim=1)


def kernel_table(lines):
    lines.append(f"image_metrics (gp_image_metrics) vs the float32 torch composition on {torch.cuda.get_device_name(DEV)}; median of 20 (ms)")
    lines.append(f"{'H x W':>12s} {'B':>2s} {'MS-SSIM':>7s} {'hip ms':>8s} {'torch ms':>9s} {'speed-up':>8s}   per launch (ms): level0 .. level4, finalize")
    for H, W in SIZES:
        for B in (1, 8):
            a, b = pair(B, H, W)
            for ms in (True, False):
                t_hip = timed(lambda: M.image_metrics(a, b, ms_ssim=ms))
                t_t = timed(lambda: torch_composition(a, b, ms), reps=5, warm=2)
                _lib.profile_enable(2)
                _lib.profile_collect()
                for _ in range(10):
                    M.image_metrics(a, b, ms_ssim=ms)
                torch.cuda.synchronize()
                prof = _lib.profile_collect()
                _lib.profile_enable(0)
                names = [f"metrics_level{l}" for l in range(5 if ms else 1)] + ["metrics_finalize"]
                per = "  ".join(f"{prof[n][1] / max(prof[n][0], 1):.4f}" for n in names if n in prof)
                lines.append(f"{H:5d} x {W:4d} {B:2d} {'yes' if ms else 'no':>7s} {t_hip:8.3f} {t_t:9.3f} {t_t / t_hip:7.1f}x   {per}")
                # the distance between the two on this input (float32 torch against the kernels), for the record
                d = (M.image_metrics(a, b, ms_ssim=ms).table[:, :(7 if ms else 5)] - torch_composition(a, b, ms).double()).abs().max(0).values
                lines.append(f"{'':31s} max |hip - torch32| per column: " + " ".join(f"{float(x):.1e}" for x in d))


def eval_loop(lines):
    import bench
    args = SimpleNamespace(gaussians=1_000_000, width=1352, height=1014, keypoints=250, nearest_num=6, time_freq=8, iteration=50000,
                           scale_lo=0.003, scale_hi=0.012)
    pc, cams, gts, _ = bench.build_workload(args, DEV)
    from gaussianprediction_amd.renderer import SpeculativeRenderer
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    bg = torch.zeros(3, device=DEV)
    n = 50
    vc = [cams[i % len(cams)] for i in range(n)]
    vg = [gts[i % len(cams)] for i in range(n)]
    vt = [torch.from_numpy(c.time).float().to(DEV) for c in vc]
    sr = SpeculativeRenderer(pc, pipe, bg)
    with torch.no_grad():
        for i in range(16):                     # the exact first frame, then the high-water mark settles
            sr(vc[i], time=vt[i], it=args.iteration)
        sr.flush()
        torch.cuda.synchronize()
        reps = []
        for _ in range(3):
            t0 = time.perf_counter()
            for i in range(n):
                sr(vc[i], time=vt[i], it=args.iteration)
            again = sr.flush()
            torch.cuda.synchronize()
            reps.append(n / (time.perf_counter() - t0))
        bare = sorted(reps)[1]
    lines.append("")
    lines.append(f"eval loop on bench.py's scene (1 M Gaussians, 1352 x 1014, {n} views, ring of {sr.slots}); median of 3")
    lines.append(f"  bare SpeculativeRenderer loop                      {bare:8.1f} views/s   (re-rendered in the last loop: {again})")
    for label, kw in (("evaluate_views, quantize8 + MS-SSIM", dict(quantize8=True, ms_ssim=True)),
                      ("evaluate_views, quantize8, no MS-SSIM", dict(quantize8=True, ms_ssim=False))):
        M.evaluate_views(pc, vc, vg, pipe, bg, args.iteration, times=vt, renderer=sr, **kw)
        reps, res = [], None
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = M.evaluate_views(pc, vc, vg, pipe, bg, args.iteration, times=vt, renderer=sr, **kw)
            reps.append(n / (time.perf_counter() - t0))
        lines.append(f"  {label:50s} {sorted(reps)[1]:8.1f} views/s   (re-rendered: {res['rerendered']})  summary {res['summary']}")
    try:        # every synchronising torch call (a .cpu(), an .item()) warns in this mode: the loop's host reads, counted
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            M.evaluate_views(pc, vc, vg, pipe, bg, args.iteration, times=vt, renderer=sr)
        torch.cuda.set_sync_debug_mode("default")
        k = sum("synchroniz" in str(x.message).lower() for x in w)
        lines.append(f"  synchronising torch calls in one evaluate_views of {n} views: {k}   (one flush() per ring of {sr.slots} frames + the table read)")
    except Exception as e:      # noqa: BLE001  (a torch build without the mode: say so)
        torch.cuda.set_sync_debug_mode("default")
        lines.append(f"  synchronising torch calls: not counted ({type(e).__name__}: {e})")
    # the torch composition per view with one .item() per view, as an evaluation script composes it today
    with torch.no_grad():
        t0 = time.perf_counter()
        for i in range(n):
            img = sr(vc[i], time=vt[i], it=args.iteration)["render"]
            sr.flush()
            q = R.quantize8(img[None])
            float(R.ms_ssim(q, vg[i][None]).item()) + float(R.ssim(q, vg[i][None]).item()) + float(R.psnr(q, vg[i][None]).item())
        torch.cuda.synchronize()
        lines.append(f"  render + torch composition + .item() per view       {n / (time.perf_counter() - t0):8.1f} views/s")


def lpips_section():
    import lpips_ref as LR
    from gaussianprediction_amd import lpips as LP, peaks
    import torch.nn.functional as F
    lines = []
    peak = peaks.measure(str(DEV), gib=0.25, reps=5)["mfma_f32_TFLOPs"]
    lines.append(f"LPIPS (gp_lpips) on {torch.cuda.get_device_name(DEV)}, B = 1, seeded weights; hipEvent-timed, median of 20 after 3 warm-ups (ms)")
    lines.append(f"measured f32 MFMA peak (peaks.measure): {peak:.1f} TF/s")
    st = _lib.stream_ptr(DEV)
    for H, W in SIZES:
        a, b = pair(1, H, W)
        for net in ("vgg", "alex"):
            w = LR.seeded_weights(net)
            m = LP.LPIPS(net, w["backbone"], w["lin"], device=DEV)
            t_hip = timed(lambda: m(a, b))
            wd = {"backbone": {k: v.to(DEV) for k, v in w["backbone"].items()}, "lin": {k: v.to(DEV) for k, v in w["lin"].items()}}
            with torch.no_grad():
                try:
                    t_t = timed(lambda: LR.lpips_terms(a, b, net, wd, torch.float32), reps=20, warm=3)
                    d = float((m(a, b).table[0, 0] - LR.lpips_terms(a, b, net, wd, torch.float32)[0, 0].double()).abs())
                    torch_txt = f"{t_t:9.3f} ms ({t_t / t_hip:5.2f}x of hip)   |hip - torch32| {d:.1e}"
                except Exception as e:      # noqa: BLE001  (no convolution library on this device: say so)
                    torch_txt = f"not measured ({type(e).__name__}: {str(e)[:80]})"
            _lib.profile_enable(2)
            _lib.profile_collect()
            for _ in range(5):
                m(a, b)
            torch.cuda.synchronize()
            prof = _lib.profile_collect()
            _lib.profile_enable(0)
            # the convolutions' operations, from the library's table: 2 M K Cout each, M the output pixels of both images
            flop, h, wd_, taps, layers = 0.0, H, W, 0, []
            for e in LP.network_table(net):
                if taps == 5:
                    break
                if e.kind in (LP.CONV, LP.POOL):
                    hi, wi = h, wd_
                    h, wd_ = (h + 2 * e.pad - e.k) // e.stride + 1, (wd_ + 2 * e.pad - e.k) // e.stride + 1
                    if e.kind == LP.CONV:
                        f = 2.0 * 2 * h * wd_ * e.k * e.k * e.cin * e.cout
                        flop += f
                        layers.append((e, hi, wi, f))
                taps += e.tap
            conv_ms = prof["lpips_conv"][1] / 5
            lines.append("")
            lines.append(f"{net} {H} x {W}: gp_lpips {t_hip:8.3f} ms   torch float32 composition (F.conv2d / F.max_pool2d, same device) {torch_txt}")
            lines.append("  per call (ms, launches): " + "  ".join(f"{n} {prof[n][1] / 5:.3f} ({prof[n][0] // 5})" for n in
                         ("lpips_prepare", "lpips_conv", "lpips_pool", "lpips_dist", "lpips_finalize") if n in prof))
            lines.append(f"  lpips_conv: {flop / 1e12:.3f} TFLOP per pair in {conv_ms:.3f} ms = {flop / conv_ms / 1e9:.1f} TF/s = "
                         f"{100 * flop / conv_ms / 1e9 / peak:.0f} % of the measured f32 MFMA peak")
            lines.append(f"  {'conv':>4s} {'Cin':>4s} {'Cout':>4s} {'k':>2s} {'in H x W':>12s} {'GFLOP':>8s} {'hip ms':>8s} {'TF/s':>6s} {'torch ms':>9s} {'TF/s':>6s}")
            for e, hi, wi, f in layers:
                x = torch.randn(2, e.cin, hi, wi, device=DEV)
                xn = x.permute(0, 2, 3, 1).contiguous()
                wt, bt = w["backbone"][[k for k in w["backbone"] if k.endswith(".weight")][e.conv]].to(DEV), torch.zeros(e.cout, device=DEV)
                ho, wo = (hi + 2 * e.pad - e.k) // e.stride + 1, (wi + 2 * e.pad - e.k) // e.stride + 1
                y, pk = torch.empty(2, ho, wo, e.cout, device=DEV), torch.empty(wt.numel(), device=DEV)
                run = lambda: _lib.check(LP.lib().gp_lpips_conv2d_relu(xn, wt, bt, pk, y, 2, hi, wi, e.cin, e.cout, e.k, e.stride, e.pad, st), "conv")   # noqa: E731
                run()
                _lib.profile_enable(2)
                _lib.profile_collect()
                for _ in range(5):
                    run()
                torch.cuda.synchronize()
                t_l = _lib.profile_collect()["lpips_conv"][1] / 5
                _lib.profile_enable(0)
                try:
                    with torch.no_grad():
                        t_tl = timed(lambda: F.relu(F.conv2d(x, wt, bt, stride=e.stride, padding=e.pad)), reps=10, warm=2)
                    tt = f"{t_tl:9.3f} {f / t_tl / 1e9:6.1f}"
                except Exception as ex:      # noqa: BLE001
                    tt = f"not measured ({type(ex).__name__})"
                lines.append(f"  {e.conv:4d} {e.cin:4d} {e.cout:4d} {e.k:2d} {f'{hi} x {wi}':>12s} {f / 1e9:8.2f} {t_l:8.3f} {f / t_l / 1e9:6.1f} {tt}")
                del x, xn, y
            del m
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "lpips_probe.txt"), "w") as f:
        f.write(text)


def trace_summary(path):
    """Mean duration per (kernel, grid) of a rocprofv3 kernel trace, in order of first appearance."""
    import csv
    groups = {}
    for row in csv.DictReader(open(path)):
        if "gp_metric" not in row["Kernel_Name"]:
            continue
        name = row["Kernel_Name"].split("(")[0].replace("void ", "")
        wg = int(row["Workgroup_Size_X"])
        key = (name, int(row["Grid_Size_X"]) // wg, int(row["Grid_Size_Y"]), int(row["Grid_Size_Z"]))
        groups.setdefault(key, []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    lines = ["", "rocprofv3 --kernel-trace --stats -- python tools/metrics_probe.py --kernels-only: mean per launch shape (a pyramid level is a grid)",
             f"{'kernel':34s} {'workgroups x, y, planes':>24s} {'calls':>6s} {'mean us':>9s} {'min us':>8s}"]
    for (name, gx, gy, gz), d in groups.items():
        lines.append(f"{name:34s} {f'{gx} x {gy} x {gz}':>24s} {len(d):6d} {sum(d) / len(d) / 1e3:9.2f} {min(d) / 1e3:8.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(os.path.join(ROOT, "profiles", "metrics_probe.txt"), "a") as f:
        f.write(text)


def main():
    if "--trace-summary" in sys.argv:
        trace_summary(sys.argv[sys.argv.index("--trace-summary") + 1])
        return
    if "--lpips" in sys.argv:
        lpips_section()
        return
    if "--kernels-only" in sys.argv:
        for H, W in SIZES:
            for B in (1, 8):
                a, b = pair(B, H, W)
                for ms in (True, False):
                    for _ in range(10):
                        M.image_metrics(a, b, ms_ssim=ms)
        torch.cuda.synchronize()
        return
    lines = []
    kernel_table(lines)
    if "--no-eval-loop" not in sys.argv:
        eval_loop(lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "metrics_probe.txt"), "w") as f:
        f.write(text)
    if "--no-lpips" not in sys.argv:
        lpips_section()


if __name__ == "__main__":
    main()
