"""On-device PNG encoding (png_ops / include/gp_png.h) measured on the GPU: gp_png_encode per frame at 1352 x 1014 and 800 x 800 with
B = 1 and 32, hipEvent-timed, median of 20 calls after 3 warm-ups; the files' bytes against Pillow's compress_level 1 and 6 for the same
frames; and eval_render.render_set to disk on bench.py's scene with PngWriter against the same loop through motion._save_png (one
device-to-host read and one host encode per file), in views/s.  Writes profiles/png_probe.txt.

    python tools/png_probe.py            (needs a GPU)
"""
import io
import os
import shutil
import sys
import tempfile
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gaussianprediction_amd import eval_render as ER, motion, png_ops as PNG  # noqa: E402

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


def frames(H, W):
    """{name: float32 [3, H, W]}: a white background with a noisy blob, a full-frame noisy texture, a smooth frame with sigma-1 noise."""
    g = torch.Generator().manual_seed(1)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    smooth = torch.nn.functional.interpolate(torch.rand(1, 3, H // 16 + 1, W // 16 + 1, generator=g), size=(H, W), mode="bicubic")[0].clamp(0, 1)
    inside = ((yy - H / 2) ** 2 + (xx - W / 2) ** 2 < (0.3 * min(H, W)) ** 2)[None]
    blob = torch.where(inside, (smooth + 0.03 * torch.randn(3, H, W, generator=g)).clamp(0, 1), torch.ones(3, H, W))
    texture = (smooth + 0.06 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    sigma1 = (smooth + (1.0 / 255.0) * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    return {"white background + blob": blob, "full-frame noisy texture": texture, "smooth, sigma-1 noise": sigma1}


def pillow_bytes(img, level):
    from PIL import Image
    a = img.clamp(0, 1).mul(255).add(0.5).clamp(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()
    buf = io.BytesIO()
    t0 = time.perf_counter()
    Image.fromarray(a).save(buf, format="PNG", compress_level=level)
    return len(buf.getvalue()), (time.perf_counter() - t0) * 1e3


def encode_table(lines):
    lines.append(f"gp_png_encode on {torch.cuda.get_device_name(DEV)}: band {PNG.BAND_BYTES} B; hipEvent-timed, median of 20 after 3 warm-ups")
    lines.append(f"{'H x W':>12s} {'B':>3s} {'frame':>26s} {'ms / call':>10s} {'ms / frame':>11s}")
    for H, W in SIZES:
        fr = frames(H, W)
        for B in (1, 32):
            for name, img in fr.items():
                x = img.to(DEV)[None].expand(B, -1, -1, -1).contiguous()
                out = torch.empty(B, PNG.bound(H, W), dtype=torch.uint8, device=DEV)
                t = timed(lambda: PNG.encode(x, out=out))
                lines.append(f"{H:5d} x {W:4d} {B:3d} {name:>26s} {t:10.3f} {t / B:11.3f}")
    lines.append("")
    lines.append("bytes out against Pillow on this host's CPU (whole-image compress_level 1 and 6) for the same frames")
    lines.append(f"{'H x W':>12s} {'frame':>26s} {'gp_png':>10s} {'Pillow 1':>10s} {'(ms)':>7s} {'Pillow 6':>10s} {'(ms)':>7s} {'vs 1':>6s} {'vs 6':>6s}")
    for H, W in SIZES:
        for name, img in frames(H, W).items():
            ours = len(PNG.encode_to_bytes(img.to(DEV))[0])
            (p1, t1), (p6, t6) = pillow_bytes(img, 1), pillow_bytes(img, 6)
            lines.append(f"{H:5d} x {W:4d} {name:>26s} {ours:10d} {p1:10d} {t1:7.1f} {p6:10d} {t6:7.1f} {ours / p1:6.3f} {ours / p6:6.3f}")


def host_render_set(render_path, gts_path, views, times, pc, pipe, bg, iteration, sr):
    """render_set's loop with the host encoder: the ring is flushed, then every frame and ground truth goes through motion._save_png."""
    ring = []

    def close_ring():
        sr.flush()
        for i, image, gt in ring:
            motion._save_png(image, os.path.join(render_path, f"{i:05d}.png"))
            motion._save_png(gt, os.path.join(gts_path, f"{i:05d}.png"))
        ring.clear()

    with torch.no_grad():
        for i, view in enumerate(views):
            if len(ring) >= sr.slots:
                close_ring()
            ring.append((i, sr(view, time=times[i], it=iteration)["render"], view.original_image))
        close_ring()


def loop_table(lines, n=32):
    import bench
    from gaussianprediction_amd.renderer import SpeculativeRenderer
    args = SimpleNamespace(gaussians=1_000_000, width=1352, height=1014, keypoints=250, nearest_num=6, time_freq=8, iteration=50000,
                           scale_lo=0.003, scale_hi=0.012)
    pc, cams, gts, _ = bench.build_workload(args, DEV)
    for cam, gt in zip(cams, gts):
        cam.original_image = gt
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    bg = torch.zeros(3, device=DEV)
    views = [cams[i % len(cams)] for i in range(n)]
    times = [torch.from_numpy(c.time).float().to(DEV) for c in views]
    sr = SpeculativeRenderer(pc, pipe, bg)
    with torch.no_grad():
        for i in range(16):                     # the exact first frame, then the high-water mark settles
            sr(views[i], time=times[i], it=args.iteration)
        sr.flush()
    root = tempfile.mkdtemp(prefix="png_probe_")
    try:
        ER.render_set(os.path.join(root, "warm"), "test", args.iteration, views[:4], pc, pipe, bg, renderer=sr)
        dev_rates, host_rates = [], []
        for rep in range(3):
            _, stats = ER.render_set(os.path.join(root, f"device{rep}"), "test", args.iteration, views, pc, pipe, bg, renderer=sr)
            dev_rates.append(stats["views_per_s"])
        for rep in range(2):
            rp, gp = os.path.join(root, f"host{rep}", "renders"), os.path.join(root, f"host{rep}", "gt")
            os.makedirs(rp)
            os.makedirs(gp)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_render_set(rp, gp, views, times, pc, pipe, bg, args.iteration, sr)
            host_rates.append(n / (time.perf_counter() - t0))
        size = sum(os.path.getsize(os.path.join(root, "device0", "eval", "test", f"ours_{args.iteration}", d, f))
                   for d in ("renders", "gt") for f in os.listdir(os.path.join(root, "device0", "eval", "test", f"ours_{args.iteration}", d)))
        hsize = sum(os.path.getsize(os.path.join(root, "host0", d, f)) for d in ("renders", "gt") for f in os.listdir(os.path.join(root, "host0", d)))
    finally:
        shutil.rmtree(root, ignore_errors=True)
    dev, host = sorted(dev_rates)[1], max(host_rates)
    lines.append("")
    lines.append(f"render_set to disk on bench.py's scene (1 M Gaussians, 1352 x 1014, {n} views, render + ground truth = {2 * n} files, ring of {sr.slots})")
    lines.append(f"  PngWriter (device encode, pinned copies, 2 writer threads)   {dev:8.1f} views/s   median of 3   {size / 2 / n / 1e6:6.2f} MB / file")
    lines.append(f"  motion._save_png (read back + Pillow, frame by frame)        {host:8.1f} views/s   best of 2     {hsize / 2 / n / 1e6:6.2f} MB / file")
    lines.append(f"  ratio                                                        {dev / host:8.1f} x")


def main():
    lines = []
    encode_table(lines)
    loop_table(lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "png_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
