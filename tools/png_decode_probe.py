"""On-device PNG decoding (png_decode / include/gp_png_decode.h) measured on the GPU: gp_png_decode per image at 1352 x 1014 and 800 x 800
with B = 1, 8 and 32, on files png_ops wrote (banded) and on Pillow-written files of the same frames (serial), hipEvent-timed with the
host-to-device copy of the staging buffer and again without it; Pillow on this host for the same files with one thread and with a pool
of 16 (what metrics._load_rgb costs); and metrics.evaluate_dirs with and without device_png on a 50-view directory written by
eval_render.render_set.  Writes profiles/png_decode_probe.txt.

    python tools/png_decode_probe.py            (needs a GPU)
"""
import io
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import png_probe  # noqa: E402  (its frames and its timer)
from gaussianprediction_amd import eval_render as ER, metrics as M, png_decode as PD, png_ops as PNG  # noqa: E402

DEV = torch.device("cuda", 0)
SIZES = ((1014, 1352), (800, 800))
FRAMES = ("white background + blob", "full-frame noisy texture")


def pillow_file(q):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(q.permute(1, 2, 0).numpy()).save(buf, format="PNG")
    return buf.getvalue()


def pillow_decode(data):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)))


def decode_table(lines):
    lines.append(f"gp_png_decode on {torch.cuda.get_device_name(DEV)}: float32 output, three channels; hipEvent-timed, median of 20 after 3 warm-ups "
                 "(5 after 1 where a call takes over 50 ms); ms per image")
    lines.append(f"{'H x W':>12s} {'B':>3s} {'frame':>26s} {'written by':>10s} {'mode':>7s} {'MB/file':>8s} {'with copy':>10s} {'kernels':>9s} {'staging':>9s}"
                 f" {'Pillow x1':>10s} {'Pillow x16':>11s}")
    pool16 = ThreadPoolExecutor(16)
    for H, W in SIZES:
        fr = png_probe.frames(H, W)
        for name in FRAMES:
            q = fr[name].clamp(0, 1).mul(255).add(0.5).floor().clamp(0, 255).to(torch.uint8)
            files = {"png_ops": PNG.encode_to_bytes(q.to(DEV))[0], "Pillow": pillow_file(q)}
            for writer, data in files.items():
                ref = torch.from_numpy(pillow_decode(data)).permute(2, 0, 1)
                assert torch.equal(ref, q)
                t0 = time.perf_counter()
                for _ in range(3):
                    pillow_decode(data)
                p1 = (time.perf_counter() - t0) / 3 * 1e3
                t0 = time.perf_counter()
                list(pool16.map(pillow_decode, [data] * 32))
                p16 = (time.perf_counter() - t0) / 32 * 1e3
                for B in (1, 8, 32):
                    t0 = time.perf_counter()
                    items = [PD.parse(data, f"{writer}-{k}") for k in range(B)]
                    banded = [it.banded for it in items]
                    shapes = PD.groups(items, 3)
                    staged = PD.stage(items, banded, shapes)
                    host_ms = (time.perf_counter() - t0) * 1e3
                    words = torch.empty(2, B, dtype=torch.int32, device=DEV)
                    kw = dict(device=DEV, dtype=torch.float32, background=None)
                    up = staged.buffer.to(DEV)
                    (dst,) = PD.launch(staged, up, shapes, words, **kw)
                    w = words.cpu()
                    assert not w[0].any() and torch.equal(dst[B - 1].view(3, H, W), (q.to(torch.float32) / 255.0).to(DEV))
                    mode = {PD.MODE_BANDED: "banded", PD.MODE_SERIAL: "serial"}[int(w[1, 0])]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    PD.launch(staged, up, shapes, words, **kw)
                    torch.cuda.synchronize()
                    reps, warm = (20, 3) if time.perf_counter() - t0 < 0.05 else (5, 1)
                    kern = png_probe.timed(lambda: PD.launch(staged, up, shapes, words, **kw), reps, warm)
                    both = png_probe.timed(lambda: PD.launch(staged, staged.buffer.to(DEV, non_blocking=True), shapes, words, **kw), reps, warm)
                    lines.append(f"{H:5d} x {W:4d} {B:3d} {name:>26s} {writer:>10s} {mode:>7s} {len(data) / 1e6:8.2f} {both / B:10.3f} {kern / B:9.3f} {host_ms / B:9.3f}"
                                 f" {p1:10.1f} {p16:11.2f}")
    pool16.shutdown()
    lines.append("with copy: the staging buffer's host-to-device copy and the four launches; kernels: the launches alone; staging: parse (every CRC-32) and the")
    lines.append("copy into the pinned buffer, on one host thread; Pillow x1 / x16: np.array(Image.open(...)) of the same file, one thread / a pool of 16, per image")


def loop_table(lines, n=50):
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
    sr = SpeculativeRenderer(pc, pipe, bg)
    with torch.no_grad():
        for v in views[:16]:                    # the exact first frame, then the high-water mark settles
            sr(v, time=torch.from_numpy(v.time).float().to(DEV), it=args.iteration)
        sr.flush()
    root = tempfile.mkdtemp(prefix="png_decode_probe_")
    try:
        ER.render_set(root, "test", args.iteration, views, pc, pipe, bg, renderer=sr)
        path = os.path.join(root, "eval", "test") if os.path.isdir(os.path.join(root, "eval", "test")) else os.path.join(root, "test")
        times = {}
        for label, kw in (("host decode (Pillow, file by file)", dict()), ("device_png=True (groups of 16 pairs)", dict(device_png=True))):
            results, ts = None, []
            for rep in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                results = M.evaluate_dirs(path, device=DEV, write=False, **kw)
                ts.append(time.perf_counter() - t0)
            times[label] = (sorted(ts[1:])[0], results)
        (ta, ra), (tb, rb) = times.values()
        assert ra == rb
    finally:
        shutil.rmtree(root, ignore_errors=True)
    lines.append("")
    lines.append(f"metrics.evaluate_dirs(write=False) on {n} views written by render_set (bench.py's scene, 1352 x 1014, {2 * n} files); best of 2 after a warm-up; equal results")
    for label, (t, _) in times.items():
        lines.append(f"  {label:40s} {t * 1e3:9.1f} ms   {t / n * 1e3:7.2f} ms / view")
    lines.append(f"  ratio {ta / tb:6.2f} x")


def main():
    lines = []
    decode_table(lines)
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    loop_table(lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "png_decode_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
