"""On-device JPEG decoding (jpeg_decode / include/gp_jpeg_decode.h) measured on the GPU: gp_jpeg_decode per image at 1352 x 1014 and
800 x 800 with B = 1, 8 and 32, on files jpeg_ops wrote at 4:2:0 and 4:4:4 (a restart marker every 8 MCUs), on Pillow-written files of
the same frames with restart_marker_blocks=8 and on Pillow-written files without restart markers (one interval: the serial path),
hipEvent-timed with the host-to-device copy of the staging buffer and again without it, and the host parse per file; Pillow on this host
for the same files with one thread and with a pool of 16; gp_png_decode on the same frames in the same run; and metrics.evaluate_dirs
with and without device_decode on a 50-view directory written by eval_render.render_set whose gt directory is re-saved as JPEG.
Writes profiles/jpeg_decode_probe.txt.

    python tools/jpeg_decode_probe.py            (needs a GPU)
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
from gaussianprediction_amd import eval_render as ER, jpeg_decode as JD, jpeg_ops as JPG, metrics as M, png_decode as PD, png_ops as PNG  # noqa: E402

DEV = torch.device("cuda", 0)
SIZES = ((1014, 1352), (800, 800))
FRAMES = ("white background + blob", "full-frame noisy texture")
QUALITY = 90


def pillow_file(q, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(q.permute(1, 2, 0).numpy()).save(buf, format="JPEG", quality=QUALITY, **kw)
    return buf.getvalue()


def pillow_decode(data):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)))


def emit(lines, text):
    lines.append(text)
    print(text, flush=True)


def reps_for(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (20, 3) if time.perf_counter() - t0 < 0.05 else (5, 1)


def decode_table(lines):
    emit(lines, f"gp_jpeg_decode on {torch.cuda.get_device_name(DEV)}: float32 output; quality {QUALITY}; hipEvent-timed, median of 20 after 3 warm-ups "
                 "(5 after 1 where a call takes over 50 ms); ms per image")
    emit(lines, f"{'H x W':>12s} {'B':>3s} {'frame':>26s} {'file':>22s} {'lanes':>6s} {'MB/file':>8s} {'with copy':>10s} {'kernels':>9s} {'staging':>9s}"
                 f" {'Pillow x1':>10s} {'Pillow x16':>11s}")
    pool16 = ThreadPoolExecutor(16)
    for H, W in SIZES:
        fr = png_probe.frames(H, W)
        for name in FRAMES:
            q = fr[name].clamp(0, 1).mul(255).add(0.5).floor().clamp(0, 255).to(torch.uint8)
            files = {"jpeg_ops 4:2:0": JPG.encode_to_bytes(q.to(DEV), quality=QUALITY, subsampling="420")[0],
                     "jpeg_ops 4:4:4": JPG.encode_to_bytes(q.to(DEV), quality=QUALITY, subsampling="444")[0],
                     "Pillow 4:2:0 restart 8": pillow_file(q, subsampling=2, restart_marker_blocks=8),
                     "Pillow 4:2:0 no restart": pillow_file(q, subsampling=2)}
            for writer, data in files.items():
                ref = torch.from_numpy(pillow_decode(data)).permute(2, 0, 1)
                t0 = time.perf_counter()
                for _ in range(3):
                    pillow_decode(data)
                p1 = (time.perf_counter() - t0) / 3 * 1e3
                t0 = time.perf_counter()
                list(pool16.map(pillow_decode, [data] * 32))
                p16 = (time.perf_counter() - t0) / 32 * 1e3
                for B in (1, 8, 32):
                    t0 = time.perf_counter()
                    items = [JD.parse(data, f"{writer}-{k}") for k in range(B)]
                    shapes = JD.groups(items)
                    staged = JD.stage(items, shapes)
                    host_ms = (time.perf_counter() - t0) * 1e3
                    words = torch.empty(B, dtype=torch.int32, device=DEV)
                    kw = dict(device=DEV, dtype=torch.float32)
                    up = staged.buffer.to(DEV)
                    (dst,) = JD.launch(staged, up, shapes, words, **kw)
                    assert not words.cpu().any() and torch.equal(dst[B - 1].view(3, H, W), (ref.to(torch.float32) / 255.0).to(DEV))
                    reps, warm = reps_for(lambda: JD.launch(staged, up, shapes, words, **kw))
                    kern = png_probe.timed(lambda: JD.launch(staged, up, shapes, words, **kw), reps, warm)
                    both = png_probe.timed(lambda: JD.launch(staged, staged.buffer.to(DEV, non_blocking=True), shapes, words, **kw), reps, warm)
                    emit(lines, f"{H:5d} x {W:4d} {B:3d} {name:>26s} {writer:>22s} {items[0].nseg:6d} {len(data) / 1e6:8.2f} {both / B:10.3f} {kern / B:9.3f}"
                                 f" {host_ms / B:9.3f} {p1:10.1f} {p16:11.2f}")
            data = PNG.encode_to_bytes(q.to(DEV))[0]                # the same frame through gp_png_decode (banded), in the same run
            for B in (1, 8, 32):
                items = [PD.parse(data, f"png-{k}") for k in range(B)]
                shapes = PD.groups(items, 3)
                staged = PD.stage(items, [it.banded for it in items], shapes)
                words = torch.empty(2, B, dtype=torch.int32, device=DEV)
                kw = dict(device=DEV, dtype=torch.float32, background=None)
                up = staged.buffer.to(DEV)
                PD.launch(staged, up, shapes, words, **kw)
                assert not words.cpu()[0].any()
                reps, warm = reps_for(lambda: PD.launch(staged, up, shapes, words, **kw))
                kern = png_probe.timed(lambda: PD.launch(staged, up, shapes, words, **kw), reps, warm)
                both = png_probe.timed(lambda: PD.launch(staged, staged.buffer.to(DEV, non_blocking=True), shapes, words, **kw), reps, warm)
                emit(lines, f"{H:5d} x {W:4d} {B:3d} {name:>26s} {'gp_png_decode (banded)':>22s} {len(items[0].pieces):6d} {len(data) / 1e6:8.2f} {both / B:10.3f} {kern / B:9.3f}")
    pool16.shutdown()
    emit(lines, "lanes: restart intervals of a file = lanes of the entropy kernel (for the PNG rows: bands = workgroups); with copy: the staging buffer's")
    emit(lines, "host-to-device copy and the four launches; kernels: the launches alone; staging: parse and the copy into the pinned buffer, on one host")
    emit(lines, "thread; Pillow x1 / x16: np.array(Image.open(...)) of the same file, one thread / a pool of 16, per image")


def loop_table(lines, n=50):
    from PIL import Image
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
    root = tempfile.mkdtemp(prefix="jpeg_decode_probe_")
    try:
        ER.render_set(root, "test", args.iteration, views, pc, pipe, bg, renderer=sr)
        path = os.path.join(root, "eval", "test") if os.path.isdir(os.path.join(root, "eval", "test")) else os.path.join(root, "test")
        for method in sorted(os.listdir(path)):                 # the gt directory re-saved as JPEG: once by Pillow's defaults for a dataset
            gdir = os.path.join(path, method, "gt")             # dump (quality 95, 4:2:0, no restart markers), once by jpeg_ops
            if not os.path.isdir(gdir):
                continue
            for f in sorted(os.listdir(gdir)):
                img = Image.open(os.path.join(gdir, f)).convert("RGB")
                os.remove(os.path.join(gdir, f))
                img.save(os.path.join(gdir, f[:-4] + ".jpg"), quality=95)
        for kind in ("Pillow-written gt (no restart markers)", "jpeg_ops-written gt (4:2:0, 680 intervals)"):
            times = {}
            for label, kw in (("host decode (Pillow, file by file)", dict()), ("device_decode=True (groups of 16 pairs)", dict(device_decode=True))):
                results, ts = None, []
                for rep in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    results = M.evaluate_dirs(path, device=DEV, write=False, **kw)
                    ts.append(time.perf_counter() - t0)
                times[label] = (sorted(ts[1:])[0], results)
            (ta, ra), (tb, rb) = times.values()
            assert ra == rb
            emit(lines, "")
            emit(lines, f"metrics.evaluate_dirs(write=False) on {n} views written by render_set (bench.py's scene, 1352 x 1014, {n} .png renders + {n} .jpg gt): {kind};")
            emit(lines, "best of 2 after a warm-up; equal results")
            for label, (t, _) in times.items():
                emit(lines, f"  {label:40s} {t * 1e3:9.1f} ms   {t / n * 1e3:7.2f} ms / view")
            emit(lines, f"  ratio {ta / tb:6.2f} x")
            for method in sorted(os.listdir(path)):             # ... and now by this project's encoder
                gdir = os.path.join(path, method, "gt")
                if not os.path.isdir(gdir):
                    continue
                for f in sorted(os.listdir(gdir)):
                    q = torch.from_numpy(np.array(Image.open(os.path.join(gdir, f)))).permute(2, 0, 1).contiguous().to(DEV)
                    with open(os.path.join(gdir, f), "wb") as fp:
                        fp.write(JPG.encode_to_bytes(q, quality=95, subsampling="420")[0])
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    lines = []
    decode_table(lines)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "jpeg_decode_probe.txt"), "w") as f:
        f.write(text)
    loop_table(lines)
    text = "\n".join(lines) + "\n"
    with open(os.path.join(ROOT, "profiles", "jpeg_decode_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
