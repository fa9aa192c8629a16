"""The self-synchronising JPEG entropy stage (jpeg_sync / include/gp_jpeg_sync.h) measured on the GPU against the one-lane path of the
same build (jpeg_decode / gp_jpeg_decode on a file without restart markers: the path such a file took before) and against Pillow on this
host with one thread and with a pool of 16.  Pillow-written files without restart markers at 1352 x 1014 and 800 x 800, 4:2:0 and
4:4:4, B = 1, 8 and 32: the two frames of tools/jpeg_decode_probe.py (white background + blob, full-frame noisy texture), a
natural-like frame (a smooth field + sigma-4 noise) and a constant frame.  The two device paths alternate in one process, ROUNDS times
each, hipEvent-timed; a row holds the median of each path's round medians and their spread (largest - smallest round median).  Also
the info words per file.  Writes profiles/jpeg_sync_probe.txt.

    python tools/jpeg_sync_probe.py            (needs a GPU)
"""
import io
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import png_probe  # noqa: E402  (its frames and its timer)
from gaussianprediction_amd import jpeg_decode as JD, jpeg_sync as JS  # noqa: E402

DEV = torch.device("cuda", 0)
SIZES = ((1014, 1352), (800, 800))
QUALITY = 90
ROUNDS = 3
OUT = os.path.join(ROOT, "profiles", "jpeg_sync_probe.txt")


def pillow_file(q, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(q.permute(1, 2, 0).numpy()).save(buf, format="JPEG", quality=QUALITY, **kw)
    return buf.getvalue()


def pillow_decode(data):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)))


def frames(H, W):
    fr = png_probe.frames(H, W)
    g = torch.Generator().manual_seed(2)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    smooth = torch.stack([0.5 + 0.3 * torch.sin(xx / 40.0 + c) * torch.cos(yy / 55.0 - c) for c in range(3)])
    return {"white background + blob": fr["white background + blob"], "full-frame noisy texture": fr["full-frame noisy texture"],
            "natural-like (sigma 4)": (smooth + (4.0 / 255.0) * torch.randn(3, H, W, generator=g)).clamp(0, 1),
            "constant white": torch.ones(3, H, W)}


def emit(lines, text):
    lines.append(text)
    print(text, flush=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    lines = []
    emit(lines, f"gp_jpeg_sync_decode against gp_jpeg_decode (one lane per file) on {torch.cuda.get_device_name(DEV)}: Pillow-written files without restart markers, "
                 f"quality {QUALITY}; float32 output;")
    emit(lines, f"S = {JS.S} B, C = {JS.C}; the launches alone, hipEvent-timed; the two paths alternate, {ROUNDS} rounds each: sync = median of 10 after 2 warm-ups per round, "
                 "one lane = median of 3 after 1; ms per image")
    emit(lines, f"{'H x W':>12s} {'sub':>5s} {'B':>3s} {'frame':>26s} {'MB/file':>8s} {'sync':>8s} {'spread':>7s} {'one lane':>9s} {'spread':>7s} {'ratio':>7s}"
                 f" {'Pillow x1':>10s} {'Pillow x16':>11s}  info (subsequences, chunks, rounds in a chunk, rounds across)")
    pool16 = ThreadPoolExecutor(16)
    for H, W in SIZES:
        for name, img in frames(H, W).items():
            q = img.clamp(0, 1).mul(255).add(0.5).floor().clamp(0, 255).to(torch.uint8)
            for sub, label in ((2, "4:2:0"), (0, "4:4:4")):
                data = pillow_file(q, subsampling=sub)
                ref = (torch.from_numpy(pillow_decode(data)).permute(2, 0, 1).to(torch.float32) / 255.0).to(DEV)
                t0 = time.perf_counter()
                for _ in range(3):
                    pillow_decode(data)
                p1 = (time.perf_counter() - t0) / 3 * 1e3
                t0 = time.perf_counter()
                list(pool16.map(pillow_decode, [data] * 32))
                p16 = (time.perf_counter() - t0) / 32 * 1e3
                for B in (1, 8, 32):
                    items = [JD.parse(data, f"{name}-{k}") for k in range(B)]
                    assert all(JS.eligible(it) for it in items)
                    shapes = JD.groups(items)
                    staged = JD.stage(items, shapes)
                    up = staged.buffer.to(DEV)
                    kw = dict(device=DEV, dtype=torch.float32)
                    words = torch.empty(B, dtype=torch.int32, device=DEV)
                    sync_words = torch.empty(B, 5, dtype=torch.int32, device=DEV)
                    (slow,) = JD.launch(staged, up, shapes, words, **kw)
                    (fast,), _ = JS.launch(staged, up, shapes, sync_words, **kw)
                    read = sync_words.cpu().reshape(-1).tolist()
                    assert not words.cpu().any() and read[:B] == [0] * B and torch.equal(fast, slow) and torch.equal(fast[B - 1].view(3, H, W), ref)
                    ts, tl = [], []
                    for _ in range(ROUNDS):
                        ts.append(png_probe.timed(lambda: JS.launch(staged, up, shapes, sync_words, **kw), 10, 2))
                        tl.append(png_probe.timed(lambda: JD.launch(staged, up, shapes, words, **kw), 3, 1))
                    ms, ml = sorted(ts)[ROUNDS // 2], sorted(tl)[ROUNDS // 2]
                    emit(lines, f"{H:5d} x {W:4d} {label:>5s} {B:3d} {name:>26s} {len(data) / 1e6:8.2f} {ms / B:8.3f} {(max(ts) - min(ts)) / B:7.3f} {ml / B:9.3f}"
                                 f" {(max(tl) - min(tl)) / B:7.3f} {ml / ms:7.1f} {p1:10.1f} {p16:11.2f}  {tuple(read[B:B + 4])}")
    pool16.shutdown()
    emit(lines, "sync / one lane: the median of the path's round medians; spread: the largest less the smallest round median; ratio: one lane / sync;")
    emit(lines, "Pillow x1 / x16: np.array(Image.open(...)) of the same file on this host, one thread / a pool of 16, per image")


if __name__ == "__main__":
    main()
