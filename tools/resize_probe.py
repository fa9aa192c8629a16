"""On-device image resizing (resize_ops / include/gp_resize.h) measured on the GPU against Pillow on this host: the workload's
shape, 1352 x 1014 -> 676 x 507 RGB with the bicubic filter, B = 1 and B = 16, uint8 and float32 output, hipEvent-timed, the result
checked against Pillow's bytes first; an RGBA batch (premultiplied alpha); the single-pass and the two-launch paths for comparison;
and Pillow's Image.resize of the same images with one thread and with a pool of 16.  Writes profiles/resize_probe.txt.

    python tools/resize_probe.py            (needs a GPU)
"""
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
from gaussianprediction_amd import resize_ops as R  # noqa: E402

DEV = torch.device("cuda", 0)
PATHS = {R.PATH_COPY: "copy", R.PATH_FUSED: "fused", R.PATH_TWO_LAUNCH: "two-launch", R.PATH_HORIZONTAL: "horizontal", R.PATH_VERTICAL: "vertical"}
# (C, source W x H, target W x H, filter)
CASES = ((3, (1352, 1014), (676, 507), "bicubic"), (4, (1352, 1014), (676, 507), "bicubic"), (3, (1352, 1014), (676, 507), "lanczos"),
         (3, (800, 800), (400, 400), "bicubic"), (3, (1352, 1014), (676, 1014), "bicubic"), (3, (1352, 1014), (1352, 507), "bicubic"),
         (3, (1352, 1014), (21, 15), "bicubic"))


def pillow_image(planes):
    from PIL import Image
    C = planes.shape[0]
    return Image.fromarray(planes[0] if C == 1 else np.ascontiguousarray(planes.transpose(1, 2, 0)), {1: "L", 3: "RGB", 4: "RGBA"}[C])


def planar(im):
    arr = np.array(im)
    return arr[None] if arr.ndim == 2 else np.ascontiguousarray(arr.transpose(2, 0, 1))


def main():
    lines = [f"resize_ops.resize on {torch.cuda.get_device_name(DEV)}: hipEvent-timed, median of 20 after 3 warm-ups, tables cached; ms per image.  Every result",
             "was first compared with Pillow's bytes.  Pillow x1 / x16: Image.resize of the same image on this host, one thread / a pool of 16, per image.",
             f"{'C':>2s} {'source':>12s} {'target':>12s} {'filter':>8s} {'path':>10s} {'B':>3s} {'uint8':>8s} {'float32':>8s} {'Pillow x1':>10s} {'Pillow x16':>11s} {'x1 / uint8':>11s}"]
    pool16 = ThreadPoolExecutor(16)
    for C, (W, H), size, name in CASES:
        frame = png_probe.frames(H, W)["full-frame noisy texture"].mul(255).add(0.5).floor().clamp(0, 255).to(torch.uint8).numpy()
        if C == 4:
            alpha = np.random.default_rng(0).choice(np.array([0, 1, 77, 200, 255], np.uint8), size=(1, H, W))
            frame = np.concatenate([frame, alpha])
        frame = frame[:C]
        im = pillow_image(frame)
        flt = R.FILTERS[name]
        want = planar(im.resize(size, flt))
        t0 = time.perf_counter()
        for _ in range(3):
            im.resize(size, flt)
        p1 = (time.perf_counter() - t0) / 3 * 1e3
        t0 = time.perf_counter()
        list(pool16.map(lambda _: im.resize(size, flt), range(32)))
        p16 = (time.perf_counter() - t0) / 32 * 1e3
        for B in (1, 16):
            x = torch.from_numpy(frame).to(DEV)[None].repeat(B, 1, 1, 1)
            got = R.resize(x, size, name)
            assert np.array_equal(got[B - 1].cpu().numpy(), want), (C, W, H, size, name)
            out8 = torch.empty_like(got)
            out32 = torch.empty(got.shape, dtype=torch.float32, device=DEV)
            u8 = png_probe.timed(lambda: R.resize(x, size, name, out=out8)) / B
            f32 = png_probe.timed(lambda: R.resize(x, size, name, dtype=torch.float32, out=out32)) / B
            assert torch.equal(out32.cpu(), out8.cpu().to(torch.float32) / 255.0)          # (the division on the host: true division)
            lines.append(f"{C:2d} {W:5d} x {H:4d} {size[0]:5d} x {size[1]:4d} {name:>8s} {PATHS[R.path((W, H), size, name)]:>10s} {B:3d} {u8:8.4f} {f32:8.4f}"
                         f" {p1:10.2f} {p16:11.3f} {p1 / u8:11.1f}")
    pool16.shutdown()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "resize_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
