"""On-device JPEG encoding (jpeg_ops / include/gp_jpeg.h) measured on the GPU: gp_jpeg_encode per frame at 1352 x 1014 and 800 x 800
with B = 1 and 32, at 4:2:0 and 4:4:4, quality 90, hipEvent-timed, median of 20 calls after 3 warm-ups, beside gp_png_encode on the
same frames (the three frame kinds of tools/png_probe.py); the files' bytes and the encode time against Pillow's JPEG encoder on this
host's CPU at the same quality.  Writes profiles/jpeg_probe.txt.

    python tools/jpeg_probe.py            (needs a GPU)
"""
import io
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from gaussianprediction_amd import jpeg_ops as JPG, png_ops as PNG  # noqa: E402
from png_probe import DEV, SIZES, frames, timed  # noqa: E402

QUALITY = 90


def pillow_jpeg(img, sub):
    from PIL import Image
    a = img.clamp(0, 1).mul(255).add(0.5).clamp(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()
    buf = io.BytesIO()
    t0 = time.perf_counter()
    Image.fromarray(a).save(buf, format="JPEG", quality=QUALITY, subsampling={"420": 2, "444": 0}[sub], optimize=False)
    return len(buf.getvalue()), (time.perf_counter() - t0) * 1e3


def main():
    lines = [f"gp_jpeg_encode on {torch.cuda.get_device_name(DEV)}: quality {QUALITY}, restart interval {JPG.RESTART_MCUS} MCUs; hipEvent-timed, "
             "median of 20 after 3 warm-ups; gp_png_encode on the same frames beside it",
             f"{'H x W':>12s} {'B':>3s} {'frame':>26s} {'420 ms/frame':>13s} {'444 ms/frame':>13s} {'PNG ms/frame':>13s}"]
    for H, W in SIZES:
        fr = frames(H, W)
        for B in (1, 32):
            for name, img in fr.items():
                x = img.to(DEV)[None].expand(B, -1, -1, -1).contiguous()
                ts = []
                for sub in ("420", "444"):
                    out = torch.empty(B, JPG.bound(H, W, sub), dtype=torch.uint8, device=DEV)
                    ts.append(timed(lambda: JPG.encode(x, quality=QUALITY, subsampling=sub, out=out)) / B)
                    del out
                out = torch.empty(B, PNG.bound(H, W), dtype=torch.uint8, device=DEV)
                ts.append(timed(lambda: PNG.encode(x, out=out)) / B)
                del out
                lines.append(f"{H:5d} x {W:4d} {B:3d} {name:>26s} {ts[0]:13.3f} {ts[1]:13.3f} {ts[2]:13.3f}")
    lines.append("")
    lines.append(f"bytes out against Pillow's JPEG encoder on this host's CPU (quality {QUALITY}, optimize off, no restart markers) and its time per frame")
    lines.append(f"{'H x W':>12s} {'frame':>26s} {'sub':>4s} {'gp_jpeg':>10s} {'Pillow':>10s} {'ratio':>6s} {'Pillow ms':>10s} {'gp_png':>10s}")
    for H, W in SIZES:
        for name, img in frames(H, W).items():
            png = len(PNG.encode_to_bytes(img.to(DEV))[0])
            for sub in ("420", "444"):
                ours = len(JPG.encode_to_bytes(img.to(DEV), quality=QUALITY, subsampling=sub)[0])
                p, t = pillow_jpeg(img, sub)
                lines.append(f"{H:5d} x {W:4d} {name:>26s} {sub:>4s} {ours:10d} {p:10d} {ours / p:6.3f} {t:10.1f} {png:10d}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "jpeg_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
