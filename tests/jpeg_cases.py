"""Shared by tests/test_jpeg_host.py (the encoder's workgroup programs emulated on the CPU) and tests/test_gpu_jpeg.py (the kernels): the
images -- the smallest shapes at which each mechanism of include/gp_jpeg.h can go wrong -- and their quantisation tables."""
import subprocess

import numpy as np

import emulate_build
import png_cases as P

ONES = [1] * 64


def textured(H, W, seed):
    """uint8 [3, H, W]: smooth structure plus noise, different in every channel."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 90 * np.sin(xx / 5.0 + c) * np.cos(yy / 7.0 - c) for c in range(3)])
    return np.clip(base + rng.normal(0, 12, (3, H, W)), 0, 255).astype(np.uint8)


def blobs(H, W, seed):
    """uint8 [3, H, W]: a dozen dim coloured Gaussian blobs on black -- smooth and dark, as a rendered frame is."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.zeros((3, H, W))
    for _ in range(12):
        cy, cx, s = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(4, 15)
        col = rng.uniform(0, 0.5, 3)
        img += col[:, None, None] * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))[None]
    return np.clip(img * 255 + 0.5, 0, 255).astype(np.uint8)


def checkerboard(n):
    """uint8 [3, 8n, 8n]: 8 x 8 blocks of 0 and 255 in turn -- with an all-ones table the DC differences are +-2040, category 11."""
    by, bx = np.mgrid[0:8 * n, 0:8 * n] // 8
    g = (((by + bx) % 2) * 255).astype(np.uint8)
    return np.stack([g, g, g])


def noise_with_extremes(H, W, seed):
    """uint8 [3, H, W]: uniform noise; the first 16 x 16 pixels are grey stripes of 0 / 255 that follow the sign of the DCT's basis
    function 4 (|F(0, 4)| = 1020, AC category 10), and a noise block nearly always ends in a non-zero coefficient 63."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    sign = np.cos((2 * np.arange(16) % 16 + 1) * 4 * np.pi / 16) > 0
    img[:, :16, :16] = np.where(sign[None, None, :], 255, 0)
    return img


def bright_pixels(n):
    """(uint8 [3, 16n, 16n], table): black with one white pixel per 16 x 16, and a table of 255 everywhere except 1 at DC and at
    zigzag position 40 -- every block with the pixel codes DC, then 39 zeros (two ZRL) before its one other coefficient."""
    img = np.zeros((3, 16 * n, 16 * n), dtype=np.uint8)
    img[:, 15::16, 15::16] = 255
    table = [255] * 64
    table[0] = 1
    table[ZIGZAG[40]] = 1
    return img, table


ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def cases():
    """[(name, image [3, H, W] float32 or uint8, (luminance, chrominance) tables in natural order or None for quality 90)]."""
    out = []
    for H, W in ((1, 1), (8, 8), (16, 16), (17, 33), (45, 67)):          # one MCU exactly; partial MCUs on both axes
        out.append((f"textured-{H}x{W}", textured(H, W, H * 100 + W), None))
    out.append(("rows-cross-40x88", textured(40, 88, 3), None))           # 6 (4:2:0) and 11 (4:4:4) MCUs per row: intervals cross MCU rows
    out.append(("wrap-144x130", textured(144, 130, 4), None))             # 81 MCUs at 4:2:0: 11 intervals (RST 0 .. 7, 0, 1), the last of one MCU
    out.append(("last-single-24x24", textured(24, 24, 5), None))          # 9 MCUs at 4:4:4: the last interval holds one
    out.append(("checkerboard-ones", checkerboard(6), (ONES, ONES)))
    out.append(("noise-ones", noise_with_extremes(48, 48, 6), (ONES, ONES)))
    img, table = bright_pixels(3)
    out.append(("bright-pixels-zrl", img, (table, table)))
    for v in (0, 128, 255):
        out.append((f"constant-{v}", np.full((3, 20, 28), v, dtype=np.uint8), None))
    out.append(("disc-100x90", P.disc(100, 90, 3), None))
    out.append(("ramp-64x100", P.ramp(64, 100), None))
    out.append(("edge-floats-37x45", P.edge_floats((3, 37, 45), 1), None))
    for seed in (0, 1):                                                   # whole MCUs: what the two chroma filters alone differ by
        out.append((f"blobs-80x96-{seed}", blobs(80, 96, seed), None))
    return out


def build_emulator(d):
    """tests/jpeg_emulate.cpp built with the host compiler into directory `d`; returns run(img [3, H, W], "420" / "444", (luminance,
    chrominance) tables, key=None) -> the file's bytes (kept per key)."""
    exe = emulate_build.build("jpeg_emulate", d)
    done = {}

    def run(img, sub, qtables, key=None):
        if key is not None and key in done:
            return done[key]
        src, qt, out = str(d / "in.raw"), str(d / "qt.bin"), str(d / "out.jpg")
        np.ascontiguousarray(img).tofile(src)
        np.array(list(qtables[0]) + list(qtables[1]), dtype=np.uint8).tofile(qt)
        _, H, W = img.shape
        subprocess.check_call([exe, str(H), str(W), "1" if img.dtype == np.uint8 else "0", {"420": "0", "444": "1"}[sub], qt, src, out],
                              timeout=60)          # (a phase that does not end is a failure here, not a hang)
        data = open(out, "rb").read()
        if key is not None:
            done[key] = data
        return data

    run.exe, run.dir = exe, d
    return run
