"""Shared by tests/test_png_host.py (the encoder's workgroup programs emulated on the CPU) and tests/test_gpu_png.py (the kernels): the
images, the 8-bit quantisation in numpy, the chunk walk with zlib's and Pillow's decoders as the oracle, and the like-for-like size
reference (zlib's own run-length strategy over the same filtered bytes, cut at the same bands)."""
import io
import struct
import subprocess
import zlib

import numpy as np

import emulate_build

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def quantise(x):
    """uint8 [.., H, W] of a float32 array as gp_png.h states it: floor(x * 255 + 0.5) in float32, clamped; NaN -> 0."""
    if x.dtype == np.uint8:
        return x
    assert x.dtype == np.float32
    with np.errstate(invalid="ignore"):
        s = np.floor(x * np.float32(255.0) + np.float32(0.5))
    s = np.where(np.isnan(s), np.float32(0.0), s)
    return np.clip(s, 0.0, 255.0).astype(np.uint8)


def edge_floats(shape, seed):
    """float32 values around the quantisation steps: below 0, above 1, k/255 and its two float32 neighbours, one NaN."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    k = rng.integers(0, 256, n).astype(np.float32) / np.float32(255.0)
    half = (rng.integers(0, 255, n).astype(np.float32) + np.float32(0.5)) / np.float32(255.0)       # the rounding boundary itself
    pick = rng.integers(0, 8, n)
    x = np.select([pick == 0, pick == 1, pick == 2, pick == 3, pick == 4, pick == 5, pick == 6],
                  [k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)), half, np.nextafter(half, np.float32(-1)),
                   rng.uniform(-3, 0, n).astype(np.float32), rng.uniform(1, 4, n).astype(np.float32)],
                  rng.uniform(0, 1, n).astype(np.float32)).astype(np.float32)
    x[n // 2] = np.nan
    x[0], x[-1] = np.float32(-0.0), np.float32(np.inf)
    return x.reshape(shape)


def disc(H, W, seed):
    """White background, a noisy disc: float32 [3, H, W]."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    inside = (yy - H / 2) ** 2 + (xx - W / 2) ** 2 < (0.3 * min(H, W)) ** 2
    body = 0.5 + 0.2 * np.sin(xx / 9.0)[None] * np.cos(yy / 7.0)[None] + rng.normal(0, 0.02, (3, H, W))
    return np.where(inside[None], body, 1.0).astype(np.float32)


def ramp(H, W):
    """uint8 [3, H, W] holding all 256 values: a diagonal ramp, another slope in every channel."""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([(xx + yy) % 256, (2 * xx + yy) % 256, (xx + 3 * yy) % 256]).astype(np.uint8)


def runs(W):
    """uint8 [3, H, W] for filter type 0: rows of runs of 2, 3, 4, 257, 258, 259, 260 and 517 equal bytes between single different bytes."""
    lengths = [2, 3, 4, 257, 258, 259, 260, 517]
    stream, v = [], 1
    for rep in range(3):
        for n in lengths[rep:] + lengths[:rep]:
            stream += [v] * n + [(v + 100) % 256]
            v = v % 250 + 1
    row = 3 * W
    H = -(-len(stream) // row)
    stream += [0] * (H * row - len(stream))
    return np.array(stream, dtype=np.uint8).reshape(H, W, 3).transpose(2, 0, 1).copy()


def run_across_cut(band, bounds=False):
    """uint8 [3, H, W] for filter type 0 whose filtered stream holds one run of equal bytes laid across the first band cut (inside one
    row, so no filter byte interrupts it); bounds=True: (the image, the run's first position, the position after it)."""
    W = 400
    row = 1 + 3 * W
    H = -(-(band + 2000) // row)
    rng = np.random.default_rng(5)
    flat = rng.integers(0, 256, H * row, dtype=np.uint8)
    flat[flat == 77] = 78
    row_start = band - band % row
    lo, hi = max(band - 300, row_start + 1), min(band + 400, row_start + row)
    assert lo + 3 <= band <= hi - 3
    flat[lo:hi] = 77
    img = flat.reshape(H, row)[:, 1:].reshape(H, W, 3).transpose(2, 0, 1).copy()
    return (img, lo, hi) if bounds else img


def fibonacci(band):
    """(uint8 [3, H, W] for filter type 0, k): the first band holds k symbols with counts F(1) .. F(k), no two neighbours equal (an
    unlimited Huffman code for it is k - 1 levels deep)."""
    W = 85                                   # rows of 256 bytes: the filter byte 0 plus 255 others
    fib = [1, 1]
    while sum(fib) + fib[-1] + fib[-2] <= band - band // 256:
        fib.append(fib[-1] + fib[-2])
    k = len(fib)
    # symbol 0 is the filter byte's value, so the counted symbols are 1 .. k; the most frequent first, dealt round the slots in steps
    # of two (the largest count is under half the total, so no two neighbours are equal)
    total = sum(fib)
    slots = np.zeros(total, dtype=np.uint8)
    order = list(range(0, total, 2)) + list(range(1, total, 2))
    pos = 0
    for s in sorted(range(k), key=lambda i: -fib[i]):
        for _ in range(fib[s]):
            slots[order[pos]] = s + 1
            pos += 1
    assert not (slots[1:] == slots[:-1]).any()
    H = -(-total // 255)
    body = np.concatenate([slots, np.tile(np.array([k + 1, k + 2], dtype=np.uint8), (H * 255 - total + 1) // 2)[:H * 255 - total]])
    return body.reshape(H, W, 3).transpose(2, 0, 1).copy(), k


def one_band_plus_one(band):
    """(H, W) whose filtered stream is exactly one band and one byte long."""
    for W in range(1, 4000):
        if (band + 1) % (1 + 3 * W) == 0 and (band + 1) // (1 + 3 * W) > 1:
            return (band + 1) // (1 + 3 * W), W
    raise AssertionError("no shape")


ZERO_CRC = bytes([0x9d, 0x0a, 0xd9, 0x6d])          # a four-byte message whose CRC-32 is 0


def zero_crc_slice():
    """uint8 [3, 3, 85] for filter type 0: 768 random stream bytes, so one stored band and a first chunk of 4 + 2 + 5 + 768 + 9 = 788
    bytes under its CRC, four per lane of the chunk kernel; stream bytes 9 .. 12 -- lane 5's slice -- are ZERO_CRC, so that lane's
    slice CRC is 0: the value zlib's own polynomial multiplication does not terminate on as its first operand."""
    assert zlib.crc32(ZERO_CRC) == 0
    img = np.random.default_rng(17).integers(0, 256, (3, 85, 3), dtype=np.uint8)
    img.reshape(3, 255)[0, 8:12] = np.frombuffer(ZERO_CRC, dtype=np.uint8)
    return img.transpose(2, 0, 1).copy()


def cases(band):
    """[(name, images [B, 3, H, W] float32 or uint8, filter_none)]."""
    rng = np.random.default_rng(11)
    out = []
    for H, W in ((1, 1), (1, 7), (7, 1), (37, 45)):
        out.append((f"edge-floats-{H}x{W}", edge_floats((1, 3, H, W), H * 100 + W), False))
    out.append(("batch-163x178", np.stack([disc(163, 178, 1), edge_floats((3, 163, 178), 2)]), False))
    H1, W1 = one_band_plus_one(band)
    out.append((f"one-band-plus-one-{H1}x{W1}", rng.integers(0, 256, (1, 3, H1, W1), dtype=np.uint8), False))
    out.append(("constant-300x400", np.full((1, 3, 300, 400), 0.25, dtype=np.float32), False))
    out.append(("disc-300x400", disc(300, 400, 3)[None], False))
    out.append(("random-300x400", rng.integers(0, 256, (1, 3, 300, 400), dtype=np.uint8), False))
    out.append(("ramp-300x400", ramp(300, 400)[None], False))
    out.append(("ramp-none-300x400", ramp(300, 400)[None], True))
    out.append(("runs", runs(211)[None], True))
    out.append(("run-across-cut", run_across_cut(band)[None], True))
    out.append(("fibonacci", fibonacci(band)[0][None], True))
    out.append(("zero-crc-slice", zero_crc_slice()[None], True))
    return out


def unfilter(stream, H, W):
    """uint8 [H, W, 3] from the filtered stream (the test's own restatement of the five filters)."""
    row = 3 * W
    rows = np.frombuffer(stream, dtype=np.uint8).reshape(H, row + 1)
    img = np.zeros((H, row), dtype=np.int32)
    for y in range(H):
        f, line = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        up = img[y - 1] if y else np.zeros(row, dtype=np.int32)
        if f == 0:
            img[y] = line
        elif f == 2:
            img[y] = (line + up) & 255
        else:
            cur = img[y]
            for j in range(row):
                a = cur[j - 3] if j >= 3 else 0
                b = up[j]
                c = up[j - 3] if j >= 3 else 0
                if f == 1:
                    pred = a
                elif f == 3:
                    pred = (a + b) >> 1
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[j] = (line[j] + pred) & 255
    return img.astype(np.uint8).reshape(H, W, 3)


def check_file(data, want, filter_none=False, pillow=True):
    """Walk the chunks of `data` (bytes) and decode it; `want`: uint8 [3, H, W].  Returns (the filtered stream, the IDAT payload's
    length, the number of IDAT chunks)."""
    _, H, W = want.shape
    assert data[:8] == SIGNATURE
    pos, chunks = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert len(body) == n, (kind, n)
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + body), (kind, len(chunks))
        chunks.append((kind, body))
        pos += 12 + n
    assert pos == len(data)
    kinds = [k for k, _ in chunks]
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and chunks[-1][1] == b"" and set(kinds[1:-1]) == {b"IDAT"}, kinds
    assert chunks[0][1] == struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)
    payload = b"".join(body for k, body in chunks if k == b"IDAT")
    stream = zlib.decompress(payload)                 # (checks the Adler-32)
    assert len(stream) == H * (3 * W + 1)
    types = np.frombuffer(stream, dtype=np.uint8).reshape(H, 3 * W + 1)[:, 0]
    assert types.max() <= 4 and (not filter_none or types.max() == 0)
    hwc = want.transpose(1, 2, 0)
    if pillow:
        from PIL import Image
        got = np.array(Image.open(io.BytesIO(data)))
        assert got.shape == (H, W, 3) and np.array_equal(got, hwc)
    else:
        assert np.array_equal(unfilter(stream, H, W), hwc)
    return stream, len(payload), len(kinds) - 2


def best_filters(want):
    """The filter type of every row under the header's rule, from the 8-bit image [3, H, W] (numpy, vectorised per row)."""
    _, H, W = want.shape
    img = want.transpose(1, 2, 0).reshape(H, 3 * W).astype(np.int32)
    types = []
    for y in range(H):
        cur = img[y]
        up = img[y - 1] if y else np.zeros_like(cur)
        a = np.concatenate([np.zeros(3, dtype=np.int32), cur[:-3]])
        c = np.concatenate([np.zeros(3, dtype=np.int32), up[:-3]])
        pa, pb, pc = np.abs(up - c), np.abs(a - c), np.abs(a + up - 2 * c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
        sums = []
        for pred in (0, a, up, (a + up) >> 1, paeth):
            r = (cur - pred) & 255
            sums.append(int(np.where(r < 128, r, 256 - r).sum()))
        types.append(int(np.argmin(sums)))           # (argmin: the first of equal sums)
    return np.array(types, dtype=np.uint8)


def rle_reference_bytes(stream, band):
    """The like-for-like size: the same filtered bytes cut at `band`, every piece deflated by zlib's run-length strategy and ended
    with a sync flush."""
    total = 0
    for k in range(0, len(stream), band):
        c = zlib.compressobj(1, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
        total += len(c.compress(stream[k:k + band]) + c.flush(zlib.Z_SYNC_FLUSH))
    return total


def build_emulator(d):
    """tests/png_emulate.cpp built into directory `d`; returns run(img [3, H, W], filter_none) -> the file's bytes."""
    exe = emulate_build.build("png_emulate", d)

    def run(img, filter_none):
        src, out = str(d / "in.raw"), str(d / "out.png")
        np.ascontiguousarray(img).tofile(src)
        _, H, W = img.shape
        subprocess.check_call([exe, str(H), str(W), "1" if img.dtype == np.uint8 else "0", "1" if filter_none else "0", src, out],
                              timeout=60)          # (a phase that does not end is a failure here, not a hang)
        return open(out, "rb").read()

    return run
