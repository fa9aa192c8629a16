"""Shared by tests/test_jpeg_decode_host.py (the decoder's workgroup programs emulated on the CPU) and tests/test_gpu_jpeg_decode.py (the
kernels): the JPEG files -- the smallest at which each mechanism of include/gp_jpeg_decode.h can go wrong -- written by Pillow and, through
a writer the caller passes (tests/jpeg_emulate.cpp on the CPU, jpeg_ops on the device), by this project's own encoder; the malformed
files derived from good ones; and the files the host refuses."""
import io
import struct
import subprocess
from types import SimpleNamespace

import numpy as np

import emulate_build
import jpeg_cases as J
import jpeg_ref as R

# GP_JPEG_DECODE_* of include/gp_jpeg_decode.h (tests/test_jpeg_decode_host.py compares them with the header)
OK, TRUNCATED, NO_CODE, CATEGORY, RUN, TRAILING, MARKER, HUFFMAN_TABLE, TABLE, BUDGET = range(10)


def noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (3, H, W), dtype=np.uint8)


def saturated(H, W, seed):
    """uint8 [3, H, W]: every sample 0 or 255 at random -- the transform overshoots on both sides and the clamps work."""
    return (np.random.default_rng(seed).integers(0, 2, (3, H, W)) * 255).astype(np.uint8)


def pillow_file(img, **kw):
    """The JPEG file Pillow writes of img [3, H, W] uint8 (save's keywords: quality, qtables, subsampling, restart_marker_blocks,
    optimize, comment, exif, icc_profile ...)."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0))).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def pillow_pixels(data):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)))


# (name, image, quality) of the shapes and contents; every one is written by the project's encoder at 4:2:0 and 4:4:4 and by Pillow
def inputs():
    out = []
    for H, W in ((1, 1), (8, 8), (16, 16), (17, 33), (45, 67), (24, 24)):
        out.append((f"textured-{H}x{W}", J.textured(H, W, H * 100 + W), 90))
    out.append(("rows-cross-40x88", J.textured(40, 88, 3), 90))          # intervals crossing MCU rows
    out.append(("wrap-144x130", J.textured(144, 130, 4), 90))            # RST 0 .. 7, 0, 1 at 4:2:0
    for H, W in ((5, 3), (9, 4), (7, 5)):                                # ceil(W / 2) <= 2: replicated chroma; 3: the first filtered width
        out.append((f"narrow-{H}x{W}", noise(H, W, 10 * H + W), 90))
    out.append(("noise-q100-48x48", J.noise_with_extremes(48, 48, 6), 100))      # 0xFF stuffing, the largest categories, coefficient 63
    out.append(("noise-checkerboard-q100", J.checkerboard(6), 100))       # DC differences of +-2040: category 11
    out.append(("noise-q1-33x31", noise(33, 31, 7), 1))                   # q = 255 everywhere
    for v in (0, 128, 255):
        out.append((f"constant-{v}", np.full((3, 20, 28), v, dtype=np.uint8), 90))
    out.append(("saturated-40x40", saturated(40, 40, 8), 95))
    return out


def pillow_variants(name):
    """(subsampling, restart_marker_blocks) pairs a content is written with by Pillow."""
    big = name.startswith(("rows-", "wrap-"))
    return ((2, 8), (0, 1), (2, 0)) if big else ((2, 0), (2, 1), (2, 8), (0, 0), (0, 1), (0, 8))


def wellformed(own):
    """own(img, "420" / "444", quality, key) -> the file this project's encoder writes.  Returns [Case(name, file)]."""
    out = []
    for name, img, q in inputs():
        for sub in ("420", "444"):
            out.append(SimpleNamespace(name=f"own-{name}-{sub}", file=own(img, sub, q, f"{name}-{sub}")))
        for sub, rmb in pillow_variants(name):
            out.append(SimpleNamespace(name=f"pillow-{name}-{'444' if sub == 0 else '420'}-r{rmb}",
                                       file=pillow_file(img, quality=q, subsampling=sub, restart_marker_blocks=rmb)))
    img = J.textured(184, 200, 9)                                         # 575 MCUs at 4:4:4: 72 intervals of 8 -- more than one wave of lanes -- and 575 of 1
    out.append(SimpleNamespace(name="own-lanes-184x200-444", file=own(img, "444", 90, "lanes-444")))
    out.append(SimpleNamespace(name="pillow-lanes-184x200-444-r1", file=pillow_file(img, quality=90, subsampling=0, restart_marker_blocks=1)))
    zimg, table = J.bright_pixels(3)                                       # two ZRL before a block's one AC coefficient
    out.append(SimpleNamespace(name="own-zrl-48x48-420", file=own(zimg, "420", (table, table), "zrl-420")))
    zz = [table[J.ZIGZAG[k]] for k in range(64)]
    for order, t in (("a", table), ("b", zz)):                            # (whichever order this Pillow reads qtables in, one of them is the table above)
        out.append(SimpleNamespace(name=f"pillow-zrl-48x48-444-{order}", file=pillow_file(zimg, qtables=[t, t], subsampling=0, restart_marker_blocks=8)))
    img = J.textured(45, 67, 11)
    for sub in (2, 0):                                                    # the file's own Huffman tables, codes of 16 bits among them on noise
        out.append(SimpleNamespace(name=f"pillow-optimize-45x67-{sub}", file=pillow_file(img, quality=90, subsampling=sub, optimize=True, restart_marker_blocks=8)))
    out.append(SimpleNamespace(name="pillow-optimize-random-48x48", file=pillow_file(noise(48, 48, 12), quality=100, subsampling=0, optimize=True)))
    out.append(SimpleNamespace(name="pillow-com-appn-45x67", file=pillow_file(img, quality=90, subsampling=2, comment=b"a comment", exif=b"Exif\0\0II*\0\x08\0\0\0\0\0\0\0\0\0",
                                                                             icc_profile=bytes(range(200)), restart_marker_blocks=8)))
    return out


# ---- surgery on a good file ----
def split(data):
    """(head: SOI .. SOS, [the intervals' bytes], tail: EOI) of a file jpeg_ref.walk takes; the RST markers are dropped."""
    pos = 2
    while True:
        m = data[pos + 1]
        n = struct.unpack(">H", data[pos + 2:pos + 4])[0]
        pos += 2 + n
        if m == 0xda:
            break
    parts, cur, i = [], pos, pos
    while True:
        i = data.index(b"\xff", i)
        if data[i + 1] == 0:
            i += 2
        elif 0xd0 <= data[i + 1] <= 0xd7:
            parts.append(data[cur:i])
            cur = i = i + 2
        else:
            parts.append(data[cur:i])
            return data[:pos], parts, data[i:]


def join(head, parts, tail=b"\xff\xd9", numbers=None):
    out = bytearray(head)
    for k, part in enumerate(parts):
        out += part
        if k + 1 < len(parts):
            out += bytes([0xff, 0xd0 + (k if numbers is None else numbers[k]) % 8])
    return bytes(out) + tail


def segment_at(data, marker):
    """(offset of the 0xFF, length with the marker) of the first segment `marker` before the scan."""
    pos = 2
    while True:
        m = data[pos + 1]
        n = struct.unpack(">H", data[pos + 2:pos + 4])[0]
        if m == marker:
            return pos, 2 + n
        assert m != 0xda, hex(marker)
        pos += 2 + n


class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, value, n):
        self.bits += [(value >> (n - 1 - i)) & 1 for i in range(n)]

    def bytes(self):
        bits = self.bits + [1] * (-len(self.bits) % 8)
        out = bytearray()
        for i in range(0, len(bits), 8):
            b = int("".join(map(str, bits[i:i + 8])), 2)
            out.append(b)
            if b == 0xff:
                out.append(0)
        return bytes(out)


def run_past_63(good8):
    """good8: an 8 x 8 4:4:4 file with the Annex K tables.  Its one MCU is replaced: DC category 0, then (run 15, category 1) four times
    -- the fourth takes the index from 49 to 64."""
    codes = {sym: lc for lc, sym in R.walk(good8)["dht_tables"][0x10].items()}
    dc = {sym: lc for lc, sym in R.walk(good8)["dht_tables"][0x00].items()}
    w = BitWriter()
    w.put(dc[0][1], dc[0][0])
    for _ in range(4):
        w.put(codes[0xf1][1], codes[0xf1][0])
        w.put(1, 1)
    for _ in range(6):
        w.put(0xffff, 16)                                                  # (enough bits behind it: the status is the run's, not the data's end)
    head, _, tail = split(good8)
    return join(head, [w.bytes()], tail)


def malformed(own):
    """[Case(name, file, status, goods)], each derived from a good 40 x 88 4:4:4 file of noise (55 MCUs, seven intervals) or, the run past
    63, from an 8 x 8 one; goods: two good files of the case's shape, to stand on both sides of it in a batch of three."""
    base = own(noise(40, 88, 21), "444", 90, "bad-base")
    goods = [own(noise(40, 88, s), "444", 90, f"good-{s}") for s in (22, 23)]
    head, parts, tail = split(base)
    assert len(parts) == 7 and all(len(p) > 120 for p in parts)
    out = []

    def case(name, file, status, goods=goods):
        out.append(SimpleNamespace(name=name, file=file, status=status, goods=goods))

    def with_part(k, part):
        return join(head, parts[:k] + [part] + parts[k + 1:], tail)

    case("interval-cut-short", with_part(2, parts[2][:-9]), TRUNCATED)
    k = next(i for i in range(40, len(parts[1]) - 17) if 0xff not in parts[1][i - 1:i + 17])
    ones = parts[1][:k] + b"\xff\x00" * 8 + parts[1][k + 16:]                # 64 one-bits: wherever a code starts in them, none matches
    case("no-code-matches", with_part(1, ones), NO_CODE)
    small = [own(J.textured(8, 8, s), "444", 90, f"good-small-{s}") for s in (808, 809)]
    case("run-past-63", run_past_63(small[0]), RUN, small)
    case("extra-byte-before-rst", with_part(3, parts[3] + b"\x55"), TRAILING)
    mid = bytearray(parts[4])
    k = next(i for i in range(40, len(mid)) if 0xff not in mid[i - 1:i + 3])
    mid[k:k + 2] = b"\xff\x01"
    case("ff-01-inside", with_part(4, bytes(mid)), MARKER)
    at, n = segment_at(base, 0xc4)
    assert base[at + 4] == 0x00 and n == 2 + 2 + 1 + 16 + 12                   # DC 0 of Annex K: bits 0 1 5 1 1 1 1 1 1 0 ...
    bits = bytearray(base[at + 5:at + 21])
    bits[0], bits[2] = 2, bits[2] - 2                                      # two codes of length 1 and one of length 2: oversubscribed; as many symbols
    case("oversubscribed-dht", base[:at + 5] + bytes(bits) + base[at + 21:], HUFFMAN_TABLE)
    return out


def rst_out_of_order(own):
    head, parts, tail = split(own(noise(40, 88, 21), "444", 90, "bad-base"))
    return join(head, parts, tail, numbers=[0, 1, 3, 2, 4, 5])


def refused(own):
    """[(name, file, the reason's words)]: what jpeg_decode.parse refuses on the host."""
    img = J.textured(17, 33, 5)
    base = pillow_file(img, quality=90, subsampling=2)
    own_file = own(img, "420", 90, "refused-base")
    out = [("progressive", pillow_file(img, progressive=True), "progressive (SOF2)")]
    at, _ = segment_at(base, 0xc0)
    out.append(("extended", base[:at + 1] + b"\xc1" + base[at + 2:], "extended sequential (SOF1)"))
    out.append(("arithmetic", base[:at + 1] + b"\xc9" + base[at + 2:], "arithmetic coding"))
    out.append(("twelve-bit", base[:at + 4] + b"\x0c" + base[at + 5:], "12-bit samples"))
    q, _ = segment_at(base, 0xdb)
    out.append(("dqt-16-bit", base[:q + 4] + bytes([0x10 | base[q + 4]]) + base[q + 5:], "16-bit quantisation table"))
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img[0]).save(buf, format="JPEG")
    out.append(("one-component", buf.getvalue(), "one component"))
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(np.concatenate([img, img[:1]]).transpose(1, 2, 0)), "CMYK").save(buf, format="JPEG")
    out.append(("four-components", buf.getvalue(), "four components"))
    out.append(("422", pillow_file(img, subsampling=1), "sampling factors 2x1 1x1 1x1"))
    for name, hv in (("440", 0x12), ("411", 0x41)):
        out.append((name, base[:at + 11] + bytes([hv]) + base[at + 12:], f"sampling factors {hv >> 4}x{hv & 15} 1x1 1x1"))
    s, _ = segment_at(own_file, 0xda)
    out.append(("two-scans", own_file[:-2] + own_file[s:], "more than one scan"))
    out.append(("scan-of-one", own_file[:s + 4] + b"\x01" + own_file[s + 5:], "more than one scan"))
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00"
    out.append(("adobe-rgb", own_file[:2] + adobe + b"\x00" + own_file[2:], "Adobe APP14 with colour transform 0"))
    out.append(("adobe-ycck", own_file[:2] + adobe + b"\x02" + own_file[2:], "Adobe APP14 with colour transform 2"))
    out.append(("dnl", own_file[:-2] + b"\xff\xdc\x00\x04\x00\x11\xff\xd9", "DNL"))
    out.append(("rst-out-of-order", rst_out_of_order(own), "RST markers do not count"))
    out.append(("no-eoi", own_file[:-2], "no EOI"))
    out.append(("not-a-jpeg", b"\x89PNG" + own_file[4:], "no SOI"))
    return out


def run_job(exe, d, group, pl, host, dtype, guard, mangle=None, most=None):
    """One process of tests/jpeg_decode_emulate.cpp or tests/jpeg_sync_emulate.cpp (they read the same job file) over one shape group of
    JD.groups(items), pl being its plan of JD.plans and host the array decode_stage.fill wrote -> the bytes it wrote."""
    import decode_stage_cases as SC
    (H, W, sub), idx = group
    seg, image_seg, tables, payload = SC.sections(host, pl)
    seg = seg if mangle is None else np.array(mangle([tuple(r) for r in pl.seg.tolist()]), dtype=np.int64).tobytes()
    job, out = str(d / "job.bin"), str(d / "out.bin")
    with open(job, "wb") as fp:
        fp.write(struct.pack("<8iq", len(idx), H, W, sub, 0 if dtype == np.uint8 else 1, len(seg) // 40, pl.most if most is None else most, guard, pl.bytes))
        fp.write(seg + image_seg + tables + payload)
    subprocess.check_call([exe, job, out], timeout=300)          # (a loop that does not end is a failure here, not a hang)
    return open(out, "rb").read()


def staged_groups(items):
    """[(group, plan)] of JD.groups(items) and the array all of them are staged in, as the device path stages them."""
    import decode_stage_cases as SC
    from gaussianprediction_amd import jpeg_decode as JD
    shapes = JD.groups(items)
    plans = JD.plans(items, shapes)
    return list(zip(shapes, plans)), SC.filled(plans)


def build_emulator(d, sanitize):
    """tests/jpeg_decode_emulate.cpp built into directory `d`; returns run(items, dtype, guard, mangle, most) -> (images [3, H, W] numpy,
    status), one process per shape group."""
    exe = emulate_build.build("jpeg_decode_emulate", d, sanitize)

    def run(items, dtype=np.uint8, guard=8, mangle=None, most=None):
        images, status = [None] * len(items), [0] * len(items)
        staged, host = staged_groups(items)
        for group, pl in staged:
            (H, W, _), idx = group
            raw = run_job(exe, d, group, pl, host, dtype, guard, mangle, most)
            B, n = len(idx), 3 * H * W
            words = np.frombuffer(raw[:4 * B], dtype=np.uint32)
            slots = np.frombuffer(raw[4 * B:], dtype=dtype).reshape(B, n + guard)
            assert (slots[:, n:].view(np.uint8) == 0xA5).all()          # the guard behind every slot
            for b, i in enumerate(idx):
                status[i] = int(words[b])
                images[i] = slots[b, :n].reshape(3, H, W)
        return images, status

    return run


def eval_directory(root, H, W, dev):
    """What metrics.evaluate_dirs reads, for the device tests: two methods of four .png renders and .jpg ground truths each, one with this
    project's JPEG files (written on `dev`) and one with Pillow's."""
    import torch
    from PIL import Image
    from gaussianprediction_amd import jpeg_ops, png_ops
    for method, own in (("ours", True), ("theirs", False)):
        for sub in ("renders", "gt"):
            (root / method / sub).mkdir(parents=True)
        for i in range(4):
            render, gt = J.textured(H, W, 10 * i + own), J.textured(H, W, 10 * i + 5)
            (root / method / "renders" / f"{i:05d}.png").write_bytes(png_ops.encode_to_bytes(torch.from_numpy(render).to(dev))[0])
            if own:
                (root / method / "gt" / f"{i:05d}.jpg").write_bytes(jpeg_ops.encode_to_bytes(torch.from_numpy(gt).to(dev), subsampling="420" if i % 2 else "444")[0])
            else:
                Image.fromarray(gt.transpose(1, 2, 0)).save(root / method / "gt" / f"{i:05d}.jpg", quality=92, subsampling=2 if i % 2 else 0)
