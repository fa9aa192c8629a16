"""Shared by tests/test_jpeg_sync_host.py (csrc/jpeg_sync_core.h emulated on the CPU) and tests/test_gpu_jpeg_sync.py (the kernels): files
without restart markers, written by Pillow -- the smallest at which each mechanism of include/gp_jpeg_sync.h can go wrong.  Every
property a case is there for is asserted here from tests/jpeg_sync_ref.py, so that a change of S or C cannot silently empty a case."""
import functools
from types import SimpleNamespace

import numpy as np

import emulate_build
import jpeg_cases as J
import jpeg_decode_cases as D
import jpeg_sync_ref as SR
import png_cases as P

OK, SERIAL = 0, 1                      # GP_JPEG_SYNC_* of include/gp_jpeg_sync.h (tests/test_jpeg_sync_host.py compares them with the header)

# (seed, quality) of J.textured(24, 40, seed) at 4:4:4 whose scan is k S - 1, k S and k S + 1 bytes long at S = 128: found by a search
# over seed 0 .. 39 and quality 50 .. 95
CUT_LENGTHS = {-1: (2, 94), 0: (0, 59), 1: (1, 82)}
NOISE_SIDE = 120                       # the smallest multiple of 8 at which saturated noise, q100, 4:4:4 exceeds 2 C S = 65536 bytes of scan


def white(H, W):
    return np.full((3, H, W), 255, dtype=np.uint8)


def natural(H, W, seed):
    """uint8 [3, H, W]: a smooth field plus noise of sigma 4."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 80 * np.sin(xx / 40.0 + c) * np.cos(yy / 55.0 - c) for c in range(3)])
    return np.clip(base + rng.normal(0, 4, (3, H, W)), 0, 255).astype(np.uint8)


def disc8(H, W, seed):
    return np.clip(P.disc(H, W, seed) * 255 + 0.5, 0, 255).astype(np.uint8)


def _case(name, img, **kw):
    return SimpleNamespace(name=name, file=D.pillow_file(img, **kw))


@functools.lru_cache(maxsize=None)
def wellformed(S, C):
    """[Case(name, file, ref = jpeg_sync_ref.analyse(file, S, C))]; items 1 - 10 of the list the tests go through (12: batch())."""
    out = []
    for H, W in ((1, 1), (8, 8)):                                          # 1. shorter than one subsequence
        for sub in (2, 0):
            out.append(_case(f"short-{H}x{W}-{sub}", J.textured(H, W, 7), quality=90, subsampling=sub))
    for d, (seed, q) in CUT_LENGTHS.items():                               # 2. the scan's length at a cut
        out.append(_case(f"length{d:+d}", J.textured(24, 40, seed), quality=q, subsampling=0))
    out.append(_case("rounds-noise-444", D.noise(96, 96, 50), quality=95, subsampling=0))     # 3. one chunk, many rounds
    out.append(_case("rounds-noise-420", D.noise(96, 96, 50), quality=90, subsampling=2))
    out.append(_case("chunks-saturated", D.saturated(NOISE_SIDE, NOISE_SIDE, 40), quality=100, subsampling=0))      # 4. 6. 7.
    out.append(_case("periodic-white-512", white(512, 512), quality=90, subsampling=2))       # 5. never synchronises by itself
    out.append(_case("periodic-white-2048", white(2048, 2048), quality=90, subsampling=2))
    for H, W in ((17, 33), (45, 67)):                                      # 8. partial MCUs
        out.append(_case(f"partial-{H}x{W}", J.textured(H, W, H), quality=90, subsampling=2))
    for H, W in ((5, 3), (9, 4), (7, 5)):                                  #    narrow widths
        for sub in (2, 0):
            out.append(_case(f"narrow-{H}x{W}-{sub}", D.noise(H, W, 10 * H + W), quality=90, subsampling=sub))
    out.append(_case("tables-optimize-noise", D.noise(48, 48, 12), quality=100, subsampling=0, optimize=True))      # 9. the file's own tables
    out.append(_case("tables-optimize-textured-420", J.textured(45, 67, 11), quality=90, subsampling=2, optimize=True))
    mixed = np.concatenate([natural(192, 256, 5), D.noise(64, 256, 3)], axis=1)       # smooth and noisy: symbols rare enough for codes of 16 bits
    out.append(_case("tables-optimize-mixed-444", mixed, quality=95, subsampling=0, optimize=True))
    out.append(_case("tables-q1", D.noise(64, 64, 13), quality=1, subsampling=2))
    out.append(_case("tables-q100", J.textured(64, 64, 14), quality=100, subsampling=0))
    out.append(_case("disc-256", disc8(256, 256, 3), quality=90, subsampling=2))              # 10. the project's own kind of frame
    out.append(_case("disc-256-optimize", disc8(256, 256, 3), quality=90, subsampling=2, optimize=True))
    out.append(_case("natural-320", natural(320, 320, 5), quality=90, subsampling=2))
    for c in out:
        c.ref = SR.analyse(c.file, S, C)
    by = {c.name: c.ref for c in out}
    for c in out:
        if c.name.startswith("short-"):
            assert c.ref.n < S and c.ref.info == (1, 1, 0, 0), c.name
    for d in CUT_LENGTHS:
        assert by[f"length{d:+d}"].n >= 2 * S and by[f"length{d:+d}"].n % S == d % S, (d, by[f"length{d:+d}"].n)
    for name in ("rounds-noise-444", "rounds-noise-420"):
        assert by[name].info[1] == 1 and by[name].info[2] >= 8, (name, by[name].info)
    sat = by["chunks-saturated"]
    assert sat.n > 2 * C * S and sat.info[1] >= 3 and sat.info[3] >= 1, sat.info
    assert sat.cuts_in_ff00 >= 1 and sat.cuts_before_ff >= 1                # 6. stuffing at a cut, both ways
    w = by["periodic-white-512"]
    assert w.info[1] == 1 and w.info[2] == w.info[0] - 1, w.info            # every lane waits for its left neighbour: a heuristic stop fails here
    w = by["periodic-white-2048"]
    assert w.info[1] >= 2 and w.info[2] == min(C, w.info[0]) - 1 and w.info[3] >= 1, w.info
    import jpeg_ref as R
    import jpeg_decode_ref as REF
    assert any(max(l for l, _ in R.walk(REF.strip(c.file))["dht_tables"][0x11]) == 16 for c in out if "-optimize" in c.name)        # a code of 16 bits
    return out


def constructed(S, C):
    """7. and 11.: a subsequence that begins no block, and a running DC that passes 32767.  No encoder writes either from pixels at
    S = 128: a block of 8-bit samples has at most 64 * 128^2 of energy, which keeps its coefficients at categories 7 and 8 on average
    and the block at about 127 bytes with the Annex K tables (measured on blocks picked for their length), and a DC is 8 times a mean.
    So the scan is written here, symbol by symbol, into the head of a Pillow file of 8 x 160 at 4:4:4 and quality 100: per MCU a Y
    block of DC difference +2047 and 63 coefficients of category 10 (206 bytes), then two empty chroma blocks.  Pillow's decoder limits
    such samples in its own way (include/gp_jpeg_decode.h), so the oracle for this file is the one-lane decoder alone."""
    import jpeg_decode_ref as REF
    import jpeg_ref as R
    base = D.pillow_file(J.textured(8, 160, 1), quality=100, subsampling=0)
    tabs = R.walk(REF.strip(base))["dht_tables"]
    dc0, ac0, dc1, ac1 = ({sym: lc for lc, sym in tabs[k].items()} for k in (0x00, 0x10, 0x01, 0x11))
    w = D.BitWriter()
    for _ in range(20):
        w.put(dc0[11][1], dc0[11][0])
        w.put(2047, 11)
        for _ in range(63):
            w.put(ac0[0x0a][1], ac0[0x0a][0])
            w.put(1023, 10)
        for _ in range(2):
            w.put(dc1[0][1], dc1[0][0])
            w.put(ac1[0][1], ac1[0][0])
    head, _, tail = D.split(base)
    c = SimpleNamespace(name="constructed-long-blocks-dc-wrap", file=D.join(head, [w.bytes()], tail))
    c.ref = SR.analyse(c.file, S, C)
    assert S >= 208 or min(c.ref.begun[:-1]) == 0, c.ref.begun             # a subsequence inside one block
    assert 17 * 2047 > 32767 and sum(c.ref.begun) == 60
    return c


def batch():
    """12. three different files of one shape."""
    return [_case(f"batch-{s}", D.noise(45, 67, s), quality=90, subsampling=2) for s in (31, 32, 33)]


def malformed():
    """13. [Case(name, file, status: the GP_JPEG_DECODE_* word the one-lane path gives, goods)], each derived from a good 40 x 88 4:4:4 file
    of noise without restart markers (the run past 63: from an 8 x 8 one)."""
    base = D.pillow_file(D.noise(40, 88, 21), quality=90, subsampling=0)
    goods = [D.pillow_file(D.noise(40, 88, s), quality=90, subsampling=0) for s in (22, 23)]
    head, (scan,), tail = D.split(base)
    assert len(scan) > 1500
    out = []

    def case(name, file, status, goods=goods):
        out.append(SimpleNamespace(name=name, file=file, status=status, goods=goods))

    case("cut-short", head + scan[:-9] + tail, D.TRUNCATED)
    k = next(i for i in range(700, len(scan) - 17) if 0xff not in scan[i - 1:i + 17])
    case("no-code-matches", head + scan[:k] + b"\xff\x00" * 8 + scan[k + 16:] + tail, D.NO_CODE)
    at, n = D.segment_at(base, 0xc4)
    assert base[at + 4] == 0x00 and n == 2 + 2 + 1 + 16 + 12                   # DC 0 of Annex K in a segment of its own
    case("category-above-11", base[:at + 21] + bytes([12] * 12) + base[at + 33:], D.CATEGORY)
    small = [D.pillow_file(J.textured(8, 8, s), quality=90, subsampling=0) for s in (808, 809)]
    case("run-past-63", D.run_past_63(small[0]), D.RUN, small)
    k = next(i for i in range(900, len(scan)) if 0xff not in scan[i - 1:i + 3])
    case("ff-01-inside", head + scan[:k] + b"\xff\x01" + scan[k + 2:] + tail, D.MARKER)
    case("trailing-bytes", head + scan + b"\x55\x55" + tail, D.TRAILING)
    bits = bytearray(base[at + 5:at + 21])
    bits[0], bits[2] = 2, bits[2] - 2
    case("oversubscribed-dht", base[:at + 5] + bytes(bits) + base[at + 21:], D.HUFFMAN_TABLE)
    return out


def build_emulator(d, sanitize):
    """tests/jpeg_sync_emulate.cpp built into directory `d`; returns run(items, dtype, guard) -> (images [3, H, W] numpy, status, info)."""
    exe = emulate_build.build("jpeg_sync_emulate", d, sanitize)

    def run(items, dtype=np.uint8, guard=8):
        images, status, info = [None] * len(items), [0] * len(items), [None] * len(items)
        staged, host = D.staged_groups(items)
        for group, pl in staged:
            (H, W, _), idx = group
            raw = D.run_job(exe, d, group, pl, host, dtype, guard)
            B, n = len(idx), 3 * H * W
            words = np.frombuffer(raw[:4 * B], dtype=np.uint32)
            infos = np.frombuffer(raw[4 * B:20 * B], dtype=np.uint32).reshape(B, 4)
            slots = np.frombuffer(raw[20 * B:], dtype=dtype).reshape(B, n + guard)
            assert (slots[:, n:].view(np.uint8) == 0xA5).all()          # the guard behind every slot
            for b, i in enumerate(idx):
                status[i], info[i], images[i] = int(words[b]), tuple(int(v) for v in infos[b]), slots[b, :n].reshape(3, H, W)
        return images, status, info

    return run
