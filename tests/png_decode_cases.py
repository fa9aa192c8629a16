"""Shared by tests/test_png_decode_host.py (the decoder's workgroup programs emulated on the CPU) and tests/test_gpu_png_decode.py (the
kernels): a PNG writer of its own (per-row filter types, any deflate bytes, IDAT chunks cut where the test says), a bit writer for
stored, fixed-Huffman and dynamic-Huffman blocks, and the case lists.  tests/png_cases.py supplies images and is not edited."""
import io
import struct
import zlib
from types import SimpleNamespace

import numpy as np

import png_cases as P

BAND = 16384
COLOUR = {1: 0, 2: 4, 3: 2, 4: 6}
SERIAL, BANDED = 1, 2

# GP_PNG_DECODE_* of include/gp_png_decode.h
(TRUNCATED, BLOCK_TYPE, STORED_LEN, TOO_MANY_CODES, CLEN_CODE, REPEAT_FIRST, REPEAT_OVERRUN, LIT_OVERSUBSCRIBED, LIT_INCOMPLETE,
 NO_END_OF_BLOCK, LIT_SYMBOL, DIST_SYMBOL, DIST_TOO_FAR, OUTPUT_LONG, OUTPUT_SHORT, ADLER, FILTER, ZLIB_METHOD, ZLIB_FDICT, ZLIB_FCHECK,
 ZLIB_WINDOW, DIST_CODE, NOT_BANDED) = range(1, 24)


# ---- the PNG writer ----
def chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def png_file(H, W, C, pieces, depth=8, colour=None, interlace=0):
    """A PNG file whose IDAT chunks hold `pieces` (a list of bytes), whatever they are."""
    ihdr = struct.pack(">IIBBBBB", W, H, depth, COLOUR[C] if colour is None else colour, 0, 0, interlace)
    return P.SIGNATURE + chunk(b"IHDR", ihdr) + b"".join(chunk(b"IDAT", p) for p in pieces) + chunk(b"IEND", b"")


def cut(payload, at):
    """`payload` cut at the byte positions `at`."""
    at = [0] + list(at) + [len(payload)]
    return [payload[a:b] for a, b in zip(at[:-1], at[1:])]


def filtered(img, types):
    """The filtered stream (bytes) of img uint8 [H, W, C] with filter type types[y] on row y."""
    H, W, C = img.shape
    rows = img.reshape(H, W * C).astype(np.int32)
    out = np.zeros((H, 1 + W * C), dtype=np.uint8)
    for y in range(H):
        cur = rows[y]
        up = rows[y - 1] if y else np.zeros_like(cur)
        a = np.concatenate([np.zeros(C, dtype=np.int32), cur[:-C]])
        c = np.concatenate([np.zeros(C, dtype=np.int32), up[:-C]])
        pa, pb, pc = np.abs(up - c), np.abs(a - c), np.abs(a + up - 2 * c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
        pred = (0, a, up, (a + up) >> 1, paeth)[types[y]]
        out[y, 0] = types[y]
        out[y, 1:] = (cur - pred) & 255
    return out.tobytes()


def cycling(H, first):
    """Filter types that cycle through 0 .. 4, row 0 taking `first`."""
    return [(y + first) % 5 for y in range(H)]


# ---- the bit writer ----
def canonical(lens):
    """{symbol: (code, length)} of the canonical Huffman code with these lengths (RFC 1951 3.2.2)."""
    codes, code = {}, 0
    for l in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == l:
                codes[s] = (code, l)
                code += 1
        code <<= 1
    return codes


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_LENS = [4] * 13 + [5] * 6                 # a complete code over all 19 code-length symbols


class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):                                    # least significant bit first
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, pair):                                           # a Huffman code: most significant bit first
        code, nbits = pair
        for k in range(nbits - 1, -1, -1):
            self.put((code >> k) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)

    def header(self, final, kind):
        self.put(final, 1)
        self.put(kind, 2)

    def stored(self, data, final=0, nlen=None):
        self.header(final, 0)
        self.align()
        self.put(len(data), 16)
        self.put((~len(data) & 0xffff) if nlen is None else nlen, 16)
        self.out += data

    @staticmethod
    def length_symbol(n):
        if n == 258:
            return 285, 0, 0
        if n < 11:
            return 254 + n, 0, 0
        e = (n - 3).bit_length() - 3
        return 261 + 4 * e + (((n - 3) >> e) & 3), e, (n - 3) & ((1 << e) - 1)

    @staticmethod
    def distance_symbol(d):
        if d < 5:
            return d - 1, 0, 0
        e = (d - 1).bit_length() - 2
        return 2 * e + 2 + (((d - 1) >> e) & 1), e, (d - 1) & ((1 << e) - 1)

    def tokens(self, toks, lit=FIXED_LIT, dist=None):
        """toks: ints (literals), (length, distance) pairs, "end", or ("lit", symbol) / ("dist", symbol) for raw symbols."""
        for t in toks:
            if t == "end":
                self.code(lit[256])
            elif isinstance(t, int):
                self.code(lit[t])
            elif t[0] == "lit":
                self.code(lit[t[1]])
            elif t[0] == "dist":
                self.code((t[1], 5) if dist is None else dist[t[1]])
            else:
                s, e, v = self.length_symbol(t[0])
                self.code(lit[s])
                self.put(v, e)
                s, e, v = self.distance_symbol(t[1])
                self.code((s, 5) if dist is None else dist[s])
                self.put(v, e)

    def dynamic_header(self, final, cl_tokens, hlit, hdist, cl_lens=CL_LENS, hclen=19):
        """cl_tokens: [(code-length symbol, extra bits' value)]."""
        self.header(final, 2)
        self.put(hlit - 257, 5)
        self.put(hdist - 1, 5)
        self.put(hclen - 4, 4)
        for i in range(hclen):
            self.put(cl_lens[CL_ORDER[i]], 3)
        codes = canonical(cl_lens)
        for s, extra in cl_tokens:
            self.code(codes[s])
            self.put(extra, {16: 2, 17: 3, 18: 7}.get(s, 0))


def length_tokens(lens):
    """Code-length tokens of `lens`, runs of zeros as 17 / 18."""
    out, i = [], 0
    while i < len(lens):
        j = i
        while j < len(lens) and lens[j] == 0:
            j += 1
        run = j - i
        if run >= 3:
            n = min(run, 138)
            out.append((18, n - 11) if n >= 11 else (17, n - 3))
            i += n
        else:
            out.append((lens[i], 0))
            i += 1
    return out


def expand(toks):
    """The bytes a token list stands for."""
    out = bytearray()
    for t in toks:
        if isinstance(t, int):
            out.append(t)
        elif t != "end" and t[0] not in ("lit", "dist"):
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


def zlib_wrap(deflate, stream, header=b"\x78\x9c"):
    return header + deflate + struct.pack(">I", zlib.adler32(stream))


# ---- the images ----
def noise(H, W, C, seed):
    """uint8 [H, W, C]: smooth enough that every filter type has something to do, noisy enough that no row is trivial."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (3 * xx + 5 * yy)[:, :, None] + 40 * np.arange(C)[None, None, :]
    return ((base + rng.integers(0, 24, (H, W, C))) % 256).astype(np.uint8)


def case(name, img, payload, cuts=(), mode=SERIAL):
    """A well-formed case: the file, the pixels [H, W, C], the mode after decode() and the joined IDAT data."""
    H, W, C = img.shape
    return SimpleNamespace(name=name, file=png_file(H, W, C, cut(payload, cuts)), want=img, mode=mode, payload=payload, status=0)


def _hand_fixed(name, toks):
    """A one-row greyscale image whose filtered stream is what the fixed-Huffman token list stands for (its first byte: filter 0)."""
    stream = expand(toks)
    assert stream[0] == 0
    b = Bits()
    b.header(1, 1)
    b.tokens(toks + ["end"])
    img = np.frombuffer(stream[1:], dtype=np.uint8).reshape(1, -1, 1)
    return case(name, img, zlib_wrap(b.bytes(), stream))


def _dynamic_case():
    """Two dynamic blocks by hand: code lengths 1 .. 15, a zero run (code 17) laid across the literal/distance boundary, ONE distance
    code of length 1 (distance 4); then a block with no distance code at all."""
    lit = [k + 1 for k in range(13)] + [15, 15] + [0] * 241 + [15, 15]          # symbols 0 .. 12, 13, 14, 256, 257; complete
    dist = [0, 0, 0, 1]
    toks1 = [0] + list(range(1, 15)) + [(3, 4), 7, 7, (3, 4)]
    toks2 = [1, 2, 3, 12, 13, 14]
    stream = expand(toks1 + toks2)
    b = Bits()
    cl = length_tokens(lit + [0, 0, 0] + dist)                                      # hlit = 261: 258 .. 260 are zeros, joined with the distance zeros
    assert (17, 3) in cl
    b.dynamic_header(0, cl, 261, 4)
    b.tokens(toks1 + ["end"], canonical(lit), canonical(dist))
    b.dynamic_header(1, length_tokens(lit + [0]), 258, 1)
    b.tokens(toks2 + ["end"], canonical(lit))
    img = np.frombuffer(stream[1:], dtype=np.uint8).reshape(1, -1, 1)
    return case("dynamic-by-hand", img, zlib_wrap(b.bytes(), stream))


def _compressed(stream, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    return c.compress(stream) + c.flush()


def pillow_file(img):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img[:, :, 0] if img.shape[2] == 1 else img).save(buf, format="PNG")
    return buf.getvalue()


def wellformed():
    """Every well-formed case that needs no encoder of this project."""
    out = []
    for H, W in ((1, 1), (1, 7), (7, 1), (37, 45)):
        for C in (1, 2, 3, 4):
            for first in (range(5) if H < 5 else (3, 4)):
                img = noise(H, W, C, 100 * H + 10 * W + C)
                out.append(case(f"filters-{H}x{W}x{C}-first{first}", img, _compressed(filtered(img, cycling(H, first)))))
    for H in (63, 64, 65, 129, 255, 256, 257):                                    # (the unfilter takes 256 rows per group)
        img = noise(H, 5, 3, H)
        out.append(case(f"rows-{H}", img, _compressed(filtered(img, cycling(H, 3)))))
    for W in (15, 16, 17, 33):                                                    # (and 16 pixels per step)
        img = noise(7, W, 4, W)
        out.append(case(f"width-{W}", img, _compressed(filtered(img, cycling(7, 4)))))
    big = noise(300, 400, 3, 9)
    stream = filtered(big, cycling(300, 0))
    for name, kw in (("level0", dict(level=0)), ("fixed", dict(strategy=zlib.Z_FIXED)), ("huffman-only", dict(strategy=zlib.Z_HUFFMAN_ONLY)),
                     ("rle", dict(strategy=zlib.Z_RLE)), ("level1", dict(level=1)), ("level9", dict(level=9))):
        out.append(case(f"zlib-{name}-300x400", big, _compressed(stream, **kw)))
    small = noise(7, 7, 3, 5)                                                      # S = 154: every distance fits a 256-byte window
    s7 = filtered(small, cycling(7, 1))
    out.append(case("window-256", small, zlib_wrap(_compressed(s7, wbits=-9), s7, header=b"\x08\x1d")))
    rng = np.random.default_rng(3)
    far = [0] + [int(v) for v in rng.integers(0, 256, 32767)]
    out.append(_hand_fixed("fixed-258-at-32768", far + [(258, 32768)] + list(range(10))))
    b = Bits()                                                                     # length 3 at distance 1, 258 at distance 2, an empty stored block
    t1, t2 = [0, 7, (3, 1), 1, 2, (258, 2)], [5, (10, 200)]
    b.header(0, 1)
    b.tokens(t1 + ["end"])
    b.stored(b"", 0)
    b.header(1, 1)
    b.tokens(t2 + ["end"])
    stream2 = expand(t1 + t2)
    out.append(case("fixed-overlaps-and-empty-stored", np.frombuffer(stream2[1:], dtype=np.uint8).reshape(1, -1, 1), zlib_wrap(b.bytes(), stream2)))
    out.append(_dynamic_case())
    # foreign files whose chunk count meets the banded rule: 60 x 120 RGB, identical random rows, filter 0: S = 21 660, two bands
    rows = np.tile(rng.integers(0, 256, (1, 120, 3), dtype=np.uint8), (60, 1, 1))
    s60 = filtered(rows, [0] * 60)
    assert len(s60) == 21660
    for name, flush, mode in (("sync-flush", zlib.Z_SYNC_FLUSH, SERIAL), ("full-flush", zlib.Z_FULL_FLUSH, BANDED)):
        c = zlib.compressobj(9)
        first = c.compress(s60[:BAND]) + c.flush(flush)
        payload = first + c.compress(s60[BAND:]) + c.flush()
        out.append(case(f"foreign-{name}", rows, payload, cuts=[len(first)], mode=mode))
    plain = _compressed(s60, level=9)
    out.append(case("foreign-cut-in-the-middle", rows, plain, cuts=[len(plain) // 2], mode=SERIAL))
    return out


def pillow_cases():
    out = []
    for mode, C in (("L", 1), ("LA", 2), ("RGB", 3), ("RGBA", 4)):
        img = noise(300, 400, C, 20 + C)
        out.append(SimpleNamespace(name=f"pillow-{mode}-300x400", file=pillow_file(img), want=img, mode=SERIAL, payload=None, status=0))
    return out


OWN = ("one-band-plus-one", "batch-163x178", "run-across-cut", "constant-300x400", "random-300x400")


def own_inputs():
    """[(name, image [3, H, W] float32 or uint8, filter_none)]: this project's own files, to be written by its encoder."""
    out = []
    for name, imgs, fnone in P.cases(BAND):
        if name.startswith(OWN):
            out += [(f"own-{name}[{b}]", imgs[b], fnone) for b in range(imgs.shape[0])]
    assert len(out) == 6
    return out


def own_case(name, data, img):
    want = P.quantise(img).transpose(1, 2, 0)
    H, W, _ = want.shape
    nb = -(-(H * (1 + 3 * W)) // BAND)
    return SimpleNamespace(name=name, file=data, want=np.ascontiguousarray(want), mode=BANDED if nb > 1 else SERIAL, payload=None, status=0)


def composite_case():
    """256 x 256 RGBA: R = x, G = 255 - x, B = 7 x mod 256, A = y -- every (value, alpha) pair."""
    yy, xx = np.mgrid[0:256, 0:256]
    img = np.stack([xx, 255 - xx, (7 * xx) % 256, yy], axis=2).astype(np.uint8)
    return case("composite-256x256", img, _compressed(filtered(img, cycling(256, 2))))


def composite_reference(img, bg):
    """[REF scene/dataset_readers.py:214-218] in numpy float64: uint8 [H, W, 3]."""
    im_data = img.astype(np.float64)
    norm_data = im_data / 255.0
    arr = norm_data[:, :, :3] * norm_data[:, :, 3:4] + np.asarray(bg, dtype=np.float64) * (1 - norm_data[:, :, 3:4])
    return np.array(arr * 255.0, dtype=np.byte).view(np.uint8)


# ---- the malformed files: all 9 x 11 RGB (S = 306), to sit between two good images of that shape ----
MH, MW, MC = 9, 11, 3


def good_small(seed):
    img = noise(MH, MW, MC, seed)
    return case(f"good-{seed}", img, _compressed(filtered(img, cycling(MH, seed % 5))))


def _bad(name, status, payload, deflate_is_bad=True):
    """deflate_is_bad: zlib.decompress must refuse the payload; otherwise it must accept it (the fault is the PNG's, not the stream's)."""
    return SimpleNamespace(name=name, file=png_file(MH, MW, MC, [payload]), want=None, mode=SERIAL, payload=payload, status=status,
                           deflate_is_bad=deflate_is_bad)


def _raw(build, header=b"\x78\x9c"):
    b = Bits()
    build(b)
    return header + b.bytes() + b"\x00\x00\x00\x01"


def malformed():
    img = noise(MH, MW, MC, 77)
    stream = filtered(img, cycling(MH, 2))
    S = len(stream)
    good = _compressed(stream)
    out = [_bad("cut-by-one-byte", TRUNCATED, good[:-1]), _bad("cut-by-half", TRUNCATED, good[:len(good) // 2])]
    out.append(_bad("block-type-3", BLOCK_TYPE, _raw(lambda b: b.header(1, 3))))
    out.append(_bad("stored-len-nlen", STORED_LEN, _raw(lambda b: b.stored(stream[:100], 1, nlen=0x1234))))
    out.append(_bad("hlit-287", TOO_MANY_CODES, _raw(lambda b: b.dynamic_header(1, [], 287, 1))))
    out.append(_bad("clen-oversubscribed", CLEN_CODE, _raw(lambda b: b.dynamic_header(1, [], 257, 1, cl_lens=[1] * 19, hclen=4))))
    out.append(_bad("code-16-first", REPEAT_FIRST, _raw(lambda b: b.dynamic_header(1, [(16, 0)], 257, 1))))
    out.append(_bad("repeat-past-the-end", REPEAT_OVERRUN, _raw(lambda b: b.dynamic_header(1, [(18, 127), (18, 127)], 257, 1))))
    over = [1, 1, 1] + [0] * 253 + [1]
    out.append(_bad("literal-oversubscribed", LIT_OVERSUBSCRIBED, _raw(lambda b: b.dynamic_header(1, length_tokens(over + [1]), 257, 1))))
    under = [2] + [0] * 255 + [2]
    out.append(_bad("literal-incomplete", LIT_INCOMPLETE, _raw(lambda b: b.dynamic_header(1, length_tokens(under + [1]), 257, 1))))
    no256 = [1, 1] + [0] * 255
    out.append(_bad("no-end-of-block", NO_END_OF_BLOCK, _raw(lambda b: b.dynamic_header(1, length_tokens(no256 + [1]), 257, 1))))
    for s in (286, 287):
        out.append(_bad(f"fixed-symbol-{s}", LIT_SYMBOL, _raw(lambda b, s=s: (b.header(1, 1), b.tokens([0, 1, ("lit", s), "end"])))))
    for s in (30, 31):
        out.append(_bad(f"fixed-distance-{s}", DIST_SYMBOL, _raw(lambda b, s=s: (b.header(1, 1), b.tokens([0, 1, 2, ("lit", 257), ("dist", s), "end"])))))
    out.append(_bad("distance-before-the-start", DIST_TOO_FAR, _raw(lambda b: (b.header(1, 1), b.tokens([0, 1, (3, 3), "end"])))))
    out.append(_bad("one-byte-too-many", OUTPUT_LONG, _compressed(stream + b"\x00"), deflate_is_bad=False))
    out.append(_bad("one-byte-too-few", OUTPUT_SHORT, _compressed(stream[:-1]), deflate_is_bad=False))
    out.append(_bad("wrong-adler", ADLER, good[:-1] + bytes([good[-1] ^ 1])))
    five = bytearray(stream)
    five[4 * (1 + MC * MW)] = 5
    out.append(_bad("filter-byte-5", FILTER, _compressed(bytes(five)), deflate_is_bad=False))
    raw = _compressed(stream, wbits=-15)
    tail = struct.pack(">I", zlib.adler32(stream))
    out.append(_bad("zlib-cm-7", ZLIB_METHOD, b"\x77\x09" + raw + tail))
    out.append(_bad("zlib-fdict", ZLIB_FDICT, b"\x78\x20" + raw + tail))
    out.append(_bad("zlib-fcheck", ZLIB_FCHECK, b"\x78\x9d" + raw + tail))
    assert S == MH * (1 + MC * MW) and 0x7709 % 31 == 0 and 0x7820 % 31 == 0 and 0x789d % 31
    return out
