"""The test's own statements about a baseline JPEG file, independent of csrc/jpeg_core.h: a marker walk, an entropy decoder that
returns the quantised coefficients of every block (pure Python / numpy), stages 1-3 of include/gp_jpeg.h in float64, and a RIFF walk
for the Motion-JPEG container."""
import struct

import numpy as np

from jpeg_cases import ZIGZAG

NAMES = {0xd8: "SOI", 0xe0: "APP0", 0xdb: "DQT", 0xc0: "SOF0", 0xc4: "DHT", 0xdd: "DRI", 0xda: "SOS", 0xd9: "EOI"}


def walk(data):
    """The segments before the entropy-coded data and what they hold; the data itself split at its RST markers.  Asserts the marker
    syntax, the stuffing rule and the RST numbering."""
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    info = {"order": ["SOI"], "dqt": {}, "dht": [], "dht_tables": {}}
    pos = 2
    while True:
        assert data[pos] == 0xff and data[pos + 1] in NAMES, (pos, data[pos:pos + 2])
        kind = NAMES[data[pos + 1]]
        n = struct.unpack(">H", data[pos + 2:pos + 4])[0]
        body = data[pos + 4:pos + 2 + n]
        assert len(body) == n - 2
        info["order"].append(kind)
        if kind == "APP0":
            info["app0"] = body
        elif kind == "DQT":
            assert len(body) == 65 and body[0] in (0, 1)
            nat = [0] * 64
            for k in range(64):
                nat[ZIGZAG[k]] = body[1 + k]
            info["dqt"][body[0]] = nat
        elif kind == "SOF0":
            P, H, W, nc = struct.unpack(">BHHB", body[:6])
            assert P == 8 and nc == 3 and len(body) == 6 + 9
            info["H"], info["W"] = H, W
            info["comps"] = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(3)]
        elif kind == "DHT":
            info["dht"].append(data[pos:pos + 2 + n])
            bits, vals = body[1:17], body[17:]
            assert len(vals) == sum(bits)
            table, code, k = {}, 0, 0
            for length in range(1, 17):
                for _ in range(bits[length - 1]):
                    table[(length, code)] = vals[k]
                    code += 1
                    k += 1
                code <<= 1
            info["dht_tables"][body[0]] = table
        elif kind == "DRI":
            info["dri"] = struct.unpack(">H", body)[0]
        elif kind == "SOS":
            assert body[0] == 3 and body[-3:] == bytes([0, 63, 0])
            info["scan"] = [(body[1 + 2 * i], body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(3)]
            pos += 2 + n
            break
        pos += 2 + n
    ecs = data[pos:-2]
    segments, cur, i, expect, stuffed = [], bytearray(), 0, 0, 0
    while i < len(ecs):
        b = ecs[i]
        if b != 0xff:
            cur.append(b)
            i += 1
            continue
        assert i + 1 < len(ecs), "a lone 0xFF ends the data"
        nxt = ecs[i + 1]
        if nxt == 0:
            cur.append(0xff)
            stuffed += 1
        else:
            assert 0xd0 <= nxt <= 0xd7 and nxt - 0xd0 == expect % 8, (i, nxt, expect)       # nothing but 0x00 or the next RST
            expect += 1
            segments.append(bytes(cur))
            cur = bytearray()
        i += 2
    segments.append(bytes(cur))
    info["segments"], info["rst"], info["stuffed"] = segments, expect, stuffed
    return info


class _Bits:
    def __init__(self, data):
        self.v = int.from_bytes(data, "big") if data else 0
        self.n = 8 * len(data)
        self.pos = 0

    def take(self, k):
        assert self.pos + k <= self.n, "ran out of bits"
        r = (self.v >> (self.n - self.pos - k)) & ((1 << k) - 1)
        self.pos += k
        return r

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.take(1)
            if (length, code) in table:
                return table[(length, code)]
        raise AssertionError("no code of 16 bits or fewer")


def _extend(v, cat):
    return v if cat == 0 or v >> (cat - 1) else v - (1 << cat) + 1


def decode(data):
    """(info of walk(), coefficients, stats): coefficients[c] is an int array [blocks down, blocks across, 64] in NATURAL order of
    the quantised coefficients of component c, over the MCU-padded plane; stats counts what the scan exercised."""
    info = walk(data)
    H, W = info["H"], info["W"]
    hmax, vmax = max(c[1] for c in info["comps"]), max(c[2] for c in info["comps"])
    mw, mh = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    coef = [np.zeros((mh * c[2], mw * c[1], 64), dtype=np.int64) for c in info["comps"]]
    stats = {"zrl": 0, "no_eob": 0, "max_ac_cat": 0, "max_dc_cat": 0, "blocks": 0}
    interval = info.get("dri", 0) or mw * mh
    assert len(info["segments"]) == -(-mw * mh // interval)
    m = 0
    for seg in info["segments"]:
        bits = _Bits(seg)
        pred = [0, 0, 0]
        for _ in range(min(interval, mw * mh - m)):
            my, mx = divmod(m, mw)
            for ci, (cid, h, v, tq) in enumerate(info["comps"]):
                _, td, ta = info["scan"][ci]
                dct, act = info["dht_tables"][td], info["dht_tables"][0x10 | ta]
                for by in range(v):
                    for bx in range(h):
                        z = [0] * 64
                        cat = bits.symbol(dct)
                        stats["max_dc_cat"] = max(stats["max_dc_cat"], cat)
                        pred[ci] += _extend(bits.take(cat), cat)
                        z[0] = pred[ci]
                        k = 1
                        while k < 64:
                            rs = bits.symbol(act)
                            run, cat = rs >> 4, rs & 15
                            if cat == 0:
                                if run == 15:
                                    stats["zrl"] += 1
                                    k += 16
                                    continue
                                assert run == 0, rs
                                break
                            k += run
                            assert k < 64
                            stats["max_ac_cat"] = max(stats["max_ac_cat"], cat)
                            z[k] = _extend(bits.take(cat), cat)
                            k += 1
                        else:
                            stats["no_eob"] += 1
                        stats["blocks"] += 1
                        nat = coef[ci][my * v + by, mx * h + bx]
                        for kk in range(64):
                            nat[ZIGZAG[kk]] = z[kk]
            m += 1
        rest = bits.n - bits.pos
        assert rest < 8 and (rest == 0 or bits.take(rest) == (1 << rest) - 1), "an interval ends with fewer than 8 one-bits"
    assert m == mw * mh
    return info, coef, stats


# ---- stages 1-3 of gp_jpeg.h, restated ----
def ycc(img8):
    """int64 [3, H, W]: Y Cb Cr of uint8 [3, H, W] by the header's 16-bit fixed point."""
    R, G, B = (img8[c].astype(np.int64) for c in range(3))
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11058 * R - 21710 * G + 32768 * B + (128 << 16) + 32768) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32768) >> 16
    return np.clip(np.stack([Y, Cb, Cr]), 0, 255)


def planes(img8, sub420):
    """The three planes as the transform sees them: padded to whole MCUs by replication, chroma averaged 2 x 2 with 4:2:0."""
    _, H, W = img8.shape
    ms = 16 if sub420 else 8
    p = np.pad(ycc(img8), ((0, 0), (0, -H % ms), (0, -W % ms)), mode="edge")
    if not sub420:
        return [p[0], p[1], p[2]]
    sub = lambda a: (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2
    return [p[0], sub(p[1]), sub(p[2])]


def dct_matrix():
    u, x = np.mgrid[0:8, 0:8]
    C = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    C[0] = np.sqrt(1 / 8)
    return C


def exact_ratio(plane, table):
    """float64 [blocks down, blocks across, 64]: F / q of every block of the plane, natural order."""
    C = dct_matrix()
    h, w = plane.shape
    s = (plane.astype(np.float64) - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)
    F = np.einsum("vy,abyx,ux->abvu", C, s, C)
    return F.reshape(h // 8, w // 8, 64) / np.asarray(table, dtype=np.float64)


def round_half_away(x):
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


# ---- the container ----
def riff_walk(data):
    """Walk a RIFF 'AVI ' file; asserts that every size adds up.  Returns {"avih", "strh", "strf", "frames": [(offset of the chunk in
    the file, payload)], "index": [(ckid, flags, offset, size)], "movi_tag": offset of the 'movi' tag}."""
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI "
    assert struct.unpack("<I", data[4:8])[0] == len(data) - 8
    out = {"frames": [], "index": [], "lists": []}

    def chunks(lo, hi, depth):
        pos = lo
        while pos < hi:
            cid, n = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
            end = pos + 8 + n
            assert end <= hi, (cid, pos, n, hi)
            if cid == b"LIST":
                kind = data[pos + 8:pos + 12]
                out["lists"].append(kind)
                if kind == b"movi":
                    out["movi_tag"] = pos + 8
                chunks(pos + 12, end, depth + 1)
            elif cid == b"00dc":
                out["frames"].append((pos, data[pos + 8:end]))
            elif cid == b"idx1":
                assert n % 16 == 0
                out["index"] = [struct.unpack("<4sIII", data[pos + 8 + 16 * i:pos + 24 + 16 * i]) for i in range(n // 16)]
            else:
                out[cid.decode()] = data[pos + 8:end]
            pos = end + (n & 1)                      # chunks are padded to an even length
        assert pos == hi, (pos, hi, depth)

    chunks(12, len(data), 0)
    assert out["lists"] == [b"hdrl", b"strl", b"movi"]
    return out
