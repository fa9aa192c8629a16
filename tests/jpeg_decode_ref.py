"""The arithmetic of include/gp_jpeg_decode.h restated in numpy, independent of csrc/jpeg_decode_core.h: the quantised coefficients come
from the entropy decoder of tests/jpeg_ref.py; dequantisation, the two-pass integer IDCT, the triangle upsampling of 4:2:0 chroma and
the colour transform are written out here in int64."""
import struct

import numpy as np

import jpeg_ref as R


def strip(data):
    """The file without its COM and APPn (n > 0) segments -- jpeg_ref.walk knows the segments this project writes."""
    out, pos = bytearray(data[:2]), 2
    while True:
        m = data[pos + 1]
        n = struct.unpack(">H", data[pos + 2:pos + 4])[0]
        if not (0xe1 <= m <= 0xef or m == 0xfe):
            out += data[pos:pos + 2 + n]
        pos += 2 + n
        if m == 0xda:
            return bytes(out) + data[pos:]


def idct_pass(d, axis, shift):
    """One pass of the header's transform along `axis` (length 8) of the int64 array d."""
    i = [np.take(d, k, axis=axis) for k in range(8)]
    z1 = (i[2] + i[6]) * 4433
    t2 = z1 - i[6] * 15137
    t3 = z1 + i[2] * 6270
    t0 = (i[0] + i[4]) * 8192
    t1 = (i[0] - i[4]) * 8192
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3 = z3 * -16069 + z5
    z4 = z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([(o + (1 << (shift - 1))) >> shift for o in out], axis=axis)


def plane(coef, table):
    """uint8 [8 blocks down, 8 blocks across]: the samples of the blocks coef [down, across, 64] (natural order), dequantised by `table`."""
    d = (coef.astype(np.int64) * np.asarray(table, dtype=np.int64)).reshape(coef.shape[0], coef.shape[1], 8, 8)
    d = idct_pass(d, 2, 11)            # over the columns: along the rows' index
    d = idct_pass(d, 3, 18)            # over the rows
    s = np.clip(d + 128, 0, 255)
    return s.transpose(0, 2, 1, 3).reshape(coef.shape[0] * 8, coef.shape[1] * 8)


def upsample(c, H, W):
    """int64 [H, W] from the chroma plane c (at least ceil(H / 2) x ceil(W / 2); only that part is read)."""
    ch, cw = -(-H // 2), -(-W // 2)
    c = c[:ch, :cw].astype(np.int64)
    if cw <= 2:
        return np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)[:H, :W]
    above = np.concatenate([c[:1], c[:-1]])
    below = np.concatenate([c[1:], c[-1:]])
    s = np.empty((2 * ch, cw), dtype=np.int64)
    s[0::2] = 3 * c + above
    s[1::2] = 3 * c + below
    left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((2 * ch, 2 * cw), dtype=np.int64)
    out[:, 0::2] = (3 * s + left + 8) >> 4
    out[:, 1::2] = (3 * s + right + 7) >> 4
    return out[:H, :W]


def pixels(data):
    """uint8 [H, W, 3]: R G B of the baseline file `data` by the header's arithmetic; also the entropy decoder's stats."""
    info, coef, stats = R.decode(strip(data))
    H, W = info["H"], info["W"]
    Y, Cb, Cr = (plane(coef[i], info["dqt"][info["comps"][i][3]]) for i in range(3))
    Y = Y[:H, :W].astype(np.int64)
    if info["comps"][0][1] == 2:
        Cb, Cr = upsample(Cb, H, W), upsample(Cr, H, W)
    else:
        Cb, Cr = Cb[:H, :W].astype(np.int64), Cr[:H, :W].astype(np.int64)
    cb, cr = Cb - 128, Cr - 128
    rgb = np.stack([Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), Y + ((116130 * cb + 32768) >> 16)], axis=2)
    return np.clip(rgb, 0, 255).astype(np.uint8), stats
