"""No GPU: include/gp_jpeg.h against the binding's table; the quantisation and Huffman tables against Pillow's; the JPEG encoder's
workgroup programs (csrc/jpeg_core.h) run lane by lane on the CPU (tests/jpeg_emulate.cpp) with Pillow's decoder, the test's own marker
walk and entropy decoder (tests/jpeg_ref.py) and a float64 restatement of the colour transform, subsampling and DCT as the oracle;
the files against Pillow's own encoding at the same tables; the Motion-JPEG container against a RIFF walk; the refusals that need no
device."""
import ctypes as C
import io
import os
import re
import struct
import subprocess
import threading
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

import abi_check
import jpeg_cases as J
import jpeg_ref as R
import png_cases as P
from gaussianprediction_amd import _lib, jpeg_ops as JPG

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SUBS = ("420", "444")

# PSNR (dB, of Pillow's decoding against the 8-bit source) and file size against Pillow's own encoder at the same tables, subsampling
# and restart interval, measured through the emulator over every case at both subsamplings (DESIGN section 14 has the table).
#   PSNR at 4:4:4: -0.038 .. +0.064 dB of Pillow's.
#   PSNR at 4:2:0: the worst deficits are 0.212 dB (blobs-80x96-1), 0.113 (blobs-80x96-0) and 0.111 (textured-8x8): smooth, dark images
#   of high PSNR, where the chroma filter shows.  gp_jpeg.h rounds a 2 x 2 chroma mean as (a + b + c + d + 2) >> 2, half a step up
#   on average; libjpeg adds 1 and 2 in turn along a row, which has no mean offset.  With that one line changed in a scratch copy of
#   the emulator the blob images come out +0.005 .. +0.076 dB against Pillow, so the filter is the whole of the deficit.  The frames
#   the GPU tests render (tests/test_gpu_jpeg.py; the device's files are the emulator's, byte for byte) reach 0.266 dB (the first
#   frame of render_kpts' video), which is the worst case measured anywhere.
#   Size at 4:4:4: 0.9932 .. 1.0017 of Pillow's.
#   Size at 4:2:0: 0.9979 .. 1.0790; whole-MCU shapes are 0.995 .. 1.002 of Pillow's, and the excess belongs to shapes with partial
#   MCUs (rows-cross-40x88 is the worst): gp_jpeg.h extends the planes to whole MCUs by replication and codes those samples, where
#   libjpeg replicates to whole blocks only and fills the rest of an MCU with blocks of no AC coefficient.
#   The constant images and the 1 x 1 image are byte-identical to Pillow's.
# A bar is the worst measured case plus a margin for what may differ between builds of libjpeg-turbo -- its DCT rounds differently
# from ours (and between its SIMD and C paths), and its 4:2:0 chroma filter adds 1 and 2 in turn before the shift where ours adds 2:
# 0.05 dB and 1 % of the size.
PSNR_MARGIN_DB = 0.266 + 0.05
SIZE_MARGIN = {"420": 1.0790 + 0.01, "444": 1.0017 + 0.01}

# ---- one signature per entry point, two statements of it: include/gp_jpeg.h and jpeg_ops.PROTOTYPES ----
_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "gp_stream_t": _lib.Ptr}
_POINTEES = {"void", "uint8_t", "uint32_t"}


def test_prototype_table_equals_the_header():
    protos = abi_check.check_table(JPG.ABI, 5, _SCALARS, _POINTEES)
    assert JPG.ABI.prototypes is JPG.PROTOTYPES and JPG.ABI.header == "gp_jpeg.h"
    assert protos["gp_jpeg_encode"][1][-1] == "gp_stream_t"        # the stream is the last parameter


def test_symbols_and_constants():
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_JPEG_[A-Z0-9_]+) (\d+)u?\b", abi_check.header_text("gp_jpeg.h"))}
    assert defs["GP_JPEG_ABI_VERSION"] == JPG.GP_JPEG_ABI_VERSION == JPG.ABI.version == 1
    abi_check.check_applied(JPG.ABI)
    assert (defs["GP_JPEG_RESTART_MCUS"], defs["GP_JPEG_BLOCK_BITS"], defs["GP_JPEG_HEAD_BYTES"], defs["GP_JPEG_MAX_BATCH"], defs["GP_JPEG_MAX_SIDE"],
            defs["GP_JPEG_420"], defs["GP_JPEG_444"]) == \
        (JPG.RESTART_MCUS, JPG.BLOCK_BITS, JPG.HEAD_BYTES, JPG.MAX_BATCH, JPG.MAX_SIDE, JPG.SUB_420, JPG.SUB_444)
    assert JPG.BLOCK_BITS == 11 + 11 + 63 * (16 + 10)
    # one interval at its worst, stuffed, stays under the 64 KB of LDS a kernel gets without opting in, with room for its tables
    assert 8 <= JPG.RESTART_MCUS <= 16 and 2 * -(-JPG.RESTART_MCUS * 6 * JPG.BLOCK_BITS // 8) < 65536 - 16384
    err = re.search(r"GP_JPEG_DCT_ERR = 2\^-(\d+)", open(os.path.join(ROOT, "include", "gp_jpeg.h")).read())
    assert err and 2.0 ** -int(err.group(1)) == DCT_ERR


DCT_ERR = 2.0 ** -12            # include/gp_jpeg.h: the bound on the integer transform's error against the exact DCT


def _worst_case(H, W, sub):
    ms, k = (16, 6) if sub == "420" else (8, 3)
    nmcu = -(-H // ms) * -(-W // ms)
    total, left = JPG.HEAD_BYTES, nmcu
    while left > 0:
        n = min(left, JPG.RESTART_MCUS)
        total += 2 * -(-n * k * JPG.BLOCK_BITS // 8) + 2          # the interval stuffed, and RST or EOI behind it
        left -= n
    return total


def test_bound_is_the_derived_worst_case_and_refuses_outside_the_limits():
    for H, W in ((1, 1), (17, 33), (45, 67), (144, 130), (1014, 1352), (1, 5000), (5000, 1)):
        for sub in SUBS:
            b = JPG.bound(H, W, sub)
            assert b % 8 == 0 and _worst_case(H, W, sub) <= b < _worst_case(H, W, sub) + 8, (H, W, sub, b)
    assert JPG.bound(37, 45) == JPG.bound(37, 45, "420")
    s = JPG.lib().gp_jpeg_scratch_bytes
    assert s(1, 163, 178, 0) > 0 and s(32, 1014, 1352, 0) < 1 << 29
    for bad, word in (((0, 4, 4, 0), b"B = 0"), ((65536, 4, 4, 0), b"B = 65536"), ((1, 0, 4, 0), b"H = 0"), ((1, 4, 65536, 0), b"W = 65536")):
        assert s(*bad) == -1 and word in JPG.lib().gp_last_error(), bad
    assert JPG.lib().gp_jpeg_bound(65535, 65535, 0) == -1 and b"2^31" in JPG.lib().gp_last_error()


def test_refusals_need_no_gpu():
    l = JPG.lib()
    lum, chr_ = (C.c_uint8 * 64)(), (C.c_uint8 * 64)()
    for q in (0, 101):
        assert l.gp_jpeg_quant_tables(q, lum, chr_) == 1 and b"quality = %d" % q in l.gp_last_error()
        with pytest.raises(ValueError, match="quality"):
            JPG.quant_tables(q)
    for bad, word in (((0, 4, 0), b"H = 0"), ((4, 0, 0), b"W = 0"), ((4, 4, 2), b"subsampling = 2"), ((4, 4, -1), b"subsampling = -1")):
        assert l.gp_jpeg_bound(*bad) == -1 and word in l.gp_last_error(), bad
    with pytest.raises(ValueError, match="subsampling"):
        JPG.bound(4, 4, "422")
    assert l.gp_jpeg_quant_tables(90, lum, chr_) == 0
    big = JPG.bound(4, 4)
    for args, word in (((0, 4, 4, None, 0, lum, chr_, 0, None, big, None, None, None), b"B = 0"),
                       ((1, 4, 0, None, 0, lum, chr_, 0, None, big, None, None, None), b"W = 0"),
                       ((1, 4, 4, None, 2, lum, chr_, 0, None, big, None, None, None), b"src_kind = 2"),
                       ((1, 4, 4, None, 0, lum, chr_, 3, None, big, None, None, None), b"subsampling = 3"),
                       ((1, 4, 4, None, 0, lum, chr_, 0, None, big - 8, None, None, None), b"out_stride"),
                       ((1, 4, 4, None, 0, lum, chr_, 0, None, big, None, None, None), b"null")):
        assert l.gp_jpeg_encode(*args) == 1 and word in l.gp_last_error(), args      # the C entry refuses before it looks at a device pointer
    x = torch.zeros(3, 8, 8)
    for call in (lambda: JPG.encode(x), lambda: JPG.encode([x, x]), lambda: JPG.encode_to_bytes(x[None]), lambda: JPG.encode(x.to(torch.uint8))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for bad in (torch.zeros(8, 8), torch.zeros(1, 4, 8, 8), torch.zeros(3, 8, 8, dtype=torch.int32)):
        with pytest.raises(RuntimeError, match="images must be"):
            JPG.encode(bad)
    with pytest.raises(ValueError, match="qtables"):
        JPG.encode(x, qtables=([0] * 64, [1] * 64))
    w = JPG.JpegWriter()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        w.submit(x, "never-written.jpg")
    w.close()
    assert not [t for t in threading.enumerate() if t.name.startswith("JpegWriter")]
    with pytest.raises(RuntimeError, match="closed"):
        w.submit(x, "never-written.jpg")
    with pytest.raises(ValueError, match="quality"):
        JPG.JpegWriter(quality=0)


# ---- Pillow as the reference for the tables ----
def _pillow_lists_natural():
    """(whether this Pillow takes `qtables=` in natural order, whether its `.quantization` lists natural order): found out from a
    table that tells the two orders apart."""
    probe = list(range(1, 65))
    buf = io.BytesIO()
    Image.new("RGB", (8, 8)).save(buf, "JPEG", qtables=[probe, probe])
    data = buf.getvalue()
    in_file = list(data[data.index(b"\xff\xdb") + 5:][:64])                    # zigzag order, by the standard
    natural = [0] * 64
    for k in range(64):
        natural[J.ZIGZAG[k]] = in_file[k]
    assert probe in (natural, in_file)
    listed = list(Image.open(io.BytesIO(data)).quantization[0])
    assert listed in (natural, in_file)
    return probe == natural, listed == natural


def _as_pillow(table, natural):
    return list(table) if natural else [table[J.ZIGZAG[k]] for k in range(64)]


def _pillow_encode(img8, qtables, sub, **kw):
    given_natural, _ = _pillow_lists_natural()
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img8.transpose(1, 2, 0))).save(
        buf, "JPEG", qtables=[_as_pillow(t, given_natural) for t in qtables], subsampling={"420": 2, "444": 0}[sub], optimize=False,
        restart_marker_blocks=JPG.RESTART_MCUS, **kw)
    return buf.getvalue()


def _quantization(data):
    """Pillow's reading of the file's tables, as (luminance, chrominance) in natural order."""
    _, listed_natural = _pillow_lists_natural()
    q = Image.open(io.BytesIO(data)).quantization
    out = []
    for i in (0, 1):
        t = list(q[i])
        if not listed_natural:
            nat = [0] * 64
            for k in range(64):
                nat[J.ZIGZAG[k]] = t[k]
            t = nat
        out.append(t)
    return out


@pytest.mark.parametrize("quality", [1, 25, 50, 75, 90, 95, 100])
def test_quant_tables_equal_pillows(quality):
    buf = io.BytesIO()
    Image.new("RGB", (8, 8)).save(buf, "JPEG", quality=quality)
    lum, chr_ = JPG.quant_tables(quality)
    assert [lum, chr_] == _quantization(buf.getvalue())
    assert R.walk(buf.getvalue())["dqt"] == {0: lum, 1: chr_}                 # (and the test's own reading of the DQT segments)


# ---- the workgroup programs on the CPU ----
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return J.build_emulator(tmp_path_factory.mktemp("jpeg_emulate"))


CASES = {name: (img, qt) for name, img, qt in J.cases()}
Q90 = None


def _tables_of(qt):
    global Q90
    if qt is not None:
        return qt
    if Q90 is None:
        Q90 = JPG.quant_tables(90)
    return Q90


def _file(emulator, name, sub):
    img, qt = CASES[name]
    return emulator(img, sub, _tables_of(qt), key=(name, sub))


def test_emulators_tables_are_the_librarys(emulator):
    for q in (1, 37, 90):
        out = str(emulator.dir / "tables.bin")
        subprocess.check_call([emulator.exe, "tables", str(q), out], timeout=60)
        lum, chr_ = JPG.quant_tables(q)
        assert list(open(out, "rb").read()) == lum + chr_


def test_dht_segments_equal_pillows(emulator):
    ours = R.walk(_file(emulator, "textured-16x16", "420"))["dht"]
    theirs = R.walk(_pillow_encode(P.quantise(CASES["textured-16x16"][0]), _tables_of(None), "420"))["dht"]
    assert len(ours) == 4 and ours == theirs


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("name", list(CASES))
def test_every_case_decodes_and_its_markers_are_legal(emulator, name, sub):
    img, qt = CASES[name]
    qt = _tables_of(qt)
    _, H, W = img.shape
    data = _file(emulator, name, sub)
    assert len(data) <= JPG.bound(H, W, sub)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(data))
        im.load()
    assert im.size == (W, H) and im.mode == "RGB"
    assert _quantization(data) == [list(qt[0]), list(qt[1])]
    info = R.walk(data)
    assert info["order"] == ["SOI", "APP0", "DQT", "DQT", "SOF0", "DHT", "DHT", "DHT", "DHT", "DRI", "SOS"]
    assert info["app0"] == b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0" and len(data) - len(b"".join(info["segments"])) >= JPG.HEAD_BYTES
    assert (info["H"], info["W"]) == (H, W) and info["dqt"] == {0: list(qt[0]), 1: list(qt[1])}
    s = 2 if sub == "420" else 1
    assert info["comps"] == [(1, s, s, 0), (2, 1, 1, 1), (3, 1, 1, 1)] and info["scan"] == [(1, 0, 0), (2, 1, 1), (3, 1, 1)]
    nmcu = -(-H // (8 * s)) * -(-W // (8 * s))
    assert info["dri"] == JPG.RESTART_MCUS and info["rst"] == -(-nmcu // JPG.RESTART_MCUS) - 1 == len(info["segments"]) - 1


def test_the_cases_are_what_they_claim(emulator):
    R_ = JPG.RESTART_MCUS
    mcus = lambda name, ms: -(-CASES[name][0].shape[1] // ms) * -(-CASES[name][0].shape[2] // ms)
    assert -(-88 // 16) % R_ and -(-88 // 8) % R_                                       # rows-cross: intervals cross MCU rows
    assert mcus("wrap-144x130", 16) > 8 * R_ and mcus("wrap-144x130", 16) % R_ == 1     # more than 8 intervals; the last holds one MCU
    assert mcus("last-single-24x24", 8) % R_ == 1
    _, _, st = R.decode(_file(emulator, "checkerboard-ones", "444"))
    assert st["max_dc_cat"] == 11
    for sub in SUBS:
        info, coef, st = R.decode(_file(emulator, "noise-ones", sub))
        assert st["max_ac_cat"] == 10 and st["no_eob"] > 0 and info["stuffed"] >= 1, (sub, st, info["stuffed"])
        _, _, st = R.decode(_file(emulator, "bright-pixels-zrl", sub))
        assert st["zrl"] >= 2, (sub, st)
    x = CASES["edge-floats-37x45"][0]
    assert x.dtype == np.float32 and np.isnan(x).sum() == 1 and (x < 0).any() and (x[np.isfinite(x)] > 1).any()


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("name", list(CASES))
def test_coefficients_against_the_exact_transform(emulator, name, sub):
    """Every decoded coefficient is round-half-away(F / q) of the float64 transform, or one off where F / q lies within
    GP_JPEG_DCT_ERR / q of a half-integer -- what the header's error bound allows, and nothing else."""
    img, qt = CASES[name]
    qt = _tables_of(qt)
    info, coef, st = R.decode(_file(emulator, name, sub))
    planes = R.planes(P.quantise(img), sub == "420")
    differ = total = 0
    for c in range(3):
        table = np.asarray(qt[0 if c == 0 else 1], dtype=np.float64)
        ratio = R.exact_ratio(planes[c], table)
        assert ratio.shape == coef[c].shape, (ratio.shape, coef[c].shape)
        want = R.round_half_away(ratio)
        d = coef[c] - want
        assert np.abs(d).max() <= 1
        to_half = np.abs(np.abs(ratio) - np.floor(np.abs(ratio)) - 0.5)
        assert (to_half[d != 0] <= DCT_ERR / np.broadcast_to(table, ratio.shape)[d != 0] + 1e-9).all()
        differ += int((d != 0).sum())
        total += d.size
    print(f"{name} {sub}: {differ} of {total} coefficients differ from the exact transform's ({differ / total:.2e})")


def _psnr(a, b):
    mse = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def _decoded(data):
    return np.array(Image.open(io.BytesIO(data))).transpose(2, 0, 1)


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("name", list(CASES))
def test_against_pillows_encoder_at_the_same_tables(emulator, name, sub):
    img, qt = CASES[name]
    qt = _tables_of(qt)
    src = P.quantise(img)
    ours, theirs = _file(emulator, name, sub), _pillow_encode(src, qt, sub)
    po, pt = _psnr(_decoded(ours), src), _psnr(_decoded(theirs), src)
    print(f"{name} {sub}: PSNR {po:.3f} dB (Pillow {pt:.3f}, {po - pt:+.3f}), size {len(ours)} B (Pillow {len(theirs)}, {len(ours) / len(theirs):.4f})")
    assert po >= pt - PSNR_MARGIN_DB
    assert len(ours) <= len(theirs) * SIZE_MARGIN[sub]
    if name.startswith("constant") or name == "textured-1x1":
        assert ours == theirs                                                 # byte for byte


# ---- the container ----
def _jpeg_bytes(w, h, seed, odd=None):
    buf = io.BytesIO()
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)).save(buf, "JPEG", quality=60)
    data = buf.getvalue()
    if odd is not None and (len(data) & 1) != odd:
        data = data[:-2] + b"\xff" + data[-2:]          # (a fill byte before EOI: legal, and one byte longer)
    return data


def check_avi(data, n, width, height, rate, scale):
    """The checks of a finished file, shared with the GPU test."""
    r = R.riff_walk(data)
    assert len(r["frames"]) == n == len(r["index"])
    avih = struct.unpack("<14I", r["avih"])
    assert avih[4] == n and avih[6] == 1 and (avih[8], avih[9]) == (width, height) and avih[3] & 0x10
    assert avih[0] == round(1e6 * scale / rate) and avih[7] == max(len(f) for _, f in r["frames"])
    strh = struct.unpack("<4s4sIHHIIIIIIIIHHHH", r["strh"])
    assert strh[0] == b"vids" and strh[1] == b"MJPG" and (strh[6], strh[7]) == (scale, rate) and strh[9] == n
    assert strh[10] == avih[7] and strh[-2:] == (width, height)
    strf = struct.unpack("<IiiHH4sIiiII", r["strf"])
    assert strf[:6] == (40, width, height, 1, 24, b"MJPG")
    for (pos, payload), (ckid, flags, off, size) in zip(r["frames"], r["index"]):
        assert ckid == b"00dc" and flags & 0x10 and r["movi_tag"] + off == pos and size == len(payload)
        assert data[pos:pos + 4] == b"00dc" and pos % 2 == 0
        im = Image.open(io.BytesIO(payload))
        im.load()
        assert im.size == (width, height)
    return r


def test_avi_container_layout(tmp_path):
    frames = [_jpeg_bytes(53, 37, 0, odd=1), _jpeg_bytes(53, 37, 1, odd=0), _jpeg_bytes(53, 37, 2, odd=1), _jpeg_bytes(53, 37, 3), _jpeg_bytes(53, 37, 4)]
    path = tmp_path / "v.avi"
    avi = JPG.AviFile(path, 53, 37, 10)
    for f in frames:
        avi.add(f)
    avi.close()
    avi.close()                                                               # (a second close is quiet)
    data = open(path, "rb").read()
    r = check_avi(data, 5, 53, 37, 10, 1)
    assert [f for _, f in r["frames"]] == frames
    pos0, f0 = r["frames"][0]
    assert len(f0) % 2 == 1 and data[pos0 + 8 + len(f0)] == 0 and r["frames"][1][0] == pos0 + 8 + len(f0) + 1      # an odd frame is padded
    assert len(data) == JPG.AviFile.final_bytes(4 + sum(8 + len(f) + (len(f) & 1) for f in frames), 5)
    with pytest.raises(RuntimeError, match="closed"):
        avi.add(frames[0])
    # a fractional rate: 30000 / 1001
    avi = JPG.AviFile(tmp_path / "ntsc.avi", 53, 37, 30000 / 1001)
    avi.add(frames[0])
    avi.close()
    check_avi(open(tmp_path / "ntsc.avi", "rb").read(), 1, 53, 37, 30000, 1001)
    with pytest.raises(ValueError):
        JPG.AviFile(tmp_path / "bad.avi", 53, 37, 0)
    assert not os.path.exists(tmp_path / "bad.avi")


def test_avi_refuses_to_pass_two_gigabytes_on_the_arithmetic(tmp_path):
    avi = JPG.AviFile(tmp_path / "big.avi", 53, 37, 10)
    frame = _jpeg_bytes(53, 37, 0)
    avi.add(frame)
    per = 8 + len(frame) + (len(frame) & 1)
    # pretend the movi list already holds as many bytes as leaves room for exactly one more frame and its index entry
    avi._movi = JPG.AVI_MAX_BYTES - (JPG.AviFile.MOVI_AT + 8 + 8 + 16 * 2) - per
    assert JPG.AviFile.final_bytes(avi._movi + per, 2) == JPG.AVI_MAX_BYTES
    avi._movi += 1
    with pytest.raises(RuntimeError, match="past 2147483647 bytes"):
        avi.add(frame)
    assert avi.frames == 1
    avi._movi -= 1
    avi._fp.close()
    avi._fp = io.BytesIO()                                                    # (the arithmetic, not two gigabytes of disk)
    avi.add(frame)
    assert avi.frames == 2 and JPG.AviFile.final_bytes(avi._movi, 2) == JPG.AVI_MAX_BYTES
    with pytest.raises(RuntimeError, match="past"):
        avi.add(b"")
    avi._fp = None


def test_video_writer_refuses_without_a_device(tmp_path):
    v = JPG.VideoWriter(tmp_path / "v.avi", 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        v.submit(torch.zeros(3, 8, 8))
    v.close()
    assert not os.path.exists(tmp_path / "v.avi") and not [t for t in threading.enumerate() if t.name.startswith("VideoWriter")]
    with pytest.raises(ValueError, match="subsampling"):
        JPG.VideoWriter(tmp_path / "v.avi", 10, subsampling="422")
