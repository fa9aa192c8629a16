"""No GPU: include/gp_jpeg_decode.h against the binding's table; the refusals that need no device; the JPEG decoder's workgroup programs
(csrc/jpeg_decode_core.h) run lane by lane on the CPU (tests/jpeg_decode_emulate.cpp, under the sanitizers where the host compiler
can link them) over every case of tests/jpeg_decode_cases.py, with Pillow's decoder and tests/jpeg_decode_ref.py -- the header's
arithmetic in numpy -- as the oracles for the pixels.  Every comparison is bit-exact."""
import ctypes as C
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import abi_check
import jpeg_cases as J
import jpeg_decode_cases as D
import jpeg_decode_ref as REF
import jpeg_ref as R
from gaussianprediction_amd import _lib, jpeg_decode as JD

_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "gp_stream_t": _lib.Ptr}
_POINTEES = {"void", "uint8_t", "uint32_t", "int64_t", "int32_t", "float"}


def test_prototype_table_equals_the_header():
    protos = abi_check.check_table(JD.ABI, 3, _SCALARS, _POINTEES)
    assert JD.ABI.prototypes is JD.PROTOTYPES and JD.ABI.header == "gp_jpeg_decode.h"
    assert protos["gp_jpeg_decode"][1][-1] == "gp_stream_t"        # the stream is the last parameter


def test_symbols_and_constants():
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_JPEG_DECODE_[A-Z0-9_]+) (\d+)u?\b", abi_check.header_text("gp_jpeg_decode.h"))}
    assert defs["GP_JPEG_DECODE_ABI_VERSION"] == JD.GP_JPEG_DECODE_ABI_VERSION == JD.ABI.version == 1
    abi_check.check_applied(JD.ABI)
    assert (defs["GP_JPEG_DECODE_MAX_BATCH"], defs["GP_JPEG_DECODE_TABLE_BYTES"], defs["GP_JPEG_DECODE_DST_U8"], defs["GP_JPEG_DECODE_DST_F32"]) \
        == (JD.MAX_BATCH, JD.TABLE_BYTES, JD.DST_U8, JD.DST_F32) == (65535, 1232, 0, 1)
    other = {"ABI_VERSION", "MAX_BATCH", "TABLE_BYTES", "DST_U8", "DST_F32"}
    codes = {k[len("GP_JPEG_DECODE_"):]: v for k, v in defs.items() if k[len("GP_JPEG_DECODE_"):] not in other}
    assert codes == {v: k for k, v in JD.STATUS.items()} and len(set(codes.values())) == len(codes) == 10     # every status a code of its own
    for name in ("OK", "TRUNCATED", "NO_CODE", "CATEGORY", "RUN", "TRAILING", "MARKER", "HUFFMAN_TABLE", "TABLE", "BUDGET"):
        assert codes[name] == getattr(D, name), name
    from gaussianprediction_amd import jpeg_ops
    assert (JD.SUB_420, JD.SUB_444) == (jpeg_ops.SUB_420, jpeg_ops.SUB_444) and list(JD.ZIGZAG) == J.ZIGZAG


def test_c_entries_refuse_before_they_look_at_a_pointer():
    l = JD.lib()
    s = l.gp_jpeg_decode_scratch_bytes
    assert s(1, 163, 178, 0, 1) > 0 and s(32, 1014, 1352, 0, 32 * 680) < 1 << 28
    for bad, word in (((0, 4, 4, 0, 1), b"B = 0"), ((65536, 4, 4, 0, 65536), b"B = 65536"), ((1, 0, 4, 0, 1), b"H = 0"), ((1, 4, 0, 1, 1), b"W = 0"),
                      ((1, 4, 65536, 1, 1), b"W = 65536"), ((1, 4, 4, 2, 1), b"subsampling = 2"), ((2, 4, 4, 0, 1), b"nseg = 1"),
                      ((1, 40000, 40000, 1, 1), b"2^31")):
        assert s(*bad) == -1 and word in l.gp_last_error(), bad

    def call(B=1, H=4, W=4, sub=0, kind=0, pay=1, pay_n=16, seg=8, nseg=1, iseg=8, most=1, tab=1, dst=1, stride=48, st=4, scr=256):
        return l.gp_jpeg_decode(B, H, W, sub, kind, pay, pay_n, seg, nseg, iseg, most, tab, dst, stride, st, scr, None)

    for kw, word in ((dict(B=0), b"B = 0"), (dict(sub=3), b"subsampling = 3"), (dict(kind=2), b"dst_kind = 2"), (dict(pay_n=-1), b"payload_bytes"),
                     (dict(most=0), b"max_image_seg = 0"), (dict(most=2), b"max_image_seg = 2"), (dict(stride=47), b"dst_stride"), (dict(pay=None), b"null"),
                     (dict(seg=None), b"null"), (dict(tab=None), b"null"), (dict(st=None), b"null"), (dict(scr=128), b"256-byte"), (dict(seg=4), b"8-byte"),
                     (dict(st=2), b"4-byte"), (dict(kind=1, dst=2), b"float32 dst")):
        assert call(**kw) == 1 and word in l.gp_last_error(), kw          # (nothing was launched: the pointers are not even memory)


# ---- the files ----
@pytest.fixture(scope="module")
def own(tmp_path_factory):
    """own(img [3, H, W] uint8, "420" / "444", quality or (luminance, chrominance), key) -> the file the encoder's workgroup programs
    write on the CPU (tests/jpeg_emulate.cpp)."""
    run = J.build_emulator(tmp_path_factory.mktemp("jpeg_emulate"))
    tables = {}

    def write(img, sub, q, key):
        if isinstance(q, int):
            if q not in tables:
                out = str(run.dir / "tables.bin")
                subprocess.check_call([run.exe, "tables", str(q), out])
                t = list(open(out, "rb").read())
                tables[q] = (t[:64], t[64:])
            q = tables[q]
        return run(img, sub, q, key)

    return write


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    """run(items, dtype, guard, mangle, most) -> (images [3, H, W] numpy, status), under the sanitizers."""
    return D.build_emulator(tmp_path_factory.mktemp("jpeg_decode_emulate"), sanitize=True)


def test_parse_walks_the_markers_and_refuses_on_the_host(own):
    c = own(J.textured(144, 130, 4), "420", 90, "wrap-144x130-420")
    it = JD.parse(c, "a.jpg")
    info = R.walk(c)
    assert (it.H, it.W, it.sub, it.nmcu, it.interval, it.nseg) == (144, 130, JD.SUB_420, 81, 8, 11) and len(it.tables) == JD.TABLE_BYTES
    assert JD.pieces(it) == D.split(c)[1] and len(info["segments"]) == 11
    assert list(it.tables[16:80]) == info["dqt"][0] and list(it.tables[80:144]) == info["dqt"][1] and list(it.tables[:9]) == [0, 1, 1, 0, 1, 1, 0, 1, 1]
    p = D.pillow_file(J.textured(17, 33, 5), quality=90, subsampling=0)
    it = JD.parse(p)
    assert (it.sub, it.nmcu, it.interval, it.nseg) == (JD.SUB_444, 15, 15, 1)
    for name, data, why in D.refused(own):
        with pytest.raises(ValueError, match=r"jpeg_decode: f\.jpg: .*" + re.escape(why)):
            JD.parse(data, "f.jpg")


def test_checked_before_the_device_and_before_any_launch(monkeypatch, tmp_path, own):
    monkeypatch.setattr(JD, "lib", lambda: pytest.fail("a launch was reached"))
    monkeypatch.setattr(torch.Tensor, "to", lambda *a, **k: pytest.fail("the device was reached"))
    good = D.pillow_file(J.textured(8, 8, 1))
    for call in (lambda: JD.decode([good], device="cpu"), lambda: JD.decode([good], device=torch.device("cpu"), dtype=torch.float32),
                 lambda: JD.decode_files([tmp_path / "never-read.jpg"], device="cpu"), lambda: JD.decode_avi(tmp_path / "never-read.avi", device="cpu")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(RuntimeError, match="dtype must be"):
        JD.decode([good], device="cuda:0", dtype=torch.float16)
    with pytest.raises(ValueError, match=r"x\.jpg: progressive"):
        JD.decode([good, D.pillow_file(J.textured(8, 8, 1), progressive=True)], device="cuda:0", names=["g.jpg", "x.jpg"])
    (tmp_path / "p.jpg").write_bytes(D.pillow_file(J.textured(8, 8, 1), subsampling=1))
    with pytest.raises(ValueError, match=r"p\.jpg: sampling factors"):
        JD.decode_files([tmp_path / "p.jpg"], device="cuda:0")
    items = [JD.parse(good), JD.parse(D.pillow_file(J.textured(8, 8, 2), subsampling=0)), JD.parse(good)]
    assert JD.groups(items) == [((8, 8, JD.SUB_420), [0, 2]), ((8, 8, JD.SUB_444), [1])]


def _check(emulator, cases):
    items = [JD.parse(c.file, c.name) for c in cases]
    images, status = emulator(items)
    floats, _ = emulator(items, dtype=np.float32)
    stats = {}
    for c, img, f, s in zip(cases, images, floats, status):
        assert s == 0, (c.name, s, JD.STATUS.get(s))
        want = D.pillow_pixels(c.file)
        ref, stats[c.name] = REF.pixels(c.file)
        assert img.dtype == np.uint8 and np.array_equal(img, ref.transpose(2, 0, 1)), c.name        # the header's arithmetic
        assert np.array_equal(img, want.transpose(2, 0, 1)), c.name                                  # Pillow's decoder
        unit = (torch.from_numpy(img.copy()).to(torch.float32) / 255.0).numpy()                      # what metrics._load_rgb computes
        assert f.dtype == np.float32 and np.array_equal(f.view(np.uint32), unit.view(np.uint32)), c.name
    return stats


KINDS = {"textured": "-textured-", "rows-and-wrap": ("-rows-", "-wrap-"), "narrow": "-narrow-", "noise-and-saturated": ("-noise-", "-saturated-"),
         "constant": "-constant-", "lanes": "-lanes-", "zrl": "-zrl-", "optimize-and-appn": ("-optimize-", "-com-appn-")}


@pytest.fixture(scope="module")
def well(own):
    return D.wellformed(own)


def test_every_case_has_one_kind(well):
    names = [c.name for c in well]
    assert len(set(names)) == len(names)
    for n in names:
        assert sum(any(k in n for k in (v if isinstance(v, tuple) else (v,))) for v in KINDS.values()) == 1, n


@pytest.mark.parametrize("kind", list(KINDS))
def test_emulated_decoder_against_the_reference_and_pillow(emulator, well, kind):
    keys = KINDS[kind] if isinstance(KINDS[kind], tuple) else (KINDS[kind],)
    cases = [c for c in well if any(k in c.name for k in keys)]
    assert cases
    stats = _check(emulator, cases)
    if kind == "zrl":
        assert all(s["zrl"] >= 9 for n, s in stats.items() if n.startswith("own-")) and sum(s["zrl"] >= 9 for s in stats.values()) >= 2
    if kind == "noise-and-saturated":
        q100 = stats["own-noise-q100-48x48-444"]
        assert q100["no_eob"] > 0 and q100["max_ac_cat"] == 10 and stats["own-noise-checkerboard-q100-444"]["max_dc_cat"] == 11
        assert any(b"\xff\x00" in c.file[700:] for c in cases)                                      # stuffing
    if kind == "lanes":
        assert sorted(JD.parse(c.file).nseg for c in cases) == [72, 575]
    if kind == "optimize-and-appn":
        assert any(max(l for l, _ in R.walk(REF.strip(c.file))["dht_tables"][0x10]) == 16 for c in cases)     # a code of 16 bits
        assert b"a comment" in cases[-1].file and b"Exif" in cases[-1].file


def test_emulated_batch_is_its_single_images(emulator, well):
    cases = [c for c in well if "-45x67-" in c.name or "-17x33-" in c.name][:8]
    items = [JD.parse(c.file) for c in cases]
    together, status = emulator(items)
    assert status == [0] * len(items)
    for it, img in zip(items, together):
        (alone,), (s,) = emulator([it])
        assert s == 0 and np.array_equal(alone, img), it.name


@pytest.fixture(scope="module")
def bad(own):
    return D.malformed(own)


@pytest.mark.parametrize("name", ["interval-cut-short", "no-code-matches", "run-past-63", "extra-byte-before-rst", "ff-01-inside", "oversubscribed-dht"])
def test_emulated_decoder_refuses_with_the_status(emulator, bad, name):
    """Between two good images of its shape; under the sanitizers, so a read or write outside a buffer fails the run."""
    c = next(c for c in bad if c.name == name)
    items = [JD.parse(f, n) for f, n in zip((c.goods[0], c.file, c.goods[1]), ("a", name, "b"))]
    images, status = emulator(items)
    assert status == [0, c.status, 0], (status, JD.STATUS.get(status[1]))
    for k in (0, 2):
        (alone,), _ = emulator([items[k]])
        assert np.array_equal(images[k], alone) and np.array_equal(alone, D.pillow_pixels(c.goods[k // 2]).transpose(2, 0, 1))


def test_categories_beyond_the_baseline_and_bad_segment_tables(emulator, own):
    """A Huffman table whose symbols name categories no baseline stream has, and segment tables that do not tile the image or leave the
    payload: a status each, never an access."""
    good = own(D.noise(40, 88, 22), "444", 90, "good-22")
    it = JD.parse(good)
    for tab, at in ((0, 144 + 16), (2, 144 + 2 * 272 + 16)):                       # DC 0: every category 12; AC 0: every (run, category) x 11
        t = bytearray(it.tables)
        for k in range(256):
            t[at + k] = 12 if tab == 0 else (t[at + k] & 0xf0) | 11
        other = JD.parse(good)
        other.tables = bytes(t)
        _, status = emulator([it, other, it])
        assert status == [0, D.CATEGORY, 0], (tab, status)
    seven = it.nseg
    assert seven == 7
    for mangle in (lambda seg: [seg[1], seg[0]] + seg[2:], lambda seg: [seg[0], seg[1][:1] + (1 << 41,) + seg[1][2:]] + seg[2:],
                   lambda seg: [(7,) + seg[0][1:]] + seg[1:], lambda seg: seg[:6] + [seg[6][:4] + (8,)], lambda seg: seg[:6] + [seg[6][:3] + (1 << 33, 7)],
                   lambda seg: [seg[0][:2] + (-5,) + seg[0][3:]] + seg[1:], lambda seg: [seg[0][:3] + (1, 8)] + seg[1:]):
        _, status = emulator([it], mangle=mangle)
        assert status == [D.TABLE]
    _, status = emulator([it], most=6)                                           # more segments than max_image_seg says
    assert status == [D.TABLE]


def test_avi_walk_against_a_file_written_by_avifile(tmp_path, own):
    from gaussianprediction_amd import jpeg_ops
    frames = [own(J.textured(24, 40, s), "420", 90, f"avi-{s}") for s in range(5)]
    path = tmp_path / "v.avi"
    avi = jpeg_ops.AviFile(path, 40, 24, 30)
    for f in frames:
        avi.add(f)
    avi.close()
    data = path.read_bytes()
    w, h, got = JD.avi_frames(data, "v.avi")
    assert (w, h) == (40, 24) and [bytes(g) for g in got] == frames == [f for _, f in R.riff_walk(data)["frames"]]
    assert any(len(f) & 1 for f in frames)                                       # a padded chunk among them
    for broken, why in ((b"RIFX" + data[4:], "not a RIFF"), (data.replace(b"MJPG", b"H264"), "not MJPG"), (data.replace(b"00dc", b"01dc", 1), "not one compressed video stream"),
                        (data[:-16] + struct.pack("<4sIII", b"00dc", 16, 4, 1), "idx1 does not list"), (data.replace(b"strh", b"strx"), "stream(s)")):
        with pytest.raises(ValueError, match=r"jpeg_decode: v\.avi: .*" + re.escape(why)):
            JD.avi_frames(broken, "v.avi")
