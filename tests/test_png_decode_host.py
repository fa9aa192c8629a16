"""No GPU: include/gp_png_decode.h against the binding's table; the refusals that need no device; the PNG decoder's workgroup programs
(csrc/png_decode_core.h) run lane by lane on the CPU (tests/png_decode_emulate.cpp, under the sanitizers where the host compiler
can link them) over every case of tests/png_decode_cases.py, with Pillow's decoder as the oracle for the pixels and zlib's
for what a well-formed and a malformed stream is.  Every comparison is bit-exact."""
import ctypes as C
import io
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest
import torch

import abi_check
import decode_stage_cases as SC
import emulate_build
import png_cases as P
import png_decode_cases as D
from gaussianprediction_amd import _lib, png_decode as PD

_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "gp_stream_t": _lib.Ptr}
_POINTEES = {"void", "uint8_t", "uint32_t", "int64_t", "int32_t", "float"}


def test_prototype_table_equals_the_header():
    protos = abi_check.check_table(PD.ABI, 3, _SCALARS, _POINTEES)
    assert PD.ABI.prototypes is PD.PROTOTYPES and PD.ABI.header == "gp_png_decode.h"
    assert protos["gp_png_decode"][1][-1] == "gp_stream_t"         # the stream is the last parameter


def test_symbols_and_constants():
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_PNG_DECODE_[A-Z0-9_]+) (\d+)u?\b", abi_check.header_text("gp_png_decode.h"))}
    assert defs["GP_PNG_DECODE_ABI_VERSION"] == PD.GP_PNG_DECODE_ABI_VERSION == PD.ABI.version == 1
    abi_check.check_applied(PD.ABI)
    assert (defs["GP_PNG_DECODE_MAX_BATCH"], defs["GP_PNG_DECODE_DST_U8"], defs["GP_PNG_DECODE_DST_F32"], defs["GP_PNG_DECODE_MODE_SERIAL"],
            defs["GP_PNG_DECODE_MODE_BANDED"]) == (PD.MAX_BATCH, PD.DST_U8, PD.DST_F32, PD.MODE_SERIAL, PD.MODE_BANDED) == (65535, 0, 1, D.SERIAL, D.BANDED)
    other = {"ABI_VERSION", "MAX_BATCH", "DST_U8", "DST_F32", "MODE_SERIAL", "MODE_BANDED"}
    codes = {k[len("GP_PNG_DECODE_"):]: v for k, v in defs.items() if k[len("GP_PNG_DECODE_"):] not in other}
    assert codes == {v: k for k, v in PD.STATUS.items()} and len(set(codes.values())) == len(codes)     # every status a code of its own
    for name in ("TRUNCATED", "BLOCK_TYPE", "STORED_LEN", "TOO_MANY_CODES", "CLEN_CODE", "REPEAT_FIRST", "REPEAT_OVERRUN", "LIT_OVERSUBSCRIBED",
                 "LIT_INCOMPLETE", "NO_END_OF_BLOCK", "LIT_SYMBOL", "DIST_SYMBOL", "DIST_TOO_FAR", "OUTPUT_LONG", "OUTPUT_SHORT", "ADLER", "FILTER",
                 "ZLIB_METHOD", "ZLIB_FDICT", "ZLIB_FCHECK", "ZLIB_WINDOW", "DIST_CODE", "NOT_BANDED"):
        assert codes[name] == getattr(D, name), name
    from gaussianprediction_amd import png_ops
    assert PD.BAND_BYTES == png_ops.BAND_BYTES == D.BAND


def test_c_entries_refuse_before_they_look_at_a_pointer():
    l = PD.lib()
    s = l.gp_png_decode_scratch_bytes
    assert s(1, 163, 178, 3, 1) > 0 and s(32, 1014, 1352, 3, 32 * 251) < 1 << 28
    for bad, word in (((0, 4, 4, 3, 1), b"B = 0"), ((65536, 4, 4, 3, 65536), b"B = 65536"), ((1, 0, 4, 3, 1), b"H = 0"), ((1, 4, 0, 3, 1), b"W = 0"),
                      ((1, 4, 4, 5, 1), b"C = 5"), ((1, 4, 4, 0, 1), b"C = 0"), ((2, 4, 4, 3, 1), b"nseg = 1"), ((1, 46341, 15447, 3, 1), b"2^31"),
                      ((1, 65536, 4, 3, 1), b"H = 65536")):
        assert s(*bad) == -1 and word in l.gp_last_error(), bad

    def call(B=1, H=4, W=4, Cn=3, c_out=3, kind=0, pay=1, pay_n=16, seg=8, nseg=1, iseg=8, bg=None, dst=1, stride=48, st=4, mo=4, scr=256):
        return l.gp_png_decode(B, H, W, Cn, c_out, kind, pay, pay_n, seg, nseg, iseg, bg, dst, stride, st, mo, scr, None)

    for kw, word in ((dict(B=0), b"B = 0"), (dict(c_out=4), b"C_out = 4"), (dict(c_out=0), b"C_out = 0"), (dict(kind=2), b"dst_kind = 2"),
                     (dict(bg=4), b"background needs"), (dict(Cn=4, c_out=4, bg=4, stride=64), b"background needs"), (dict(pay_n=-1), b"payload_bytes"),
                     (dict(stride=47), b"dst_stride"), (dict(pay=None), b"null"), (dict(seg=None), b"null"), (dict(st=None), b"null"),
                     (dict(scr=128), b"256-byte"), (dict(seg=4), b"8-byte"), (dict(mo=2), b"4-byte"), (dict(kind=1, dst=2), b"float32 dst")):
        assert call(**kw) == 1 and word in l.gp_last_error(), kw          # (nothing was launched: the pointers are not even memory)


def _png(H=4, W=4, Cn=3, **kw):
    img = D.noise(H, W, Cn, 1)
    payload = zlib.compress(D.filtered(img, [0] * H))
    return D.png_file(H, W, Cn, [payload], **kw)


def test_parse_walks_the_chunks_and_refuses_on_the_host():
    it = PD.parse(_png(), "a.png")
    assert (it.H, it.W, it.C, it.S, len(it.pieces), it.banded) == (4, 4, 3, 52, 1, False)
    c = D.wellformed()[-1]
    it = PD.parse(c.file)
    assert len(it.pieces) == 2 and it.banded and b"".join(bytes(p) for p in it.pieces) == c.payload
    good = _png()
    text = D.chunk(b"tEXt", b"k\0v")
    for data, why in ((_png(depth=16), "bit depth 16"), (_png(Cn=1, depth=4), "bit depth 4"), (_png(Cn=1, depth=1), "bit depth 1"),
                      (_png(colour=3), "palette"), (_png(interlace=1), "interlaced"), (D.png_file(4, 4, 3, []), "no IDAT"),
                      (b"\x89PNX" + good[4:], "signature"), (good[:40] + bytes([good[40] ^ 1]) + good[41:], "CRC-32"),
                      (good[:-12], "no IEND"), (good[:-5], "past the end"), (good[:33] + struct.pack(">I", 1 << 20) + good[37:], "past the end"),
                      (good[:8] + good[33:], "not IHDR"), (_png(colour=5), "colour type 5"),
                      (D.png_file(4, 4, 3, [b"ab"])[:-12] + text + D.chunk(b"IDAT", b"cd") + D.chunk(b"IEND", b""), "not consecutive")):
        with pytest.raises(ValueError, match=r"png_decode: f\.png: .*" + re.escape(why)):
            PD.parse(data, "f.png")


def test_checked_before_the_device_and_before_any_launch(monkeypatch, tmp_path):
    monkeypatch.setattr(PD, "lib", lambda: pytest.fail("a launch was reached"))
    monkeypatch.setattr(torch.Tensor, "to", lambda *a, **k: pytest.fail("the device was reached"))
    good = _png()
    for call in (lambda: PD.decode([good], device="cpu"), lambda: PD.decode([good], device=torch.device("cpu"), dtype=torch.float32),
                 lambda: PD.decode_files([tmp_path / "never-read.png"], device="cpu")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(RuntimeError, match="dtype must be"):
        PD.decode([good], device="cuda:0", dtype=torch.float16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PD.decode([good], device="cuda:0", background=torch.zeros(3))
    with pytest.raises(RuntimeError, match="three floats"):
        PD.decode([good], device="cuda:0", background=[0, 0, 0])
    with pytest.raises(ValueError, match="x.png: bit depth 16"):
        PD.decode([good, _png(depth=16)], device="cuda:0", names=["g.png", "x.png"])
    (tmp_path / "p.png").write_bytes(_png(colour=3))
    with pytest.raises(ValueError, match=r"p\.png: palette"):
        PD.decode_files([tmp_path / "p.png"], device="cuda:0")
    items = [PD.parse(good), PD.parse(_png(Cn=4))]
    assert [(s, c, i) for s, c, i in PD.groups(items, channels=3)] == [((4, 4, 3), 3, [0]), ((4, 4, 4), 3, [1])]
    assert PD.groups(items[:1] * 2 + items[1:], channels=None)[0][2] == [0, 1]
    with pytest.raises(ValueError, match="background composites RGBA"):
        PD.groups(items, background=torch.zeros(3))
    with pytest.raises(ValueError, match="channels = 4"):
        PD.groups(items[1:], channels=4, background=torch.zeros(3))


# ---- the workgroup programs on the CPU ----
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    """run(items, banded, dtype, channels, bg, guard) -> (images [C_out, H, W] numpy, status, modes), one process per shape group."""
    d = tmp_path_factory.mktemp("png_decode_emulate")
    exe = emulate_build.build("png_decode_emulate", d, sanitize=True)

    def run(items, banded, dtype=np.uint8, channels=None, bg=None, guard=8, mangle=None):
        images, status, modes = [None] * len(items), [0] * len(items), [0] * len(items)
        shapes = PD.groups(items, channels, None if bg is None else torch.tensor(bg))
        plans = PD.plans(items, banded, shapes)
        host = SC.filled(plans)                                              # (staged as the device path stages: all groups in one array)
        for ((H, W, Cn), c_out, idx), pl in zip(shapes, plans):
            seg, image_seg, _, payload = SC.sections(host, pl)
            seg = seg if mangle is None else np.array(mangle(list(pl.seg)), dtype=np.int64).tobytes()
            job, out = str(d / "job.bin"), str(d / "out.bin")
            with open(job, "wb") as fp:
                fp.write(struct.pack("<9i3fq", len(idx), H, W, Cn, c_out, 0 if dtype == np.uint8 else 1, bg is not None, len(seg) // 40, guard,
                                     *(bg if bg is not None else (0, 0, 0)), pl.bytes))
                fp.write(seg + image_seg + payload)
            subprocess.check_call([exe, job, out], timeout=120)          # (a loop that does not end is a failure here, not a hang)
            raw = open(out, "rb").read()
            B, n = len(idx), c_out * H * W
            words = np.frombuffer(raw[:8 * B], dtype=np.uint32).reshape(2, B)
            slots = np.frombuffer(raw[8 * B:], dtype=dtype).reshape(B, n + guard)
            assert (slots[:, n:].view(np.uint8) == 0xA5).all()          # the guard behind every slot
            for b, i in enumerate(idx):
                status[i], modes[i] = int(words[0, b]), int(words[1, b])
                images[i] = slots[b, :n].reshape(c_out, H, W) if status[i] == 0 else None
                assert status[i] == 0 or (slots[b].view(np.uint8) == 0xA5).all()      # a refused image leaves its slot alone
        return images, status, modes

    return run


def _decode(run, files, **kw):
    """png_decode.decode's two passes, through the emulator: banded where the chunk count says so, NOT_BANDED images again serially."""
    items = [PD.parse(f, f"<{k}>") for k, f in enumerate(files)]
    banded = [it.banded for it in items]
    images, status, modes = run(items, banded, **kw)
    again = [i for i, s in enumerate(status) if s == D.NOT_BANDED and banded[i]]
    if again:
        im2, st2, mo2 = run([items[i] for i in again], [False] * len(again), **kw)
        for k, i in enumerate(again):
            images[i], status[i], modes[i] = im2[k], st2[k], mo2[k]
    return images, status, modes, banded


def _pillow(data):
    from PIL import Image
    arr = np.array(Image.open(io.BytesIO(data)))
    return arr[:, :, None] if arr.ndim == 2 else arr


def _check(cases, images, status, modes):
    for c, img, s, m in zip(cases, images, status, modes):
        assert s == 0, (c.name, s, PD.STATUS.get(s))
        want = _pillow(c.file)
        assert np.array_equal(want, c.want), c.name
        assert img.dtype == np.uint8 and np.array_equal(img, want.transpose(2, 0, 1)), c.name
        assert m == c.mode, (c.name, m)


WELL = D.wellformed()
KINDS = {"filters": "filters-", "rows-and-widths": ("rows-", "width-"), "zlib": ("zlib-", "window-"), "by-hand": ("fixed-", "dynamic-"),
         "foreign": "foreign-"}


@pytest.mark.parametrize("kind", list(KINDS))
def test_emulated_decoder_against_pillow(emulator, kind):
    cases = [c for c in WELL if c.name.startswith(KINDS[kind])]
    assert cases
    for c in cases:
        assert len(zlib.decompress(c.payload)) == c.want.shape[0] * (1 + c.want.shape[1] * c.want.shape[2]), c.name      # zlib accepts it
    images, status, modes, banded = _decode(emulator, [c.file for c in cases])
    _check(cases, images, status, modes)
    if kind == "foreign":
        assert all(banded)                                                         # all three were tried banded; one of them is
        sync, full, _ = (PD.parse(c.file).pieces for c in cases)
        for pieces, alone in ((sync, False), (full, True)):                        # ... and zlib agrees about each second chunk
            try:
                zlib.decompressobj(-15).decompress(bytes(pieces[1]))
                assert alone
            except zlib.error:
                assert not alone


def test_emulated_decoder_on_pillows_files(emulator):
    cases = D.pillow_cases()
    for c in cases:
        assert len(PD.parse(c.file).pieces) >= 1
    _check(cases, *_decode(emulator, [c.file for c in cases])[:3])


def test_emulated_decoder_on_this_projects_files(emulator, tmp_path):
    """The encoder's workgroup programs write the files (tests/png_emulate.cpp): every one with more than one band must decode BANDED
    -- the serial pass behind decode() would otherwise hide a broken fast path."""
    encode = P.build_emulator(tmp_path)
    cases = [D.own_case(name, encode(img, fnone), img) for name, img, fnone in D.own_inputs()]
    assert sum(c.mode == D.BANDED for c in cases) >= 5
    items = [PD.parse(c.file) for c in cases]
    images, status, modes = emulator(items, [it.banded for it in items])          # ONE pass: no serial pass behind it
    _check(cases, images, status, modes)
    for it in items:                                                               # every chunk inflates on its own, as the issue checked
        for k, piece in enumerate(it.pieces):
            body = bytes(piece)[2:] if k == 0 else bytes(piece)
            n = len(zlib.decompressobj(-15).decompress(body))
            assert n == min(D.BAND, it.S - k * D.BAND), (it.name, k, n)


def test_emulated_float_output_and_channel_subsets(emulator):
    cases = [c for c in WELL if c.name.startswith("filters-37x45")]
    files = [c.file for c in cases]
    as_float, status, _, _ = _decode(emulator, files, dtype=np.float32)
    first, _, _, _ = _decode(emulator, files, channels=1)
    three, _, _, _ = _decode(emulator, files, dtype=np.float32, channels=3)
    for c, f, one, t in zip(cases, as_float, first, three):
        u8 = torch.from_numpy(c.want.transpose(2, 0, 1).copy())
        want = (u8.to(torch.float32) / 255.0).numpy()                              # what metrics._load_rgb and PILtoTorch compute
        assert f.dtype == np.float32 and np.array_equal(f.view(np.uint32), want.view(np.uint32)), c.name
        assert np.array_equal(one, c.want.transpose(2, 0, 1)[:1]), c.name
        assert np.array_equal(t.view(np.uint32), want[:3].view(np.uint32)), c.name
    assert np.array_equal(np.arange(256, dtype=np.float32) / np.float32(255), (torch.arange(256, dtype=torch.uint8).to(torch.float32) / 255.0).numpy())


@pytest.mark.parametrize("bg", [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0)])
def test_emulated_composite_against_the_readers_formula(emulator, bg):
    c = D.composite_case()
    want = D.composite_reference(c.want, bg)                                       # [REF scene/dataset_readers.py:214-218]
    (u8,), status, _, _ = _decode(emulator, [c.file], bg=bg)
    (f32,), _, _, _ = _decode(emulator, [c.file], bg=bg, dtype=np.float32)
    assert status == [0] and np.array_equal(u8, want.transpose(2, 0, 1))
    assert np.array_equal(f32.view(np.uint32), (torch.from_numpy(want.transpose(2, 0, 1).copy()).to(torch.float32) / 255.0).numpy().view(np.uint32))
    assert len(np.unique(c.want[:, :, [0, 3]].reshape(-1, 2), axis=0)) == 65536    # every (value, alpha) pair


BAD = D.malformed()


@pytest.mark.parametrize("name", [c.name for c in BAD])
def test_emulated_decoder_refuses_with_the_status(emulator, name):
    """Between two good images of its shape; under the sanitizers, so a read or write outside a buffer fails the run."""
    c = next(c for c in BAD if c.name == name)
    try:
        zlib.decompress(c.payload)
        assert not c.deflate_is_bad, "zlib accepts this stream"
    except zlib.error:
        assert c.deflate_is_bad, "zlib refuses this stream"
    a, b = D.good_small(1), D.good_small(2)
    images, status, modes, _ = _decode(emulator, [a.file, c.file, b.file])
    assert status == [0, c.status, 0], (status, PD.STATUS.get(status[1]))
    assert modes == [D.SERIAL] * 3
    assert np.array_equal(images[0], a.want.transpose(2, 0, 1)) and np.array_equal(images[2], b.want.transpose(2, 0, 1)) and images[1] is None


def test_a_damaged_band_of_this_projects_kind_comes_back_not_banded(emulator):
    """Two chunks of which the second is cut: the banded pass says NOT_BANDED, the serial pass names the fault."""
    c = next(c for c in WELL if c.name == "foreign-full-flush")
    it = PD.parse(c.file)
    bad = PD.parse(D.png_file(60, 120, 3, [bytes(it.pieces[0]), bytes(it.pieces[1])[:-3]]))
    assert bad.banded
    _, status, modes = emulator([it, bad], [True, True])
    assert status == [0, D.NOT_BANDED] and modes == [D.BANDED, D.BANDED]
    _, status, modes, _ = _decode(emulator, [c.file, D.png_file(60, 120, 3, [bytes(it.pieces[0]), bytes(it.pieces[1])[:-3]])])
    assert status == [0, D.TRUNCATED] and modes == [D.BANDED, D.SERIAL]
    # a table that does not tile the image or leaves the payload is a status too, never an access
    for mangle in (lambda seg: [seg[1], seg[0]], lambda seg: [seg[0], seg[1][:2] + (1 << 33,) + seg[1][3:]], lambda seg: [seg[0], (7,) + seg[1][1:]],
                   lambda seg: [seg[0], seg[1][:3] + (D.BAND + 1, seg[1][4])], lambda seg: [seg[0], seg[1][:4] + (1 << 31,)],
                   lambda seg: [seg[0], seg[1][:1] + (-5,) + seg[1][2:]]):
        _, status, _ = emulator([it], [True], mangle=mangle)
        assert status == [25]


def test_the_cases_are_what_they_claim():
    names = [c.name for c in WELL]
    assert len(set(names)) == len(names)
    far = next(c for c in WELL if c.name == "fixed-258-at-32768")
    stream = zlib.decompress(far.payload)
    assert stream[32768:32768 + 258] == stream[:258] and len(stream) == 32768 + 258 + 10
    level0 = next(c for c in WELL if c.name == "zlib-level0-300x400")
    assert len(level0.payload) > 360300 and level0.payload[2] == 0 and level0.payload[3:5] == b"\xff\xff"     # stored blocks of 65 535
    assert next(c for c in WELL if c.name == "window-256").payload[:2] == b"\x08\x1d"
    for c in D.pillow_cases():
        stream = zlib.decompress(b"".join(bytes(p) for p in PD.parse(c.file).pieces))
        types = np.frombuffer(stream, dtype=np.uint8).reshape(300, -1)[:, 0]
        assert len(stream) > 3 * 32768 and (types == 4).sum() >= 100, (c.name, np.bincount(types))      # past the window; mostly Paeth
    assert P.unfilter(D.filtered(D.noise(9, 7, 3, 1), D.cycling(9, 3)), 9, 7).tobytes() == D.noise(9, 7, 3, 1).tobytes()
