"""No GPU: include/gp_jpeg_sync.h against the binding's table; the self-synchronising entropy stage's workgroup programs
(csrc/jpeg_sync_core.h) run lane by lane on the CPU (tests/jpeg_sync_emulate.cpp, a program of its own under
the sanitizers where the host compiler can link them) over every case of tests/jpeg_sync_cases.py.  The oracles: Pillow's
decoder and tests/jpeg_decode_ref.py for the pixels, tests/jpeg_sync_ref.py -- the header's rule in Python -- for the info words.
Every comparison is bit-exact, and no well-formed case may come back SERIAL."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest
import torch

import abi_check
import jpeg_decode_cases as D
import jpeg_decode_ref as REF
import jpeg_sync_cases as SC
from gaussianprediction_amd import _lib, jpeg_decode as JD, jpeg_sync as JS

_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "gp_stream_t": _lib.Ptr}
_POINTEES = {"void", "uint8_t", "uint32_t", "int64_t", "int32_t", "float"}


def test_prototype_table_equals_the_header():
    protos = abi_check.check_table(JS.ABI, 3, _SCALARS, _POINTEES)
    assert JS.ABI.prototypes is JS.PROTOTYPES and JS.ABI.header == "gp_jpeg_sync.h"
    assert protos["gp_jpeg_sync_decode"][1][-1] == "gp_stream_t"         # the stream is the last parameter
    # gp_jpeg_decode's arguments, and info in front of the scratch
    assert [c for c in JS.PROTOTYPES["gp_jpeg_sync_decode"][1]] == JD.PROTOTYPES["gp_jpeg_decode"][1][:15] + [_lib.Ptr] + JD.PROTOTYPES["gp_jpeg_decode"][1][15:]


def test_symbols_and_constants():
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_JPEG_SYNC_[A-Z0-9_]+) (\d+)u?\b", abi_check.header_text("gp_jpeg_sync.h"))}
    assert defs["GP_JPEG_SYNC_ABI_VERSION"] == JS.GP_JPEG_SYNC_ABI_VERSION == JS.ABI.version == 1
    assert (defs["GP_JPEG_SYNC_SUBSEQ_BYTES"], defs["GP_JPEG_SYNC_CHUNK"]) == (JS.S, JS.C)
    codes = {k[len("GP_JPEG_SYNC_"):]: v for k, v in defs.items() if k[len("GP_JPEG_SYNC_"):] not in ("ABI_VERSION", "SUBSEQ_BYTES", "CHUNK")}
    assert codes == {v: k for k, v in JS.STATUS.items()} == {"OK": SC.OK, "SERIAL": SC.SERIAL}
    assert JS.MIN_BYTES >= 2 * JS.S and JS.MIN_BYTES % JS.S == 0
    abi_check.check_applied(JS.ABI)


def test_c_entries_refuse_before_they_look_at_a_pointer():
    l = JS.lib()
    s = l.gp_jpeg_sync_scratch_bytes
    assert s(1, 163, 178, 0, 4000) > 0 and s(32, 1014, 1352, 0, 32 * 600000) < 1 << 29
    for bad, word in (((0, 4, 4, 0, 1), b"B = 0"), ((1, 0, 4, 0, 1), b"H = 0"), ((1, 4, 65536, 1, 1), b"W = 65536"), ((1, 4, 4, 2, 1), b"subsampling = 2"),
                      ((1, 4, 4, 0, -1), b"payload_bytes"), ((1, 4, 4, 0, 1 << 37), b"payload_bytes"), ((1, 40000, 40000, 1, 1), b"2^31")):
        assert s(*bad) == -1 and word in l.gp_last_error(), bad

    def call(B=1, H=4, W=4, sub=0, kind=0, pay=1, pay_n=16, seg=8, nseg=1, iseg=8, most=1, tab=1, dst=1, stride=48, st=4, info=4, scr=256):
        return l.gp_jpeg_sync_decode(B, H, W, sub, kind, pay, pay_n, seg, nseg, iseg, most, tab, dst, stride, st, info, scr, None)

    for kw, word in ((dict(B=0), b"B = 0"), (dict(sub=3), b"subsampling = 3"), (dict(kind=2), b"dst_kind = 2"), (dict(pay_n=-1), b"payload_bytes"),
                     (dict(nseg=2), b"nseg = 2 is not B = 1"), (dict(most=2), b"max_image_seg = 2"), (dict(stride=47), b"dst_stride"), (dict(pay=None), b"null"),
                     (dict(info=None), b"null"), (dict(scr=128), b"256-byte"), (dict(seg=4), b"8-byte"), (dict(info=2), b"4-byte"),
                     (dict(kind=1, dst=2), b"float32 dst")):
        assert call(**kw) == 1 and word in l.gp_last_error(), kw          # (nothing was launched: the pointers are not even memory)


def test_eligible_is_one_segment_and_a_scan_of_some_length():
    long = JD.parse(D.pillow_file(D.noise(40, 88, 1), quality=90, subsampling=0))
    short = JD.parse(D.pillow_file(D.noise(8, 8, 1), quality=90, subsampling=0))
    marked = JD.parse(D.pillow_file(D.noise(40, 88, 1), quality=90, subsampling=0, restart_marker_blocks=8))
    assert len(long.scan) >= JS.MIN_BYTES > len(short.scan) and marked.nseg > 1
    assert [JS.eligible(it) for it in (long, short, marked)] == [True, False, False]


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return SC.build_emulator(tmp_path_factory.mktemp("jpeg_sync_emulate"), sanitize=True)


@pytest.fixture(scope="module")
def one_lane(tmp_path_factory):
    """run(item) -> (image, the GP_JPEG_DECODE_* word): csrc/jpeg_decode_core.h's one-lane program on the same single segment."""
    decode = D.build_emulator(tmp_path_factory.mktemp("jpeg_decode_emulate"), sanitize=False)

    def run(item):
        (image,), (word,) = decode([item], guard=0)
        return image, word

    return run


@pytest.fixture(scope="module")
def well():
    return SC.wellformed(JS.S, JS.C)


KINDS = ["short-", "length", "rounds-", "chunks-", "periodic-white-512", "periodic-white-2048", "partial-", "narrow-", "tables-", "disc-", "natural-"]


def test_every_case_has_one_kind(well):
    names = [c.name for c in well]
    assert len(set(names)) == len(names)
    for n in names:
        assert sum(n.startswith(k) for k in KINDS) == 1, n


@pytest.mark.parametrize("kind", KINDS)
def test_emulated_stage_against_the_references_and_pillow(emulator, well, kind):
    cases = [c for c in well if c.name.startswith(kind)]
    assert cases
    items = [JD.parse(c.file, c.name) for c in cases]
    images, status, info = emulator(items)
    floats, fstatus, _ = emulator(items, dtype=np.float32)
    for c, img, f, s, words in zip(cases, images, floats, status, info):
        assert s == SC.OK, (c.name, s)                                     # a condition, not a tolerance: never SERIAL on a well-formed file
        assert words == c.ref.info, (c.name, words, c.ref.info)            # the header's rule restated
        ref, _ = REF.pixels(c.file)
        assert img.dtype == np.uint8 and np.array_equal(img, ref.transpose(2, 0, 1)), c.name         # the header's arithmetic
        assert np.array_equal(img, D.pillow_pixels(c.file).transpose(2, 0, 1)), c.name                # Pillow's decoder
        unit = (torch.from_numpy(img.copy()).to(torch.float32) / 255.0).numpy()
        assert f.dtype == np.float32 and np.array_equal(f.view(np.uint32), unit.view(np.uint32)), c.name
    assert fstatus == status


def test_emulated_batch_is_its_single_images(emulator):
    cases = SC.batch()
    items = [JD.parse(c.file, c.name) for c in cases]
    together, status, info = emulator(items)
    assert status == [SC.OK] * 3
    for it, c, img, words in zip(items, cases, together, info):
        (alone,), (s,), (w,) = emulator([it])
        assert s == SC.OK and np.array_equal(alone, img) and w == words == SR_info(c), it.name
        assert np.array_equal(img, D.pillow_pixels(c.file).transpose(2, 0, 1))
    assert not np.array_equal(together[0], together[1])


def SR_info(c):
    import jpeg_sync_ref as SR
    return SR.analyse(c.file, JS.S, JS.C).info


@pytest.mark.parametrize("name", ["cut-short", "no-code-matches", "category-above-11", "run-past-63", "ff-01-inside", "trailing-bytes", "oversubscribed-dht"])
def test_emulated_stage_answers_serial_to_a_malformed_stream(emulator, one_lane, name):
    """Between two good images of its shape; under the sanitizers, so a read or write outside a buffer fails the run.  The one-lane
    program (tests/jpeg_decode_emulate.cpp's job, csrc/jpeg_decode_core.h) gives the case's GP_JPEG_DECODE_* word for the same segment."""
    c = next(c for c in SC.malformed() if c.name == name)
    items = [JD.parse(f, n) for f, n in zip((c.goods[0], c.file, c.goods[1]), ("a", name, "b"))]
    assert all(it.nseg == 1 for it in items)
    images, status, _ = emulator(items)
    assert status == [SC.OK, SC.SERIAL, SC.OK], status
    for k in (0, 2):
        (alone,), _, _ = emulator([items[k]])
        assert np.array_equal(images[k], alone) and np.array_equal(alone, D.pillow_pixels(c.goods[k // 2]).transpose(2, 0, 1))
    assert one_lane(items[1])[1] == c.status


def test_a_subsequence_inside_one_block_and_a_dc_that_wraps(emulator, one_lane):
    c = SC.constructed(JS.S, JS.C)
    it = JD.parse(c.file, c.name)
    (img,), (s,), (words,) = emulator([it])
    want, word = one_lane(it)
    assert word == D.OK and s == SC.OK and words == c.ref.info and np.array_equal(img, want)
    assert np.array_equal(want[:, :, 112:120], want[:, :, 120:128]) and not np.array_equal(want[:, :, 120:128], want[:, :, 128:136])      # the DC of block 16 wrapped


def test_bad_segment_rows_are_serial(emulator):
    """nseg != B and max_image_seg != 1 are refused by the entry (exit code 4 here); a row that lies is SERIAL for its image alone."""
    good = JD.parse(D.pillow_file(D.noise(40, 88, 22), quality=90, subsampling=0))
    marked = JD.parse(D.pillow_file(D.noise(40, 88, 22), quality=90, subsampling=0, restart_marker_blocks=8))
    with pytest.raises(subprocess.CalledProcessError) as e:
        emulator([marked])
    assert e.value.returncode == 4
    liar = JD.parse(D.pillow_file(D.noise(40, 88, 23), quality=90, subsampling=0))
    liar.nmcu -= 1                                                         # its row says one MCU fewer than the shape has
    images, status, info = emulator([good, liar, good])
    assert status == [SC.OK, SC.SERIAL, SC.OK] and info[1] == (0, 0, 0, 0) and np.array_equal(images[0], images[2])
