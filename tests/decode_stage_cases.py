"""Shared by the emulator job writers (tests/test_png_decode_host.py, tests/jpeg_decode_cases.py) and the staging tests
(tests/test_decode_stage_host.py, tests/test_gpu_decode_stage.py): decode_stage.layout and fill into a plain numpy array -- the code
the device path stages with -- a group's sections cut out of it, and per format a tiny file set of two shape groups."""
import zlib

import numpy as np

import jpeg_decode_cases as JC
import png_decode_cases as PC
from gaussianprediction_amd import decode_stage as S, jpeg_decode as JD, png_decode as PD


def filled(plans, pool=None):
    """The staging bytes of `plans` (laid out here) in a numpy array; 0xEE wherever fill writes nothing."""
    host = np.full(S.layout(plans), 0xEE, dtype=np.uint8)
    S.fill(host, plans, pool)
    return host


def spans(pl):
    """[(first byte, byte count)] of a laid-out plan's segment table, image table, table bytes and payload."""
    return [(pl.seg_at, 40 * len(pl.seg)), (pl.img_at, 4 * len(pl.image_seg)), (pl.tab_at, len(pl.tables)), (pl.pay_at, pl.bytes)]


def sections(host, pl):
    """(segment table, image table, table bytes, payload) of one group, as bytes, out of a filled array."""
    return tuple(host[at:at + n].tobytes() for at, n in spans(pl))


def png_set():
    """(items, banded, shapes, plans): small, two-band, small -- the groups [0, 2] (one segment each) and [1] (two segments)."""
    rows = np.tile(np.random.default_rng(3).integers(0, 256, (1, 120, 3), dtype=np.uint8), (60, 1, 1))
    stream = PC.filtered(rows, [0] * 60)
    c = zlib.compressobj(9)
    first = c.compress(stream[:PC.BAND]) + c.flush(zlib.Z_FULL_FLUSH)
    two_bands = PC.case("two-bands", rows, first + c.compress(stream[PC.BAND:]) + c.flush(), cuts=[len(first)], mode=PC.BANDED)
    items = [PD.parse(c.file, c.name) for c in (PC.good_small(1), two_bands, PC.good_small(2))]
    banded = [it.banded for it in items]
    shapes = PD.groups(items)
    assert banded == [False, True, False] and [idx for _, _, idx in shapes] == [[0, 2], [1]]
    return items, banded, shapes, PD.plans(items, banded, shapes)


def jpeg_set():
    """(items, shapes, plans): 17 x 33 at 4:2:0 with a restart marker behind every MCU, 8 x 8 at 4:4:4 without, 17 x 33 again."""
    files = [JC.pillow_file(JC.noise(17, 33, 1), quality=90, subsampling=2, restart_marker_blocks=1),
             JC.pillow_file(JC.noise(8, 8, 2), quality=90, subsampling=0),
             JC.pillow_file(JC.noise(17, 33, 3), quality=90, subsampling=2, restart_marker_blocks=1)]
    items = [JD.parse(f, f"<{k}>") for k, f in enumerate(files)]
    shapes = JD.groups(items)
    assert [it.nseg for it in items] == [6, 1, 6] and [idx for _, idx in shapes] == [[0, 2], [1]]
    return items, shapes, JD.plans(items, shapes)
