"""No GPU: the byte layout of the decoders' staging buffer (decode_stage.layout and fill) on two shape groups of 2 + 1 tiny files per
format -- the alignments gp_png_decode, gp_jpeg_decode and gp_jpeg_sync_decode demand of their pointers, and that what they read
there is what tables() returned."""
import numpy as np
import pytest

import decode_stage_cases as SC
from gaussianprediction_amd import decode_stage as S, jpeg_decode as JD, png_decode as PD


@pytest.fixture(scope="module")
def png():
    return SC.png_set()


@pytest.fixture(scope="module")
def jpeg():
    return SC.jpeg_set()


def _plans(request, kind):
    return request.getfixturevalue(kind)[-1]


@pytest.mark.parametrize("kind", ["png", "jpeg"])
def test_alignment_and_no_overlap(request, kind):
    plans = _plans(request, kind)
    total = S.layout(plans)
    assert len(plans) == 2 and [len(pl.idx) for pl in plans] == [2, 1]
    taken = []
    for pl in plans:
        assert pl.seg_at % 8 == 0 and pl.img_at % 4 == 0 and pl.tab_at % 16 == 0 and pl.pay_at % 16 == 0
        assert len(pl.image_seg) == len(pl.idx) + 1 and pl.image_seg[-1] == len(pl.seg) and pl.bytes > 0
        taken += SC.spans(pl)
    seg, img, tab, pay = ([s for s in taken[k::4]] for k in range(4))
    assert seg[0][0] == 0 and tab[0][0] % 16 == 0 and pay[0][0] % 256 == 0              # where each of the four parts begins
    assert img[0][0] == seg[-1][0] + seg[-1][1]                                         # the image tables directly behind the segment tables
    flat = seg + img + tab + pay                                                         # ... in the order they lie in the buffer
    for (a, n), (b, _) in zip(flat, flat[1:]):
        assert n >= 0 and a + n <= b, flat
    assert total == -(-(pay[-1][0] + pay[-1][1]) // 16) * 16 + 16                       # the last payload's end, rounded up as every group's, plus 16


@pytest.mark.parametrize("kind", ["png", "jpeg"])
def test_tables_and_payload_read_back(request, kind):
    got = request.getfixturevalue(kind)
    items, shapes, plans = got[0], got[-2], got[-1]
    host = SC.filled(plans)
    for group, pl in zip(shapes, plans):
        want = PD.tables(items, got[1], group[-1]) if kind == "png" else JD.tables(items, group[-1])
        rows = host[pl.seg_at:pl.seg_at + 40 * len(want[0])].view(np.int64).reshape(-1, 5)
        assert np.array_equal(rows, np.array(want[0], dtype=np.int64).reshape(-1, 5)) and len(rows) == len(pl.seg)
        assert host[pl.img_at:pl.img_at + 4 * len(want[1])].view(np.int32).tolist() == list(want[1])
        assert pl.bytes == want[3] and len(pl.copies) == len(want[2]) > 0
        for (at, piece), (at2, _) in zip(pl.copies, want[2]):
            assert at == at2 and host[pl.pay_at + at:pl.pay_at + at + len(piece)].tobytes() == bytes(piece) and len(piece) > 0
        if kind == "jpeg":
            assert pl.most == want[4] and len(pl.tables) == JD.TABLE_BYTES * len(pl.idx)
            assert host[pl.tab_at:pl.tab_at + len(pl.tables)].tobytes() == b"".join(items[i].tables for i in pl.idx)
    used = np.zeros(len(host), dtype=bool)                                               # fill writes the defined sections and nothing else
    for pl in plans:
        for at, n in SC.spans(pl):
            used[at:at + n] = True
    assert (host[~used] == 0xEE).all() and not used[-16:].any()


def test_png_has_an_empty_table_section(png):
    plans = png[-1]
    S.layout(plans)
    nseg, nimg = sum(len(pl.seg) for pl in plans), sum(len(pl.image_seg) for pl in plans)
    assert (nseg, nimg) == (4, 5)
    at = -(-(40 * nseg + 4 * nimg) // 256) * 256                                         # where png_decode.stage put the payload before decode_stage
    for pl in plans:
        assert pl.tables == b"" and pl.tab_at == -(-(40 * nseg + 4 * nimg) // 16) * 16 and pl.pay_at == at
        at += -(-pl.bytes // 16) * 16


def test_a_pool_fills_the_same_bytes(jpeg):
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(2) as pool:
        assert np.array_equal(SC.filled(jpeg[-1], pool), SC.filled(jpeg[-1]))
