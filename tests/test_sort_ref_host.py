"""CPU: the vectorised host references of tests/sort_ref.py against plain Python-loop restatements of the same definitions, at
n <= 200 (zero-area rectangles, empty tiles, garbage key bits above nbits included).  The GPU tests (test_gpu_sort_scan.py,
test_gpu_binning_direct.py) compare the kernels with sort_ref exactly, so sort_ref itself has to be right first."""
import numpy as np
import pytest

import sort_ref as SR


def _loop_sort(keys, vals, nbits):
    """Insertion sort on the masked key: an element moves in front of its left neighbour only when its key is strictly smaller."""
    mask = (1 << nbits) - 1
    out = []
    for k, v in zip(keys.tolist(), vals.tolist()):
        pos = len(out)
        while pos > 0 and (out[pos - 1][0] & mask) > (k & mask):
            pos -= 1
        out.insert(pos, (k, v))
    return [k for k, _ in out], [v for _, v in out]


@pytest.mark.parametrize("n", [0, 1, 2, 63, 200])
@pytest.mark.parametrize("nbits", [1, 5, 9, 13, 17, 25, 31, 32])
def test_stable_sort_pairs_against_an_insertion_sort(n, nbits):
    rng = np.random.default_rng(1000 * n + nbits)
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    if n >= 63:
        keys[: n // 2] = (keys[: n // 2] & ~np.uint32(7)) | np.uint32(3)       # many ties in the low bits, garbage above them
    vals = rng.integers(0, 50, n, dtype=np.uint64).astype(np.uint32)            # duplicate values
    for v in (None, vals):
        ks, vs = SR.stable_sort_pairs(keys, v, nbits)
        lk, lv = _loop_sort(keys, np.arange(n) if v is None else v, nbits)
        assert ks.dtype == np.uint32 and vs.dtype == np.uint32
        assert ks.tolist() == lk and vs.tolist() == lv


def test_sort_epilogue_follows_the_values():
    rng = np.random.default_rng(7)
    n = 150
    keys = rng.integers(0, 40, n, dtype=np.uint64).astype(np.uint32)
    w, h = rng.integers(0, 41, n), rng.integers(0, 41, n)
    w[:5] = 0
    h[5:10] = 0
    by_value = SR.pack_rects(rng.integers(0, 100, n), rng.integers(0, 100, n), w, h)
    ks, vs, so, co = SR.stable_sort_pairs(keys, None, 32, by_value)
    for pos in range(n):
        v = int(vs[pos])
        assert so[pos].tolist() == by_value[v].tolist()
        assert int(co[pos]) == int(w[v]) * int(h[v])
    assert co.dtype == np.uint32 and so.shape == (n, 2)


@pytest.mark.parametrize("n", [1, 7, 200])
def test_scan_blocks_small(n):
    data = np.random.default_rng(n).integers(0, 5001, n).astype(np.uint32)
    excl, sums, total = SR.scan_blocks(data)
    run = 0
    for i in range(n):
        assert int(excl[i]) == run
        run += int(data[i])
    assert sums.tolist() == [run] and total == run


def test_scan_blocks_restarts_at_every_block_and_wraps_the_total():
    n = 2 * SR.SCAN_TILE + 3
    data = np.full(n, 0xFFFFFF, dtype=np.uint32)
    excl, sums, total = SR.scan_blocks(data)
    for i in (0, 1, SR.SCAN_TILE - 1, SR.SCAN_TILE, SR.SCAN_TILE + 1, 2 * SR.SCAN_TILE, n - 1):
        assert int(excl[i]) == ((i % SR.SCAN_TILE) * 0xFFFFFF) % (1 << 32)       # (u32 arithmetic, as on the device)
    assert sums.tolist() == [(SR.SCAN_TILE * 0xFFFFFF) & 0xFFFFFFFF] * 2 + [3 * 0xFFFFFF]
    assert n * 0xFFFFFF > 1 << 32 and total == (n * 0xFFFFFF) % (1 << 32)
    e0, s0, t0 = SR.scan_blocks(np.zeros(0, dtype=np.uint32))
    assert len(e0) == 0 and len(s0) == 0 and t0 == 0


def _loop_bin_lists(sorted_ids, minx, miny, w, h, gx, T):
    lists = [[] for _ in range(T)]
    for i in range(len(sorted_ids)):                 # depth order
        for yy in range(int(h[i])):
            for xx in range(int(w[i])):
                lists[(int(miny[i]) + yy) * gx + int(minx[i]) + xx].append(int(sorted_ids[i]))
    point_list, ranges = [], []
    for t in range(T):
        ranges.append([len(point_list), len(point_list) + len(lists[t])] if lists[t] else [0, 0])
        point_list += lists[t]
    return point_list, ranges


@pytest.mark.parametrize("n,gx,gy", [(1, 1, 1), (30, 2, 1), (200, 7, 5), (200, 65, 1), (120, 16, 16)])
def test_bin_lists_against_nested_loops(n, gx, gy):
    rng = np.random.default_rng(n * 131 + gx)
    T = gx * gy
    w = rng.integers(0, min(gx, 4) + 1, n)
    h = rng.integers(0, min(gy, 4) + 1, n)
    if n > 20:
        if (gx, gy) != (16, 16):
            w[:3], h[:3] = gx, gy                    # whole-grid rectangles (the 16 x 16 case keeps tiles empty instead)
        w[3:8] = 0                                   # zero-area: no width ...
        h[8:13] = 0                                  # ... or no height (the other extent is not 0)
    minx = np.array([rng.integers(0, gx - max(int(x), 1) + 1) for x in w])
    miny = np.array([rng.integers(0, gy - max(int(y), 1) + 1) for y in h])
    ids = rng.permutation(n).astype(np.uint32)
    rects = SR.pack_rects(minx, miny, w, h)
    pl, ranges, R = SR.bin_lists(ids, rects, gx, T)
    lpl, lranges = _loop_bin_lists(ids, minx, miny, w, h, gx, T)
    assert R == len(lpl) == SR.instance_count(rects) == int((w * h).sum())
    assert pl.dtype == np.uint32 and pl.tolist() == lpl
    assert ranges.dtype == np.int32 and ranges.tolist() == lranges
    if (gx, gy) == (16, 16):
        assert any(r == [0, 0] for r in lranges[1:]), "the case is meant to leave tiles empty"


def test_bin_lists_without_instances():
    ids = np.arange(5, dtype=np.uint32)
    rects = SR.pack_rects([0, 1, 2, 0, 1], [0, 0, 1, 1, 0], [0, 3, 0, 0, 2], [2, 0, 0, 5, 0])
    pl, ranges, R = SR.bin_lists(ids, rects, 4, 8)
    assert R == 0 and len(pl) == 0 and ranges.tolist() == [[0, 0]] * 8
