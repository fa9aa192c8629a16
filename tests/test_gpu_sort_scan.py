"""-m gpu: the stable radix sort, the three-pass counting depth sort and the block scan (csrc/sort_scan.hip, csrc/bin_kernels.hip) on
their own, through gp_debug_sort_pairs / gp_debug_scan_blocks, at every size at which the code takes another kernel or branch.
All integer work: every comparison is exact (np.array_equal against tests/sort_ref.py); no number here is a tolerance.
Every output buffer carries 64 canary words behind its length and is filled with the canary word up front.

What each size reaches (arithmetic from rs_items_for, gp_radix_rowscan_kernel and the kpb loop of gp_depth_sort3):
  radix   n <= 262144: 4 keys per thread (1024 per block); 262145 .. 8388608: 8 (RS_ITEMS_MID); above: 16 (RS_ITEMS_LARGE)
          n = 8388608: nblocks = 8388608 / 2048 = 4096 -- the batched row scan with all 16 chunks of 256 counters full
          n = 4096 * 4096 + 4097: nblocks = 4098 > 4096 -- the chunk-at-a-time row scan
          nbits: passes share the bits evenly, per = ceil(nbits / ceil(nbits / 8)): 9 = 5+4, 13 = 7+6, 17 = 6+6+5, 25 = 7+7+7+4,
          31 = 8+8+8+7; an odd number of passes leaves the result in the other buffer pair
  dsort   n <= 512 * 2048: 8 keys per thread (dsort_pass<8>); up to 512 * 4096: dsort_pass<16>; up to 512 * 8192: dsort_pass<32>"""
import numpy as np
import pytest
import torch

import sort_ref as SR
from gpu_util import CANARY, CANARY_WORDS, canary_buffer as out_buf, read_canary_buffer as read_out, u32_to_device as to_dev

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _lib():
    from gaussianprediction_amd import _lib as m
    return m


def gpu_sort(algo, keys, vals, nbits, by_value):
    m = _lib()
    n = len(keys)
    k, v = to_dev(keys), (None if vals is None else to_dev(vals))
    bv = None if by_value is None else to_dev(by_value.reshape(-1))
    ko, vo = out_buf(n), out_buf(n)
    so, co = (out_buf(2 * n), out_buf(n)) if by_value is not None else (None, None)
    m.check(m.lib().gp_debug_sort_pairs(algo, k, v, n, nbits, bv, ko, vo, so, co, m.stream_ptr(torch.device(DEV))), "gp_debug_sort_pairs")
    res = [read_out(ko, n), read_out(vo, n)]
    if by_value is not None:
        res += [read_out(so, 2 * n).reshape(n, 2), read_out(co, n)]
    return res


def rand_u32(rng, n):
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def rand_rects(rng, n):
    """by_value of the epilogue: w, h in 0 .. 40, zeros included (count_out = w * h)."""
    w, h = rng.integers(0, 41, n), rng.integers(0, 41, n)
    return SR.pack_rects(rng.integers(0, 1 << 16, n), rng.integers(0, 1 << 16, n), w, h)


# (keys, reference order) of the last (n, nbits): the iota and the explicit-values case of one size share them
_last = {}


def random_case(n, nbits):
    if _last.get("key") != (n, nbits):
        _last.clear()
        keys = rand_u32(np.random.default_rng(n * 64 + nbits), n)          # full 32-bit keys: the bits at and above nbits are garbage to ignore
        _last.update(key=(n, nbits), keys=keys, order=SR.stable_order(keys, nbits))
    return _last["keys"], _last["order"]


def check_sort(algo, keys, nbits, explicit, seed, order=None):
    """One run with iota values (NULL) and the epilogue, or one with explicit random values (duplicates allowed)."""
    rng = np.random.default_rng(seed)
    n = len(keys)
    if explicit:
        pool = rand_u32(rng, max(n // 2, 1))
        vals = pool[rng.integers(0, len(pool), n)]                          # random u32, every value about twice
        ks, vs = SR.stable_sort_pairs(keys, vals, nbits, order=order)
        gk, gv = gpu_sort(algo, keys, vals, nbits, None)
    else:
        by_value = rand_rects(rng, n)
        ks, vs, so, co = SR.stable_sort_pairs(keys, None, nbits, by_value, order=order)
        gk, gv, gso, gco = gpu_sort(algo, keys, None, nbits, by_value)
        assert np.array_equal(gso, so), "epilogue: sorted_out"
        assert np.array_equal(gco, co), "epilogue: count_out"
    assert np.array_equal(gk, ks), "keys (full 32 bits, in the order of the low nbits)"
    assert np.array_equal(gv, vs), "values (equal keys keep their input order)"
    return gk, gv


SMALL_N = [1, 63, 64, 65, 1023, 1024, 1025, 3 * 1024 + 7, 9 * 1024 + 1, 262144, 262145]
SMALL_BITS = [1, 5, 8, 9, 13, 16, 17, 24, 25, 31, 32]
LARGE_N = {8388608: "mid8_rowscan_16_full_chunks", 8388609: "large16_items", 4096 * 4096 + 4097: "large16_rowscan_chunk_loop"}
_NOTE = {3 * 1024 + 7: "3blocks_idle_ids", 9 * 1024 + 1: "10blocks_per2", 262144: "last_4_items", 262145: "first_8_items"}
RADIX_CASES = [pytest.param(n, b, e, id=f"n{n}{'_' + _NOTE[n] if n in _NOTE else ''}-bits{b}-{'vals' if e else 'iota_epilogue'}")
               for n in SMALL_N for b in SMALL_BITS for e in (False, True)]
RADIX_CASES += [pytest.param(n, b, e, id=f"n{n}_{LARGE_N[n]}-bits{b}-{'vals' if e else 'iota_epilogue'}")
                for n in LARGE_N for b in (13, 32) for e in (False, True)]


@pytest.mark.parametrize("n,nbits,explicit", RADIX_CASES)
def test_radix_sort_random_keys(n, nbits, explicit):
    """gp_radix_sort_pairs.  n = 8388608 is the batched branch of gp_radix_rowscan_kernel with nblocks == 4096; n = 8388609 the first
    size on the RS_ITEMS_LARGE kernels; n = 4096 * 4096 + 4097 the chunk-at-a-time branch (nblocks = 4098) and the only size above
    10 M elements.  The sizes above 8 Mi run with 13 and 32 key bits only (two and four passes)."""
    keys, order = random_case(n, nbits)
    check_sort(0, keys, nbits, explicit, seed=n + 7 * nbits + int(explicit), order=order)


def pattern_keys(name, n):
    rng = np.random.default_rng(n)
    if name == "all_equal":
        return np.full(n, 0x1234ABCD, dtype=np.uint32)
    if name == "distinct60":
        return rand_u32(rng, 60)[rng.integers(0, 60, n)]
    if name == "ascending":
        return np.arange(n, dtype=np.uint32) * np.uint32(3)
    if name == "descending":
        return (np.arange(n, dtype=np.uint32) * np.uint32(3))[::-1].copy()
    if name == "all_ones":                 # the value the scatter kernel pads invalid lanes with, in a partial last block
        return np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    if name == "half_ones_half_zero":
        return np.where(rng.integers(0, 2, n) == 1, 0xFFFFFFFF, 0).astype(np.uint32)
    raise KeyError(name)


PATTERNS = ["all_equal", "distinct60", "ascending", "descending", "all_ones", "half_ones_half_zero"]


@pytest.mark.parametrize("nbits", [13, 32])
@pytest.mark.parametrize("n", [1025, 9 * 1024 + 1, 262145])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_radix_sort_key_patterns(pattern, n, nbits):
    keys = pattern_keys(pattern, n)
    order = SR.stable_order(keys, nbits)
    for explicit in (False, True):
        check_sort(0, keys, nbits, explicit, seed=n + nbits, order=order)


DSORT_N = {1: "", 2047: "", 2048: "", 2049: "", 512 * 2048: "_last_IT8", 512 * 2048 + 1: "_dsort_pass16", 512 * 4096 + 1: "_dsort_pass32",
           512 * 8192: "_dsort_pass32_max"}


@pytest.mark.parametrize("pattern", ["random", "distinct60", "all_ones"])
@pytest.mark.parametrize("n", [pytest.param(n, id=f"n{n}{note}") for n, note in DSORT_N.items()])
def test_counting_depth_sort(n, pattern):
    """gp_depth_sort3, called directly: dsort_pass<8> up to 512 * 2048 keys, dsort_pass<16> from 512 * 2048 + 1, dsort_pass<32> from
    512 * 4096 + 1 to the maximum 512 * 8192; epilogue on.  Equal to the host reference AND to the radix sort's result."""
    keys = rand_u32(np.random.default_rng(n), n) if pattern == "random" else pattern_keys(pattern, n)
    order = SR.stable_order(keys, 32)
    ck, cv = check_sort(1, keys, 32, False, seed=n, order=order)
    rk, rv = check_sort(0, keys, 32, False, seed=n, order=order)
    assert np.array_equal(ck, rk) and np.array_equal(cv, rv)


def test_counting_depth_sort_refuses_what_it_cannot_take():
    m = _lib()
    L = m.lib()
    n = 512 * 8192 + 1
    k, ko, vo = to_dev(np.zeros(16, dtype=np.uint32)), out_buf(16), out_buf(16)
    st = m.stream_ptr(torch.device(DEV))
    assert L.gp_debug_sort_pairs(1, k, None, n, 32, None, ko, vo, None, None, st) != 0 and b"n <= 4194304" in L.gp_last_error()
    assert L.gp_debug_sort_pairs(1, k, None, 16, 24, None, ko, vo, None, None, st) != 0 and b"32 key bits" in L.gp_last_error()
    assert L.gp_debug_sort_pairs(1, k, k, 16, 32, None, ko, vo, None, None, st) != 0 and b"iota values" in L.gp_last_error()
    for t in (ko, vo):
        assert np.array_equal(t.cpu().numpy(), np.full(16 + CANARY_WORDS, CANARY, dtype=np.int32)), "a refused call wrote its output"


@pytest.mark.parametrize("n", [1, 7, 8, 9, 2047, 2048, 2049, pytest.param(16 * 2048 + 5, id="32773_block17_wraps_to_slot0"), 300001])
def test_scan_blocks(n):
    """gp_scan_blocks_u32: exclusive scan inside blocks of 2048, the blocks' totals, and the grand total spread over 16 slots (only the
    slots' sum is contract)."""
    m = _lib()
    data = np.random.default_rng(n).integers(0, 5001, n).astype(np.uint32)
    excl, sums, total = SR.scan_blocks(data)
    nb = len(sums)
    d = out_buf(n)
    d[:n] = to_dev(data)
    bs, slots = out_buf(nb), out_buf(SR.TOTAL_SLOTS)
    m.check(m.lib().gp_debug_scan_blocks(d, n, bs, slots, m.stream_ptr(torch.device(DEV))), "gp_debug_scan_blocks")
    assert np.array_equal(read_out(d, n), excl)
    assert np.array_equal(read_out(bs, nb), sums)
    got = read_out(slots, SR.TOTAL_SLOTS)
    assert int(got.astype(np.uint64).sum() & 0xFFFFFFFF) == total == int(data.sum(dtype=np.uint64))
