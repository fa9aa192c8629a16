"""Host reference of the index primitives behind the tile binning (csrc/sort_scan.hip, csrc/bin_kernels.hip, gp_duplicate_kernel /
gp_tile_ranges_kernel): vectorised numpy, integers only -- every comparison against it is exact.  The restatements the references
themselves are checked against (plain Python loops, small n) live in tests/test_sort_ref_host.py."""
import numpy as np

SCAN_TILE = 2048            # gp_scan_blocks_u32 scans inside blocks of this many elements
TOTAL_SLOTS = 16            # ... and spreads the grand total over this many words


def stable_order(keys, nbits=32):
    """argsort(keys & mask, kind="stable"): the permutation a stable sort by the low `nbits` key bits applies."""
    keys = np.asarray(keys, dtype=np.uint32)
    masked = keys & np.uint32(0xFFFFFFFF if nbits >= 32 else (1 << nbits) - 1)
    if nbits <= 16:
        masked = masked.astype(np.uint16)       # (same order; numpy's stable sort of 16-bit integers is a radix sort: linear time)
    return np.argsort(masked, kind="stable")


def stable_sort_pairs(keys, vals=None, nbits=32, by_value=None, order=None):
    """Stable sort by the low `nbits` key bits.  Returns (keys, vals) in sorted order -- the FULL keys: the bits at and above nbits are
    carried along, never compared -- and, with by_value [n, 2], the epilogue's (sorted_out [n, 2], count_out [n]) as well.
    vals None: the values are 0 .. n-1.  order: stable_order(keys, nbits) where the caller has it already."""
    keys = np.asarray(keys, dtype=np.uint32)
    n = len(keys)
    vals = np.arange(n, dtype=np.uint32) if vals is None else np.asarray(vals, dtype=np.uint32)
    if order is None:
        order = stable_order(keys, nbits)
    ks, vs = keys[order], vals[order]
    if by_value is None:
        return ks, vs
    sorted_out = np.asarray(by_value, dtype=np.uint32).reshape(-1, 2)[vs]
    y = sorted_out[:, 1]
    return ks, vs, sorted_out, (y & np.uint32(0xFFFF)) * (y >> np.uint32(16))


def scan_blocks(data):
    """(exclusive scan inside blocks of SCAN_TILE, the blocks' totals, grand total mod 2^32)."""
    data = np.asarray(data, dtype=np.uint32)
    n = len(data)
    nb = (n + SCAN_TILE - 1) // SCAN_TILE
    pad = np.zeros(nb * SCAN_TILE, dtype=np.uint64)
    pad[:n] = data
    blocks = pad.reshape(nb, SCAN_TILE)
    incl = np.cumsum(blocks, axis=1)
    excl = (incl - blocks).reshape(-1)[:n]
    sums = incl[:, -1] if nb else np.zeros(0, dtype=np.uint64)
    m = np.uint64(0xFFFFFFFF)
    return (excl & m).astype(np.uint32), (sums & m).astype(np.uint32), int(int(pad.sum()) & 0xFFFFFFFF)


def pack_rects(minx, miny, w, h):
    """[n, 2] u32: .x = minx | miny << 16, .y = w | h << 16 (tiles)."""
    u = lambda a: np.asarray(a, dtype=np.uint32)
    return np.stack([u(minx) | (u(miny) << np.uint32(16)), u(w) | (u(h) << np.uint32(16))], axis=1)


def instance_count(rects):
    y = np.asarray(rects, dtype=np.uint32).reshape(-1, 2)[:, 1].astype(np.int64)
    return int(((y & 0xFFFF) * (y >> 16)).sum())


def bin_lists(sorted_ids, rects, gx, T):
    """Per-tile lists of depth-ordered Gaussians.  rects [n, 2] as pack_rects; Gaussian i (in depth order) covers the tiles
    (miny + yy) * gx + minx + xx, row-major.  Instances are generated in input order, then stably sorted by tile.
    Returns (point_list [R] u32, ranges [T, 2] i32 with [start, end) -- (0, 0) for an empty tile --, R)."""
    sorted_ids = np.asarray(sorted_ids, dtype=np.uint32)
    rects = np.asarray(rects, dtype=np.uint32).reshape(-1, 2)
    minx = (rects[:, 0] & 0xFFFF).astype(np.int64)
    miny = (rects[:, 0] >> 16).astype(np.int64)
    w = (rects[:, 1] & 0xFFFF).astype(np.int64)
    h = (rects[:, 1] >> 16).astype(np.int64)
    cnt = w * h
    R = int(cnt.sum())
    owner = np.repeat(np.arange(len(cnt), dtype=np.int64), cnt)
    k = np.arange(R, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)       # index inside the owner's rectangle
    wo = np.maximum(w[owner], 1)
    yy = k // wo
    tile = (miny[owner] + yy) * gx + minx[owner] + (k - yy * wo)
    order = np.argsort(tile.astype(np.uint16) if T <= 65536 else tile, kind="stable")
    point_list = sorted_ids[owner[order]]
    per_tile = np.bincount(tile, minlength=T).astype(np.int64)
    assert len(per_tile) == T, "a rectangle leaves the grid"
    end = np.cumsum(per_tile)
    ranges = np.stack([end - per_tile, end], axis=1)
    ranges[per_tile == 0] = 0
    return point_list, ranges.astype(np.int32), R
