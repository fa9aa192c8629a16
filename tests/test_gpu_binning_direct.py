"""-m gpu: the binning stage of the forward on its own (gp_debug_bin_lists runs the function gp_raster_forward runs), both ways --
path 0 by counting (gp_bin_count_kernel / gp_bin_scan_kernel / gp_bin_scatter_kernel of csrc/bin_kernels.hip), path 1 by scan +
gp_duplicate_kernel + radix sort by tile + gp_tile_ranges_kernel -- against tests/sort_ref.bin_lists.  Integer work: every comparison
is exact, and where both paths run they must agree entry for entry.  Outputs carry 64 canary words behind their length.

What each case reaches (arithmetic from gp_bin_plan: G doubles from 256 while ceil(N / G) > 512, up to 8192):
  N <= 131072: G 256 (count<1>, scatter<1>); 131073: G 512 (count<1>, scatter<2>); 262145: G 1024 (count<1>, scatter<4>);
  524289: G 2048 (count<2>, scatter<8>); 1048577: G 4096 (count<4>, scatter<16>); 2097153 .. 4194304: G 8192 (count<8>, scatter<32>)
  tile sort of path 1: tile_bits_for(T) bits -- T = 8193: 14 = 7+7; 65536: 16 = 8+8; 65792: 17 = 6+6+5, three passes: the sorted
  result lands in buffer pair 1, which is then the one aliasing point_list (res = passes & 1)."""
import ctypes as C

import numpy as np
import pytest
import torch

import sort_ref as SR
from gpu_util import CANARY, CANARY_WORDS, canary_buffer as out_buf, read_canary_buffer as read_out, u32_to_device as to_dev

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
R_LIMIT = 12_000_000


def _lib():
    from gaussianprediction_amd import _lib as m
    return m


def make_scene(N, gx, gy, seed, heavy=False, n_full=16):
    """sorted_ids = a permutation of 0 .. N-1; rectangles inside the grid: ~30 % zero-area (w = 0 or h = 0), ~60 % 1x1, the rest up to
    8x8 (small extents likelier), and n_full Gaussians (all of them below N = n_full) that cover the whole grid."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(N).astype(np.uint32)
    if heavy:                       # every Gaussian covers tile 0 and nothing else
        z = np.zeros(N, dtype=np.int64)
        return ids, SR.pack_rects(z, z, z + 1, z + 1)
    kind = rng.random(N)
    w = np.ones(N, dtype=np.int64)
    h = np.ones(N, dtype=np.int64)
    big = kind >= 0.9
    w[big] = 1 + (8 * rng.random(int(big.sum())) ** 2).astype(np.int64)
    h[big] = 1 + (8 * rng.random(int(big.sum())) ** 2).astype(np.int64)
    w, h = np.minimum(w, gx), np.minimum(h, gy)
    w[kind < 0.15] = 0
    h[(kind >= 0.15) & (kind < 0.3)] = 0
    full = rng.choice(N, size=min(n_full, N), replace=False)
    w[full], h[full] = gx, gy
    minx = (rng.random(N) * (gx - np.maximum(w, 1) + 1)).astype(np.int64)
    miny = (rng.random(N) * (gy - np.maximum(h, 1) + 1)).astype(np.int64)
    return ids, SR.pack_rects(minx, miny, w, h)


_scene = {}


def scene_and_reference(N, gx, gy, heavy=False, n_full=16):
    """(ids, rects, point_list, ranges, R), built once per case (the last one is kept)."""
    key = (N, gx, gy, heavy, n_full)
    if _scene.get("key") != key:
        _scene.clear()
        ids, rects = make_scene(N, gx, gy, seed=N * 7 + gx * 3 + gy, heavy=heavy, n_full=n_full)
        assert SR.instance_count(rects) <= R_LIMIT
        _scene.update(key=key, val=(ids, rects) + SR.bin_lists(ids, rects, gx, gx * gy))
    return _scene["val"]


def gpu_bin(path, ids_d, rects_d, N, gx, gy, capacity, list_words):
    m = _lib()
    T = gx * gy
    pl, ranges, status = out_buf(list_words), out_buf(2 * T), out_buf(3)
    r_out = C.c_uint32(0xFFFFFFFF)
    m.check(m.lib().gp_debug_bin_lists(path, N, gx, gy, ids_d, rects_d, capacity, pl, ranges, status, C.byref(r_out),
                                       m.stream_ptr(torch.device(DEV))), "gp_debug_bin_lists")
    return read_out(pl, list_words), read_out(ranges, 2 * T).view(np.int32).reshape(T, 2), read_out(status, 3), int(r_out.value)


def assert_refused(path, ids_d, rects_d, N, gx, gy):
    m = _lib()
    L = m.lib()
    T = gx * gy
    pl, ranges, status = out_buf(16), out_buf(2 * T), out_buf(3)
    r_out = C.c_uint32(0)
    rc = L.gp_debug_bin_lists(path, N, gx, gy, ids_d, rects_d, 0, pl, ranges, status, C.byref(r_out), m.stream_ptr(torch.device(DEV)))
    assert rc != 0 and b"binning by counting does not take" in L.gp_last_error()
    assert np.array_equal(ranges.cpu().numpy(), np.full(2 * T + CANARY_WORDS, CANARY, dtype=np.int32)), "a refused call wrote its output"


def assert_exact(got, ref_list, ref_ranges, R):
    pl, ranges, status, r_out = got
    assert r_out == R
    assert np.array_equal(pl[:R], ref_list), "point_list"
    filled = ref_ranges[:, 1] > ref_ranges[:, 0]
    assert np.array_equal(ranges[filled], ref_ranges[filled]), "ranges of the tiles that have instances"
    assert np.array_equal(ranges[~filled, 0], ranges[~filled, 1]), "an empty tile's range is empty"
    assert int(status[0]) == R and int(status[1]) == 0, "status = {R, no overflow}"


def run_exact(N, gx, gy, paths, heavy=False, n_full=16):
    ids, rects, ref_list, ref_ranges, R = scene_and_reference(N, gx, gy, heavy, n_full)
    ids_d, rects_d = to_dev(ids), to_dev(rects.reshape(-1))
    got = {}
    for path in paths:
        got[path] = gpu_bin(path, ids_d, rects_d, N, gx, gy, 0, R)
        assert_exact(got[path], ref_list, ref_ranges, R)
    if len(got) == 2:
        assert np.array_equal(got[0][0], got[1][0]), "the two paths' lists differ"
        filled = ref_ranges[:, 1] > ref_ranges[:, 0]
        assert np.array_equal(got[0][1][filled], got[1][1][filled]), "the two paths' ranges differ"
    return ids_d, rects_d


PLAN_N = {1: "tiny", 1000: "G256_4blocks", 131072: "G256_NB512", 131073: "G512_count1_scatter2", 262145: "G1024_count1_scatter4",
          524289: "G2048_count2_scatter8", 1048577: "G4096_count4_scatter16", 2097153: "G8192_count8_scatter32", 4194304: "G8192_NB512_max"}


@pytest.mark.parametrize("N", [pytest.param(n, id=f"N{n}_{note}") for n, note in PLAN_N.items()])
def test_plan_boundaries_at_the_training_grid(N):
    """Every block size gp_bin_plan can pick, at T = 85 x 64 = 5440 tiles, both paths.  G = 512, 1024, 4096 and 8192 select
    gp_bin_scatter_kernel<2>, <4>, <16>, <32> and gp_bin_count_kernel<4>, <8>."""
    run_exact(N, 85, 64, (0, 1))


def test_one_gaussian_beyond_the_counting_plan():
    """N = 512 * 8192 + 1: the counting path is refused (not silently replaced), the duplicate + sort path bins it."""
    N = 512 * 8192 + 1
    ids_d, rects_d = run_exact(N, 85, 64, (1,))
    assert_refused(0, ids_d, rects_d, N, 85, 64)


GRIDS = [(1, 1), (2, 1), (63, 1), (64, 1), (65, 1), (91, 45), (125, 63), (128, 64)]


@pytest.mark.parametrize("gx,gy", [pytest.param(gx, gy, id=f"{gx}x{gy}_T{gx * gy}") for gx, gy in GRIDS])
def test_tile_counts_both_paths(gx, gy):
    """N = 20000.  T = 1, 2, 63, 64, 65: gp_bin_scan_kernel's grid of 64-tile workgroups and odd T in the packed 16-bit counters;
    4095 (odd), 7875, and 8192 = GP_BIN_MAX_TILES, the counting path's largest LDS footprint."""
    run_exact(20000, gx, gy, (0, 1))


@pytest.mark.parametrize("gx,gy", [pytest.param(8193, 1, id="8193x1_14bits_7+7"), pytest.param(256, 256, id="256x256_16bits_8+8"),
                                   pytest.param(257, 256, id="257x256_17bits_three_passes_res_parity_1")])
def test_tile_counts_beyond_the_counting_path(gx, gy):
    """More than GP_BIN_MAX_TILES tiles: duplicate + radix tile sort only (counting refused).  257 x 256 = 65792 tiles need 17 key bits:
    three passes, so the sorted values end in buffer pair 1 (res = passes & 1) -- the pair that aliases point_list then."""
    ids_d, rects_d = run_exact(20000, gx, gy, (1,))
    assert_refused(0, ids_d, rects_d, 20000, gx, gy)


def test_heavy_tile_both_paths():
    """70000 Gaussians that all cover tile 0 only: one list of length 70000 -- more than a 16-bit per-wave packed counter holds, spread
    over 274 blocks of the counting path."""
    run_exact(70000, 85, 64, (0, 1), heavy=True)


def test_sparse_scene_leaves_tiles_empty_both_paths():
    """No Gaussian covers the whole grid: 3000 Gaussians on 128 x 64 tiles leave most tiles without a list (their range stays empty)."""
    ref_ranges = scene_and_reference(3000, 128, 64, n_full=0)[3]
    assert int((ref_ranges[:, 0] == ref_ranges[:, 1]).sum()) > 4000
    run_exact(3000, 128, 64, (0, 1), n_full=0)


@pytest.mark.parametrize("gx,gy,paths", [pytest.param(85, 64, (0, 1), id="85x64_both_paths"),
                                         pytest.param(127, 129, (1,), id="127x129_T16383_sort_path_sentinels_behind_tile_16382"),
                                         pytest.param(128, 128, (1,), id="128x128_T16384_sort_path_one_more_key_bit")])
def test_capacity_mode(gx, gy, paths):
    """capacity > 0 (gp_raster_settings.binning_capacity): the sort path pads its keys up to the capacity with 0xFFFFFFFF, whose low
    tile_bits_for(T + 1) bits have to sort behind every real tile id.  T = 16383 = 2^14 - 1: the padding's 14 low bits are 16383, one
    more than the last tile; T = 16384: the padding needs a 15th bit to differ from the last tile.
    Room to spare: lists, ranges and status as in exact mode.  Half the room: status = {R, 1} and nothing at or behind the capacity is
    written (what the cut lists hold is not compared: the two paths cut differently, by design)."""
    N = 20000
    ids, rects, ref_list, ref_ranges, R = scene_and_reference(N, gx, gy)
    ids_d, rects_d = to_dev(ids), to_dev(rects.reshape(-1))
    for path in paths:
        cap = R + 5000
        pl, ranges, status, r_out = gpu_bin(path, ids_d, rects_d, N, gx, gy, cap, cap)
        assert r_out == cap
        assert_exact((pl, ranges, status, R), ref_list, ref_ranges, R)
        cap = R // 2
        pl, ranges, status, r_out = gpu_bin(path, ids_d, rects_d, N, gx, gy, cap, cap)          # (gpu_bin checks the canaries behind cap)
        assert r_out == cap and int(status[0]) == R and int(status[1]) == 1
