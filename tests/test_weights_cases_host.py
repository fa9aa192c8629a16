"""The conditions the direct GPU tests of the weights kernels (test_gpu_weights_direct.py) rely on, asserted on the reference
alone: every regime-named case is in its regime, the excluded shares stay under their cap, every tie has one answer."""
import numpy as np
import pytest
import torch

import weights_cases as wc
from gaussianprediction_amd.weights_ops import morton_order


def test_dense_level_counts():
    assert [len(wc.dense_levels(wc.grid(t))) for t in (9, 10, 12, 15, 17, 19)] == [0, 0, 1, 3, 4, 5]
    meta = wc.grid(19)
    assert meta["total"] == 6098120
    assert [meta["resolutions"][l] for l in wc.dense_levels(meta)] == [16, 23, 31, 43, 59]      # only the first is a power of two
    # a dense level whose table is res^3 rounded up to a multiple of 8 (the modulo is NOT the identity's natural size)
    assert any(meta["sizes"][l] != meta["resolutions"][l] ** 3 for l in wc.dense_levels(meta))


def test_edge_points_are_where_they_claim():
    meta = wc.grid(15)
    e = wc.edge_points(meta)
    assert np.all(e[0] == 0)
    c0 = np.float32(meta["scales"][0])
    for v in wc.EXACT_ON_LEVEL0:
        pos = np.float32(np.float64(np.float32(v)) * np.float64(c0) + 0.5)
        assert pos == np.floor(pos), v                               # weight exactly 0 on level 0
    for l in range(16):                                              # the last cell of every level, both signs
        c = wc.cells(e, meta["scales"][l])
        assert (c == meta["resolutions"][l] - 1).all(axis=1).any() and (c <= -(meta["resolutions"][l] - 1)).all(axis=1).any()
    assert np.abs(e).max() == 1e4
    assert any(np.array_equal(e[i], e[i + 1]) for i in range(len(e) - 1))       # twins
    # random fill: about half of the cells negative
    p = wc.points_with_edges(513, meta, 1)
    assert p.shape == (513, 3) and 0.3 < (wc.cells(p, 15.0) < 0).mean() < 0.7
    assert np.array_equal(wc.points_with_edges(1, meta, 1), e[:1])


def _perm_of(xyz):
    return morton_order(torch.tensor(xyz)).numpy() if len(xyz) > 4096 else None      # WeightsModel.forward's rule


@pytest.mark.parametrize("name", list(wc.BACKWARD_CASES))
def test_backward_cases_are_in_their_regimes(name):
    r = wc.backward_reference(name)
    meta, n = r["meta"], r["n"]
    bm = wc.boxed_map(r["xyz"], _perm_of(r["xyz"]), meta)
    share = bm.mean(axis=0)
    print(name, "boxed share per dense level", share, "excluded share", r["excluded_share"])
    assert bm.shape == ((n + 31) // 32, len(wc.dense_levels(meta)))
    assert bm.any(axis=0).all() and (~bm).any(axis=0).all()          # both forms on every dense level
    assert (bm.any(axis=1) & (~bm).any(axis=1)).any()                # a workgroup boxed on one level and not on another
    assert r["excluded"] * 100 <= n                                  # AMBIGUOUS_CAP, in whole rows
    if name.startswith("persistent_mixed"):
        assert np.all(share > 0.10) and np.all(share < 0.90)
        assert wc.wm_blocks_per_workgroup(n) == (2, 3)               # persistent loop with prefetch, ragged split
        assert (wc.cells(r["xyz"], 15.0) < 0).mean() > 0.3
    if name == "four_dense_levels":
        assert len(wc.dense_levels(meta)) == 4 and meta["resolutions"][3] == 43
    for y in r["yardstick"].values():                               # the float32 oracle itself is far inside the floor of the bar
        assert wc.bar(y[0]) == 1e-5 and wc.bar(y[1]) == 1e-5


def test_boxed_map_on_constructed_groups():
    meta = wc.grid(15)
    tight = np.full((32, 3), 0.301, np.float32)                      # one cell: extents 2 x 2 x 2
    wide = np.linspace(-1.5, 1.5, 32, dtype=np.float32)[:, None].repeat(3, 1)
    bm = wc.boxed_map(np.concatenate([tight, wide, tight[:5]]), None, meta)
    assert bm.tolist() == [[True] * 3, [False] * 3, [True] * 3]
    # extents 9 x 9 x 9 = 729 boxed, 10 x 10 x 11 = 1100 not (level 0: cell = floor(15 x + 0.5))
    g = np.zeros((32, 3), np.float32)
    g[1] = (7 / 15, 7 / 15, 7 / 15)
    assert wc.boxed_map(g, None, meta)[0, 0]
    g[1] = (8 / 15, 8 / 15, 9 / 15)
    assert not wc.boxed_map(g, None, meta)[0, 0]
    perm = np.arange(64)[::-1].copy()
    assert wc.boxed_map(np.concatenate([tight, wide]), perm, meta)[:, 0].tolist() == [False, True]


def test_fused_loop_regimes():
    assert wc.wm_blocks_per_workgroup(777) == (1, 1)
    assert wc.wm_blocks_per_workgroup(64 * 3 * 2 + 17, cap=3) == (2, 3)
    assert wc.wm_blocks_per_workgroup(32768) == (1, 1) and wc.wm_blocks_per_workgroup(32769) == (1, 2)
    assert (65573 + 63) // 64 == 1025


def test_knn_forms():
    assert wc.knn_form(262144 + 300, 9, True) == "persistent" and wc.knn_form(262144, 9, True) == "one_chunk_per_workgroup"
    assert wc.knn_form(524288 + 300, 7, False) == "persistent" and wc.knn_form(524288, 7, False) == "one_chunk_per_workgroup"
    assert wc.knn_form(262144 + 300, 9, False) == "one_chunk_per_workgroup"
    assert wc.knn_form(3000, 256, True) == "one_chunk_per_workgroup" and wc.knn_form(3000, 257, True) == "restaged"
    assert wc.knn_form(10 ** 6, 301, True) == "restaged"


@pytest.mark.parametrize("hybrid", [False, True])
@pytest.mark.parametrize("K,nn,ties", wc.KNN_TIE_CASES)
def test_knn_tie_cases_have_one_answer(K, nn, ties, hybrid):
    xyz, feat, kp, kpf = wc.knn_inputs(3000, K, K + nn, ties=ties)
    idx, d2 = wc.knn_oracle(xyz, feat, kp, kpf, min(nn + 1, K), hybrid)
    full = np.concatenate([kp, kpf], 1) if hybrid else kp
    # equal distances among a point's nn + 1 nearest occur only between coincident keypoints, which come lower index first:
    # "ties go to the lower index" decides every one of them, the cut after the nn-th included
    eq = d2[:, 1:] == d2[:, :-1]
    assert eq.any()
    a, b = idx[:, :-1][eq], idx[:, 1:][eq]
    assert np.all(a < b) and np.array_equal(full[a], full[b])
    for lo, hi in ties:                                              # every constructed tie is seen, and is cut between its two
        rows = (idx[:, :nn] == lo).any(axis=1)
        assert rows.any(), (lo, hi)
        if nn > 1:
            assert ((idx[:, :nn - 1] == lo) & (idx[:, 1:nn] == hi)).any(), (lo, hi)
    if nn == 1:                                                      # the cut after the only neighbour falls between a tie's two
        assert any(((idx[:, 0] == lo) & (idx[:, 1] == hi)).any() for lo, hi in ties)
