"""CPU: tests/blend_ref.py itself -- the gather-form float64 reference against the dense restatement of the reference model
(oracle/deform_oracle.py fill_nearest / quat_mul, as test_gpu_deform.test_blend_forward_backward uses them), what the index
patterns promise (list lengths per 256-row chunk, counted in numpy), RTOL against a float32 restatement, and the teeth of the
per-element bound on the inputs of every case of tests/test_gpu_blend_direct.py at CPU scale."""
import numpy as np
import pytest
import torch

import blend_ref as BR
from blend_ref import spec
from oracle import deform_oracle as do
from test_gpu_blend_direct import ALL_SPECS, N_COH_UNI, N_LISTS

F = torch.nn.functional


def dense_reference(inp):
    """the blend as the reference model writes it: softmax weights scattered into [N, K], two matmuls (float64)."""
    nn_, norm = inp["nn"], inp["norm"]
    d64 = inp["delta"].double().requires_grad_(True)
    x64, r64 = inp["xyz"].double().requires_grad_(True), inp["rot"].double().requires_grad_(True)
    dq, dxyz = d64[:, 3:7], d64[:, 0:3]
    if norm:
        dq = F.normalize(dq)
    if nn_:
        w64 = inp["raw_w"].double().requires_grad_(True)
        wx, wr = do.fill_nearest(w64, inp["idx"], inp["K"], nn_)
        dq, dxyz = wr @ dq, wx @ dxyz
    xt = x64 + dxyz
    qt = F.normalize(do.quat_mul(F.normalize(dq), r64))
    ((xt * inp["gx"].double()).sum() + (qt * inp["gq"].double()).sum()).backward()
    out = {"xyz_t": xt, "q_t": qt, "g_delta": d64.grad, "g_xyz": x64.grad, "g_rot": r64.grad}
    if nn_:
        out["g_raw_w"] = w64.grad
    return {k: v.detach().numpy() for k, v in out.items()}


@pytest.mark.parametrize("od", [7, 8])
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("N,K,nn_", [(600, 100, 1), (577, 100, 6), (600, 97, 8), (513, 100, 16), (300, 16, 16), (600, 0, 0)])
def test_gather_reference_equals_the_dense_restatement(N, K, nn_, norm, od):
    inp = BR.make_inputs(spec("uniform" if nn_ else "stage1", N, K, nn_, od, norm))
    ref, dense = BR.blend_reference(inp), dense_reference(inp)
    for k, want in dense.items():
        scale = max(1.0, float(np.abs(want).max()))
        assert np.abs(ref[k] - want).max() <= 1e-13 * scale, k          # float64 round-off of sums of at most a few hundred terms
        if k != "g_xyz":
            A = ref["A_" + k]
            assert A.shape == want.shape and (A >= 0).all() and (np.abs(want)[..., :7] <= A[..., :7] * (1 + 1e-9) + 1e-300).all(), k


# ------------------------------------------------------------------------------------------------
# what the patterns promise
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nn_,K", [(1, 40), (6, 300), (8, 300), (16, 240)])
def test_threshold_chunk_holds_exactly_the_promised_lists(nn_, K):
    inp = BR.make_inputs(spec("threshold", N_LISTS, K, nn_))
    idx, meta = inp["idx"].numpy(), inp["meta"]
    BR.check_indices(idx, K)
    L = BR.list_lengths(idx, K)
    c = meta["chunk"]
    assert 0 < c and (c + 1) * BR.CHUNK <= N_LISTS
    assert tuple(L[c, meta["targets"]]) == BR.THRESH_LENGTHS == (1, 2, 19, 20, 21, 63, 64, 65)
    assert L[c, meta["empty"]] == 0
    assert L[c].sum() == BR.CHUNK * nn_
    # short path: an odd length (e1 = -1 in the two-at-a-time loop), an even one, exactly BB_LONG; long path: BB_LONG + 1, one
    # stride less one, exactly one stride, one stride and one
    assert BR.BB_LONG == 20 and (L[c] > BR.BB_LONG).sum() >= 4
    # every neighbour slot holds a target somewhere (the slot is part of the sorted entry)
    block = idx[c * BR.CHUNK:(c + 1) * BR.CHUNK]
    assert all(np.isin(block[:, j], meta["targets"]).any() for j in range(nn_))


@pytest.mark.parametrize("nn_,K", [(6, 300), (8, 300), (16, 240)])
def test_coherent_chunks_have_nn_lists_of_256(nn_, K):
    idx = BR.make_inputs(spec("coherent", N_LISTS, K, nn_))["idx"].numpy()
    L = BR.list_lengths(idx, K)
    for c, rows in enumerate((256, 256, N_LISTS - 512)):
        assert sorted(L[c][L[c] > 0]) == [rows] * nn_
        assert (L[c] > BR.BB_LONG).sum() == nn_
    # a keypoint sits in every slot of its chunk in turn
    assert all(len(set(idx[:nn_, j])) == nn_ for j in range(nn_))


@pytest.mark.parametrize("nn_,K", [(6, 300), (8, 300), (16, 240)])
def test_hot_keypoint_is_in_every_row(nn_, K):
    inp = BR.make_inputs(spec("hot", N_LISTS, K, nn_))
    idx, hot = inp["idx"].numpy(), inp["meta"]["hot"]
    L = BR.list_lengths(idx, K)
    assert list(L[:, hot]) == [256, 256, N_LISTS - 512]
    assert all((idx[:, j] == hot).any() for j in range(nn_))
    assert np.delete(L, hot, axis=1).max() < 64          # the rest stays random


@pytest.mark.parametrize("nn_", [6, 8, 16])
def test_k_equal_nn_rows_are_permutations(nn_):
    idx = BR.make_inputs(spec("perm", N_LISTS, nn_, nn_))["idx"].numpy()
    assert (np.sort(idx, axis=1) == np.arange(nn_)).all() and len({tuple(r) for r in idx}) > nn_
    L = BR.list_lengths(idx, nn_)
    assert (L[:2] == 256).all() and (L[2] == N_LISTS - 512).all()


def test_uniform_rows_on_the_shipped_shape_have_no_long_list():
    L = BR.list_lengths(BR.make_inputs(spec("uniform", N_LISTS, 300, 6))["idx"].numpy(), 300)
    assert L.max() <= BR.BB_LONG and (L == 0).any() and (L[:2] % 2 == 1).any()


@pytest.mark.parametrize("nn_,K", [(6, 300), (8, 300), (16, 240)])
def test_coherent_then_uniform_chunks(nn_, K):
    """at full size: workgroup 0 sees nlong = nn, then 0; workgroup 1 sees 0, then nn (index rows alone: no reference here)."""
    rng = np.random.default_rng(nn_)
    idx = BR.coherent_then_uniform_rows(rng, N_COH_UNI, K, nn_)
    L = BR.list_lengths(idx, K)
    nlong = (L > BR.BB_LONG).sum(axis=1)
    P = BR.MAX_BLOCKS
    assert L.shape[0] == P + 2
    assert (nlong[0], nlong[P], nlong[1], nlong[P + 1]) == (nn_, 0, 0, nn_)
    assert L[0].max() == 256 and L[P + 1].max() == 256
    small = BR.make_inputs(BR.cpu_scale(spec("coh_uni", N_COH_UNI, K, nn_)))
    nl = (BR.list_lengths(small["idx"].numpy(), K) > BR.BB_LONG).sum(axis=1)
    assert tuple(nl) == (nn_, 0, nn_)


def test_builders_refuse_duplicates_and_out_of_range():
    ok = np.array([[0, 1, 2], [2, 0, 1]], dtype=np.int64)
    BR.check_indices(ok, 3)
    for bad, K in ((np.array([[0, 1, 1]], dtype=np.int64), 3), (np.array([[0, 1, 3]], dtype=np.int64), 3), (np.array([[-1, 1, 2]], dtype=np.int64), 3)):
        with pytest.raises(AssertionError):
            BR.check_indices(bad, K)


def test_largest_keypoint_counts_follow_the_lds_expression():
    for (nn_, od), K in (((6, 7), 632), ((8, 8), 525), ((16, 8), 241)):       # (as DESIGN.md states them)
        assert BR.max_keypoints(nn_, od) == K
        assert BR.bwd_lds_bytes(K, nn_, od) <= 64 * 1024 < BR.bwd_lds_bytes(K + 1, nn_, od)


# ------------------------------------------------------------------------------------------------
# RTOL and the teeth of the bound, on every GPU case's inputs at CPU scale
# ------------------------------------------------------------------------------------------------
CPU_SPECS = sorted({BR.cpu_scale(sp) for sp in ALL_SPECS})
_refs = {}


def _ref(sp):
    if sp not in _refs:
        inp = BR.make_inputs(sp)
        _refs[sp] = (inp, BR.blend_reference(inp))
    return _refs[sp]


def _compared(ref, inp):
    """(name, want, A) of every compared output; the zero-quaternion keypoint's gradient row is left out, as on the GPU."""
    for k in BR.COMPARED:
        if k in ref:
            want, A = ref[k], ref["A_" + k]
            if k == "g_delta" and "zero_kp" in inp["meta"]:
                keep = np.arange(want.shape[0]) != inp["meta"]["zero_kp"]
                want, A = want[keep], A[keep]
            yield k, want, A


def test_rtol_is_four_times_the_float32_restatement():
    worst = {}
    for sp in CPU_SPECS:
        inp, ref = _ref(sp)
        f32 = BR.blend_reference(inp, dtype=torch.float32, magnitudes=False)
        for k, want, A in _compared(ref, inp):
            got = f32[k]
            if k == "g_delta" and "zero_kp" in inp["meta"]:
                got = got[np.arange(got.shape[0]) != inp["meta"]["zero_kp"]]
            assert np.isfinite(want).all(), (sp, k)
            worst[k] = max(worst.get(k, 0.0), BR.worst_ratio(got, want, A))
    print("float32 restatement, worst err / A:", {k: f"{v:.3g}" for k, v in worst.items()})
    measured = max(worst.values())
    assert 4 * measured <= BR.RTOL <= 8 * measured, (measured, BR.RTOL)


def _rejected(pert, ref, inp):
    """does the per-element bound, with the final RTOL, refuse `pert` as an answer for `ref`?"""
    zk = inp["meta"].get("zero_kp")
    for k, want, A in _compared(ref, inp):
        got = np.delete(pert[k], zk, axis=0) if (k == "g_delta" and zk is not None) else pert[k]
        if not BR.within_bound(got, want, A):
            return True
    return False


@pytest.mark.parametrize("sp", [s for s in CPU_SPECS if s.nn], ids=lambda s: "-".join(map(str, s)))
def test_bound_rejects_a_dropped_term_swapped_weights_and_a_shifted_row(sp):
    inp, ref = _ref(sp)
    N, K, nn_ = sp.N, sp.K, sp.nn
    idx = inp["idx"].numpy()
    assert not _rejected(ref, ref, inp)
    # (1) one (Gaussian, neighbour) term dropped from one keypoint's sum: the keypoint with the most terms, its median term
    kp = int(np.bincount(idx.reshape(-1), minlength=K).argmax())
    if kp == inp["meta"].get("zero_kp"):
        kp = int(np.bincount(idx.reshape(-1), minlength=K).argsort()[-2])
    rows, slots = np.nonzero(idx == kp)
    wx = torch.softmax(inp["raw_w"].double()[:, :nn_], dim=-1).numpy()
    term = wx[rows, slots, None] * inp["gx"].double().numpy()[rows]          # what each entry adds to g_delta[kp, 0:3]
    drop = int(np.argsort(np.abs(term).max(axis=1))[len(rows) // 2])
    pert = dict(ref)
    pert["g_delta"] = ref["g_delta"].copy()
    pert["g_delta"][kp, 0:3] -= term[drop]
    assert not BR.within_bound(pert["g_delta"][kp, 0:3], ref["g_delta"][kp, 0:3], ref["A_g_delta"][kp, 0:3]), "a dropped term passes"
    # (2) wx and wr swapped for one row
    i = N // 3
    swapped = dict(inp)
    swapped["raw_w"] = inp["raw_w"].clone()
    swapped["raw_w"][i] = torch.cat([inp["raw_w"][i, nn_:], inp["raw_w"][i, :nn_]])
    if nn_ > 1 and not torch.equal(swapped["raw_w"][i], inp["raw_w"][i]):
        assert _rejected(BR.blend_reference(swapped, magnitudes=False), ref, inp), "swapped weight halves pass"
    # (3) one row's indices shifted by one (the whole row, modulo K: it stays distinct)
    moved = dict(inp)
    moved["idx"] = inp["idx"].clone()
    moved["idx"][i] = (inp["idx"][i] + 1) % K
    if K > nn_:                      # (K = nn: the shifted row is another permutation of every keypoint -- the slots change, the set does not)
        assert sorted(moved["idx"][i].tolist()) != sorted(inp["idx"][i].tolist())
    assert _rejected(BR.blend_reference(moved, magnitudes=False), ref, inp), "a shifted index row passes"
