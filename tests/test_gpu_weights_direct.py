"""The kernels of csrc/weights_kernels.hip in the regimes production runs them in, each against oracle/weights_oracle.py:
dense levels with resolutions that are no power of two, the LDS box of the table gradient (boxed and unboxed workgroups in one
launch), the persistent loops of the fused kernels, every masked n_out, and the kNN kernel at odd and ragged keypoint counts,
ties, restaged tiles and its staged-once persistent form.  tests/weights_cases.py builds the inputs and restates the regime
predicates; test_weights_cases_host.py checks those on the CPU.  parity unpinned, as in test_gpu_weights.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import weights_cases as wc  # noqa: E402
from gaussianprediction_amd import _lib  # noqa: E402
from gaussianprediction_amd.weights_ops import WeightsModel, _HashGridEncode, knn_keypoints, morton_order  # noqa: E402
from oracle import weights_oracle as wo  # noqa: E402


def _model(log2_T, n_out, params=None):
    m = WeightsModel(n_out, n_levels=16, log2_hashmap_size=log2_T, base_resolution=16, seed=7, device="cuda")
    if params is not None:
        assert m.params.numel() == params.size
        with torch.no_grad():
            m.params.copy_(torch.from_numpy(np.array(params)))
    return m


# ---- A. encoding, bit for bit ---------------------------------------------------------------------------------------
# T = 19 is the production grid (6 098 120 entries, five dense levels): one case
@pytest.mark.parametrize("log2_T,n,with_perm", [(t, n, p) for t in (12, 15, 17) for n in (1, 63, 64, 65, 513) for p in (False, True)]
                         + [(19, 513, True)])
def test_encoding_bit_exact_on_dense_levels(log2_T, n, with_perm):
    meta = wc.grid(log2_T)
    m = _model(log2_T, 12)
    assert m.table_entries == meta["total"]
    rng = np.random.default_rng(100 * log2_T + n)
    xyz = torch.from_numpy(wc.points_with_edges(n, meta, n, half=3.0))
    table = torch.from_numpy(rng.normal(size=(meta["total"], 4)).astype(np.float32))
    perm = torch.from_numpy(rng.permutation(n).astype(np.int32)).cuda() if with_perm else None
    enc = _HashGridEncode.apply(xyz.cuda(), table.cuda(), m.cfg, perm).cpu().numpy()
    ref = wo.hash_encode(xyz, table, meta).numpy()
    bad = np.argwhere(enc != ref)
    assert np.array_equal(enc, ref), f"first mismatch (point, feature) {bad[0]}, level {bad[0][1] // 4}, {len(bad)} in all"


# ---- B. fused forward ------------------------------------------------------------------------------------------------
def _forward_case(log2_T, n_out, n, kind, seed):
    meta = wc.grid(log2_T)
    xyz = wc.case_points(kind, n, meta, seed)
    params = wc.model_params(meta, seed + 1)
    ref = wo.weights_model(torch.from_numpy(xyz).double(), torch.from_numpy(params).double(), meta, n_out).numpy()
    return _model(log2_T, n_out, params), torch.from_numpy(xyz).cuda(), ref


def _meets_forward_bar(out, ref):
    err = np.abs(out.astype(np.float64) - ref).max()
    assert err < 2e-4 * max(1.0, float(np.abs(ref).max())), err


@pytest.mark.parametrize("n_out,n", [(1, 777), (12, 777), (13, 777), (16, 777), (16, 1), (16, 63), (16, 64), (16, 65), (16, 4097)])
def test_fused_forward_matches_oracle(n_out, n):
    m, xyz, ref = _forward_case(15, n_out, n, "edges", 1000 * n_out + n)
    with torch.no_grad():
        out = m(xyz)
    assert out.shape == (n, n_out)
    assert (m._perm is not None) == (n > 4096)               # 4097: the first n that goes through a Morton permutation
    _meets_forward_bar(out.cpu().numpy(), ref)


def test_fused_forward_multi_block_loop_small():
    """Three workgroups walk two or three 64-point blocks each (the last one ragged): same bits as one block per workgroup."""
    n = 64 * 3 * 2 + 17
    assert wc.wm_blocks_per_workgroup(n, cap=3) == (2, 3) and wc.wm_blocks_per_workgroup(n) == (1, 1)
    m, xyz, ref = _forward_case(15, 13, n, "edges", 5)
    perm = morton_order(xyz)
    from gaussianprediction_amd.weights_ops import _WeightsModelFused
    outs = {}
    for pm in (None, perm):
        with torch.no_grad():
            outs[pm is None, 0] = _WeightsModelFused.apply(xyz, m.params, m.cfg, 13, pm).cpu().numpy()
            try:
                _lib.check(_lib.lib().gp_debug_option(4, 3), "gp_debug_option")
                outs[pm is None, 3] = _WeightsModelFused.apply(xyz, m.params, m.cfg, 13, pm).cpu().numpy()
            finally:
                _lib.check(_lib.lib().gp_debug_option(4, 0), "gp_debug_option")
        assert np.array_equal(outs[pm is None, 3], outs[pm is None, 0])
        _meets_forward_bar(outs[pm is None, 3], ref)
    assert np.array_equal(outs[True, 0], outs[False, 0])    # the permutation only regroups the points


def test_fused_forward_default_cap():
    """1025 blocks on 512 workgroups, clustered points in the model's own Morton order."""
    n = 65573
    assert wc.wm_blocks_per_workgroup(n) == (2, 3)
    m, xyz, ref = _forward_case(15, 16, n, "clustered", 65589)
    with torch.no_grad():
        out = m(xyz)
    _meets_forward_bar(out.cpu().numpy(), ref)


# ---- C. fused backward -----------------------------------------------------------------------------------------------
# float32-oracle yardsticks (rel-L2 of the float32 CPU oracle against the float64 one), the largest measured over the tensors
# of a case and over two hosts (they vary in the last digit with the host's BLAS and thread count):
#   n = 300: W 3.9e-7, table levels 2.1e-7;  n = 4097 (T = 17): W 3.2e-7, levels 1.9e-7;  n = 65573: W 4.5e-7, levels 2.0e-7
# (max-abs relative to the tensor's largest gradient: at most 7.3e-7).  Four times any of them is below 1e-5, so every bar
# is the existing 1e-5 (wc.bar; test_weights_cases_host.py asserts that this is what it evaluates to).  The kernels measured
# at most 4.9e-7 rel-L2 and 9.3e-7 max-abs (n = 65573, the weight matrices).
@pytest.mark.parametrize("name", list(wc.BACKWARD_CASES))
def test_fused_backward_matches_f64_autograd(name):
    r = wc.backward_reference(name)
    meta, n, n_out = r["meta"], r["n"], r["n_out"]
    m = _model(r["log2_T"], n_out, r["params"])
    xyz = torch.from_numpy(np.array(r["xyz"])).cuda()
    assert r["excluded"] * 100 <= n                          # AMBIGUOUS_CAP, in whole rows
    out = m(xyz)
    (out * torch.from_numpy(np.array(r["gy"])).cuda()).sum().backward()
    g = m.params.grad.cpu().numpy()
    # the launch really was what the case is named for
    perm = m._perm.cpu().numpy() if n > 4096 else None
    assert (m._perm is not None) == (n > 4096)
    bm = wc.boxed_map(r["xyz"], perm, meta)
    assert bm.any(axis=0).all() and (~bm).any(axis=0).all(), bm.mean(axis=0)
    if name.startswith("persistent_mixed"):
        assert wc.wm_blocks_per_workgroup(n) == (2, 3)
    # rows of the padded output layer at n_out and beyond: exactly zero
    assert np.all(g[8192 + n_out * 64: wc.MLP_FLOATS] == 0)
    err = wc.errors(g, r["grad"], meta)
    for k, (rel, mx) in err.items():
        print(f"{name} {k}: rel-L2 {rel:.3e} (float32 oracle {r['yardstick'][k][0]:.3e})  max-abs {mx:.3e} ({r['yardstick'][k][1]:.3e})")
    failed = {k: (rel, mx) for k, (rel, mx) in err.items()
              if not (rel < wc.bar(r["yardstick"][k][0]) and mx < wc.bar(r["yardstick"][k][1]))}
    assert not failed, failed


# ---- D. kNN ----------------------------------------------------------------------------------------------------------
def _knn_check(xyz, feat, kp, kpf, nn, hybrid, order=None, ref=None):
    t = lambda a: torch.from_numpy(a).cuda()
    idx, d2 = knn_keypoints(t(xyz), t(kp), nn, t(feat), t(kpf), 5.0, "hybird" if hybrid else "3D", return_dist=True, order=order)
    ri, rd = ref if ref is not None else wc.knn_oracle(xyz, feat, kp, kpf, nn, hybrid)
    gi = idx.cpu().numpy()
    bad = np.argwhere(gi != ri)
    assert np.array_equal(gi, ri), f"{len(bad)} indices differ, first at (point, rank) {bad[0]}: {gi[tuple(bad[0])]} != {ri[tuple(bad[0])]}"
    assert np.array_equal(d2.cpu().numpy(), rd)
    assert kp.shape[0] < 65536
    assert np.array_equal(idx._gp_idx16[1].cpu().numpy().astype(np.int64) & 0xFFFF, ri)     # the blend kernels' packed copy
    return ri, rd


@pytest.mark.parametrize("hybrid", [False, True])
@pytest.mark.parametrize("K,nn", [(7, 7), (9, 1), (16, 16), (255, 6), (256, 6), (257, 8), (301, 5), (513, 2)])
def test_knn_odd_and_ragged_keypoint_counts(K, nn, hybrid):
    _knn_check(*wc.knn_inputs(3000, K, 10 * K + nn), nn, hybrid)


@pytest.mark.parametrize("hybrid", [False, True])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_knn_small_point_counts(n, hybrid):
    xyz, feat, kp, kpf = wc.knn_inputs(n, 9, n)
    _knn_check(xyz, feat, kp, kpf, 6, hybrid)
    order = torch.from_numpy(np.random.default_rng(n).permutation(n).astype(np.int32)).cuda()
    _knn_check(xyz, feat, kp, kpf, 6, hybrid, order=order)


@pytest.mark.parametrize("hybrid", [False, True])
@pytest.mark.parametrize("K,nn,ties", wc.KNN_TIE_CASES)
def test_knn_ties_go_to_the_lower_index(K, nn, ties, hybrid):
    _knn_check(*wc.knn_inputs(3000, K, K + nn, ties=ties), nn, hybrid)


@pytest.mark.parametrize("feat_scale", [1e-3, 1.0])
def test_knn_order_with_restaged_tiles(feat_scale):
    """`order` (early drop of keypoints per wavefront) together with K > 256 (tiles restaged per chunk), ragged last chunk."""
    n, K, nn = 3000, 301, 5
    assert wc.knn_form(n, K, True) == "restaged"
    xyz, feat, kp, kpf = wc.knn_inputs(n, K, 77, feat_scale=feat_scale, ties=((255, 256), (299, 300)))
    ref = _knn_check(xyz, feat, kp, kpf, nn, True)
    rnd = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(torch.int32).cuda()
    for order in (morton_order(torch.from_numpy(xyz).cuda()), rnd):
        _knn_check(xyz, feat, kp, kpf, nn, True, order=order, ref=ref)


@pytest.mark.parametrize("hybrid,n,K,nn", [(True, 262144 + 300, 9, 6), (False, 524288 + 300, 7, 7)])
def test_knn_persistent_form(hybrid, n, K, nn):
    """More chunks than resident workgroups: keypoints staged on a workgroup's first chunk only, later chunks reuse LDS."""
    assert wc.knn_form(n, K, hybrid) == "persistent"
    xyz, feat, kp, kpf = wc.knn_inputs(n, K, K, ties=((2, 3),))
    if not hybrid:
        feat = feat[:1]                                       # (unused in 3-D; keeps the upload small)
    ref = _knn_check(xyz, feat, kp, kpf, nn, hybrid)
    _knn_check(xyz, feat, kp, kpf, nn, hybrid, order=morton_order(torch.from_numpy(xyz).cuda()), ref=ref)
