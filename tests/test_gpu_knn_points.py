"""GPU: gp_knn_points / gp_knn_points_backward (csrc/knn_kernels.hip) through gaussianprediction_amd.knn_ops and the pytorch3d / frnn
shims, against a brute-force numpy oracle computed here: fp32 distances summed in dimension order (the kernel's arithmetic), neighbours
ordered by (distance, index)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dist_rows(q, c, norm):
    """[len(q), len(c)] fp32 distances, summed over the dimensions in order."""
    s = np.zeros((q.shape[0], c.shape[0]), np.float32)
    for d in range(q.shape[1]):
        df = q[:, None, d] - c[None, :, d]
        s = s + (df * df if norm == 2 else np.abs(df))
    return s


def oracle(q, c, K, norm, rows=None, chunk=256):
    """(sorted distances [R, K+1] (inf-padded), indices [R, K+1] (-1 padded)) of the query rows `rows` (default all)."""
    rows = np.arange(q.shape[0]) if rows is None else rows
    od = np.full((len(rows), K + 1), np.inf, np.float32)
    oi = np.full((len(rows), K + 1), -1, np.int64)
    n = min(K + 1, c.shape[0])
    for r0 in range(0, len(rows), chunk):
        r = rows[r0:r0 + chunk]
        if n == 0:
            continue
        d = _dist_rows(q[r], c, norm)
        o = np.argsort(d, axis=1, kind="stable")[:, :n]
        od[r0:r0 + len(r), :n] = np.take_along_axis(d, o, 1)
        oi[r0:r0 + len(r), :n] = o
    return od, oi


def check_rows(dist, idx, rd, ri, K, pad_idx, pad_dist, r2_max=math.inf):
    """dist/idx [R, K] from the kernel against the oracle's rows."""
    real = np.isfinite(rd[:, :K]) & (rd[:, :K] <= r2_max)
    assert np.array_equal(idx[~real], np.full((~real).sum(), pad_idx)), "padding index"
    assert np.array_equal(dist[~real], np.full((~real).sum(), pad_dist, np.float32)), "padding distance"
    ref = rd[:, :K][real]
    assert np.all(np.abs(dist[real] - ref) <= 1e-6 * np.maximum(np.abs(ref), 1e-30)), "distances"
    # indices exact wherever the distance is separated from both neighbours in the order by more than 1e-5 relative
    full = np.concatenate([np.full((rd.shape[0], 1), -np.inf, np.float32), rd], 1)
    lo, mid, hi = full[:, :K], full[:, 1:K + 1], full[:, 2:K + 2]
    tol = 1e-5 * np.maximum(np.abs(mid), 1e-30)
    with np.errstate(invalid="ignore"):                  # (inf - inf in padded slots: not separated, not checked)
        sep = real & (mid - lo > tol) & (hi - mid > tol)
    assert sep.sum() >= 0.5 * real.sum(), "too few unambiguous slots to check"
    assert np.array_equal(idx[sep], ri[:, :K][sep]), "indices"


def _lengths(rng, B, P):
    return np.array([P] + [int(rng.integers(P // 3, P + 1)) for _ in range(B - 1)], np.int64)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("D", [3, 5, 35])
@pytest.mark.parametrize("K", [1, 6, 21, 32])
@pytest.mark.parametrize("norm", [1, 2])
def test_knn_points_small(B, D, K, norm):
    from gaussianprediction_amd.knn_ops import knn_points
    rng = np.random.default_rng(1000 * B + 10 * D + K + norm)
    P1, P2 = 150, 200
    p1 = rng.normal(size=(B, P1, D)).astype(np.float32)
    p2 = rng.normal(size=(B, P2, D)).astype(np.float32)
    p2[:, 7] = p2[:, 3]                      # a duplicate candidate: ties go to the lower index
    p1[:, 5] = p2[:, 3]                      # a query on a candidate: distance exactly 0
    l1 = _lengths(rng, B, P1) if B > 1 else None
    l2 = _lengths(rng, B, P2) if B > 1 else None
    if B > 1:
        l2[-1] = K // 2                      # fewer candidates than K: padded slots
    t1, t2 = torch.tensor(p1, device=DEV), torch.tensor(p2, device=DEV)
    tl1 = torch.tensor(l1, device=DEV) if l1 is not None else None
    tl2 = torch.tensor(l2, device=DEV) if l2 is not None else None
    outs = {s: knn_points(t1, t2, tl1, tl2, K=K, norm=norm, splits=s, pad_idx=-1, pad_dist=-1.0) for s in (1, 7, 0)}
    d1, i1 = outs[1]
    for s in (7, 0):
        assert torch.equal(outs[s][0], d1) and torch.equal(outs[s][1], i1), f"splits={s} differs from splits=1"
    d1, i1 = d1.cpu().numpy(), i1.cpu().numpy()
    for b in range(B):
        n1 = P1 if l1 is None else l1[b]
        n2 = P2 if l2 is None else l2[b]
        rd, ri = oracle(p1[b, :n1], p2[b, :n2], K, norm)
        check_rows(d1[b, :n1], i1[b, :n1], rd, ri, K, -1, -1.0)
        assert np.all(i1[b, n1:] == -1) and np.all(d1[b, n1:] == -1.0), "rows beyond lengths1"
        if n2 > 3:
            assert i1[b, 5, 0] == 3 and d1[b, 5, 0] == 0.0, "a query on a candidate"
            if n2 > 7 and K > 1:
                assert list(i1[b, 5, :2]) == [3, 7] and d1[b, 5, 0] == 0.0 and d1[b, 5, 1] == 0.0


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("D", [3, 35])
def test_knn_points_backward(norm, D):
    from gaussianprediction_amd.knn_ops import knn_points
    rng = np.random.default_rng(7 + norm + D)
    B, P1, P2, K = 3, 90, 120, 6
    p1 = torch.tensor(rng.normal(size=(B, P1, D)).astype(np.float32), device=DEV, requires_grad=True)
    p2 = torch.tensor(rng.normal(size=(B, P2, D)).astype(np.float32), device=DEV, requires_grad=True)
    l1 = torch.tensor([P1, 50, 70], device=DEV)
    l2 = torch.tensor([P2, 4, 100], device=DEV)          # batch 1: fewer candidates than K
    w = torch.tensor(rng.normal(size=(B, P1, K)).astype(np.float32), device=DEV)
    for pad in (0, -1):                                # pytorch3d's and frnn's padding: neither reaches the gradient
        p1.grad = p2.grad = None
        dists, idx = knn_points(p1, p2, l1, l2, K=K, norm=norm, pad_idx=pad, pad_dist=float(pad))
        (dists * w).sum().backward()
        valid = torch.zeros(B, P1, K, dtype=torch.bool, device=DEV)
        for b in range(B):
            valid[b, :int(l1[b]), :min(K, int(l2[b]))] = True
        a = p1.detach().double().requires_grad_(True)
        c = p2.detach().double().requires_grad_(True)
        g = torch.gather(c[:, None].expand(B, P1, P2, D), 2, idx.clamp_min(0)[..., None].expand(B, P1, K, D))
        df = a[:, :, None] - g
        ref = (df * df).sum(-1) if norm == 2 else df.abs().sum(-1)
        assert torch.allclose(ref[valid].float(), dists[valid], rtol=1e-5, atol=1e-6)
        (ref * w.double() * valid).sum().backward()
        for got, want in ((p1.grad, a.grad), (p2.grad, c.grad)):
            err = (got.double() - want).abs().max() / want.abs().max()
            assert err < 1e-5, f"pad={pad}: gradient error {err}"


def test_shim_padding_and_radius():
    from frnn import frnn_grid_points
    from pytorch3d.ops import knn_points
    rng = np.random.default_rng(3)
    B, P1, P2, K = 2, 300, 250, 8
    p1 = rng.uniform(size=(B, P1, 3)).astype(np.float32)
    p2 = rng.uniform(size=(B, P2, 3)).astype(np.float32)
    l2 = np.array([P2, 5], np.int64)
    t1, t2, tl2 = torch.tensor(p1, device=DEV), torch.tensor(p2, device=DEV), torch.tensor(l2, device=DEV)
    res = knn_points(t1, t2, lengths2=tl2, K=K, return_nn=True)
    assert len(res) == 3 and res.knn.shape == (B, P1, K, 3)
    r = 0.1
    dists, idxs, nn, grid = frnn_grid_points(t1, t2, lengths2=tl2, K=K, r=r, return_nn=True)
    d2, i2, _, _ = frnn_grid_points(t1, t2, lengths2=tl2, K=K, r=r, grid=grid)
    assert torch.equal(d2, dists) and torch.equal(i2, idxs)
    for b in range(B):
        rd, ri = oracle(p1[b], p2[b, :l2[b]], K, 2)
        check_rows(res.dists[b].cpu().numpy(), res.idx[b].cpu().numpy(), rd, ri, K, 0, 0.0)
        check_rows(dists[b].cpu().numpy(), idxs[b].cpu().numpy(), rd, ri, K, -1, -1.0, r2_max=np.float32(r * r))
        cut = (rd[:, :K] > np.float32(r * r)) & np.isfinite(rd[:, :K])
        assert cut.any() and (~cut & np.isfinite(rd[:, :K])).any(), "the radius must cut some neighbours and keep others"
        gathered = p2[b][np.clip(res.idx[b].cpu().numpy(), 0, None)]
        gathered[res.idx[b].cpu().numpy() >= l2[b]] = 0
        assert np.array_equal(res.knn[b].cpu().numpy()[:, :min(K, l2[b])], gathered[:, :min(K, l2[b])])
        assert np.all(res.knn[b].cpu().numpy()[:, min(K, l2[b]):] == 0)


def test_pointops_knnquery_shim():
    import pointops_cuda
    rng = np.random.default_rng(5)
    n_b, m_b = [400, 3, 250], [40, 20, 30]
    xyz = torch.tensor(rng.normal(size=(sum(n_b), 3)).astype(np.float32), device=DEV)
    new_xyz = torch.tensor(rng.normal(size=(sum(m_b), 3)).astype(np.float32), device=DEV)
    off = torch.tensor(np.cumsum(n_b), dtype=torch.int32, device=DEV)
    noff = torch.tensor(np.cumsum(m_b), dtype=torch.int32, device=DEV)
    K = 5
    idx = torch.zeros(sum(m_b), K, dtype=torch.int32, device=DEV)
    dist2 = torch.zeros(sum(m_b), K, device=DEV)
    pointops_cuda.knnquery_cuda(sum(m_b), K, xyz, new_xyz, off, noff, idx, dist2)
    x, nx = xyz.cpu().numpy(), new_xyz.cpu().numpy()
    s0 = q0 = 0
    for nb, mb in zip(n_b, m_b):
        rd, ri = oracle(nx[q0:q0 + mb], x[s0:s0 + nb], K, 2)
        ri = np.where(ri >= 0, ri + s0, ri)
        got_i = idx[q0:q0 + mb].cpu().numpy().astype(np.int64)
        got_d = dist2[q0:q0 + mb].cpu().numpy()
        check_rows(got_d, got_i, rd, ri, K, s0, np.float32(1e10))
        s0, q0 = s0 + nb, q0 + mb


def _splits_identical(t1, t2, K, expect_split):
    from gaussianprediction_amd.knn_ops import knn_points
    ref = knn_points(t1, t2, K=K, splits=1)
    for s in (7, 0):
        out = knn_points(t1, t2, K=K, splits=s)
        assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1]), f"splits={s}"
    return ref


def test_reference_shape_keypoint_growth():
    """get_new_kpts [REF scene/gaussian_model.py:208]: ~300 new keypoints against 1e6 Gaussians, K = 1."""
    rng = np.random.default_rng(11)
    c = rng.uniform(-1, 1, size=(1, 1_000_000, 3)).astype(np.float32)
    q = c[:, rng.choice(1_000_000, 300, replace=False)] + rng.normal(scale=1e-3, size=(1, 300, 3)).astype(np.float32)
    d, i = _splits_identical(torch.tensor(q, device=DEV), torch.tensor(c, device=DEV), 1, True)
    rd, ri = oracle(q[0], c[0], 1, 2, chunk=8)
    check_rows(d[0].cpu().numpy(), i[0].cpu().numpy(), rd, ri, 1, 0, 0.0)


def test_reference_shape_iso_loss():
    """iso_loss [REF utils/loss_utils.py:36]: 2e4 points against themselves, K = k + 1 = 21."""
    rng = np.random.default_rng(12)
    p = rng.uniform(-1, 1, size=(1, 20_000, 3)).astype(np.float32)
    t = torch.tensor(p, device=DEV)
    d, i = _splits_identical(t, t, 21, False)
    rows = rng.choice(20_000, 1500, replace=False)
    rd, ri = oracle(p[0], p[0], 21, 2, rows=rows)
    check_rows(d[0].cpu().numpy()[rows], i[0].cpu().numpy()[rows], rd, ri, 21, 0, 0.0)
    assert torch.equal(i[0, :, 0], torch.arange(20_000, device=DEV)) and torch.all(d[0, :, 0] == 0)   # every point finds itself first


def test_reference_shape_gaussians_to_keypoints():
    """get_nearest_mask, knn_type "3D" [REF scene/gaussian_model.py:113]: 1e6 Gaussians against 512 keypoints, K = 8; the indices
    equal gp_knn_keypoints' wherever the order is unambiguous."""
    from gaussianprediction_amd.weights_ops import knn_keypoints
    rng = np.random.default_rng(13)
    x = rng.uniform(-1, 1, size=(1_000_000, 3)).astype(np.float32)
    kp = rng.uniform(-1, 1, size=(512, 3)).astype(np.float32)
    tx, tk = torch.tensor(x, device=DEV), torch.tensor(kp, device=DEV)
    d, i = _splits_identical(tx[None], tk[None], 8, False)
    ik = knn_keypoints(tx, tk, 8, knn_type="3D").cpu().numpy()
    rows = rng.choice(1_000_000, 20_000, replace=False)
    rd, ri = oracle(x, kp, 8, 2, rows=rows)
    check_rows(d[0].cpu().numpy()[rows], i[0].cpu().numpy()[rows], rd, ri, 8, 0, 0.0)
    check_rows(d[0].cpu().numpy()[rows], ik[rows], rd, ri, 8, 0, 0.0)


def test_refusals():
    from gaussianprediction_amd import _lib
    from gaussianprediction_amd.knn_ops import knn_points
    a = torch.zeros(1, 4, 65, device=DEV)
    with pytest.raises(_lib.GpHipError, match="D = 65"):
        knn_points(a, a, K=1)
    b = torch.zeros(1, 40, 3, device=DEV)
    with pytest.raises(_lib.GpHipError, match="K = 33"):
        knn_points(b, b, K=33)
    with pytest.raises(_lib.GpHipError, match="norm"):
        knn_points(b, b, K=1, norm=3)
