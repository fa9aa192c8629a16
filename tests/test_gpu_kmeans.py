"""The device k-means (include/gp_kmeans.h through gaussianprediction_amd.kmeans_ops, the model's opt-in and the two import shims)
against the float64 restatement of tests/kmeans_ref.py.

Ids are compared on the rows that are not `ambiguous` (kmeans_ref.ambiguous_rows: second-best and best distance within 1e-4 relative
in float64; fp32 accumulation of D <= 64 non-negative terms errs by about 2 D 2^-24 = 8e-6), and the share of rows left out is
asserted to be at most 0.5 % on the reference itself.  The shapes are the smallest at which each mechanism can go wrong: one row, less
than a wave, a batch and one row, several workgroups, D = 35 (padded to 36) and 64, K = 1024 at D = 64 (the centres pass through LDS
in tiles, and so does the table of sums)."""
import functools
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

import kmeans_ref as R  # noqa: E402
import gaussianprediction_amd as gpa  # noqa: E402
from gaussianprediction_amd import kmeans_ops as KM  # noqa: E402
from gaussianprediction_amd.scene_synth import SceneSpec, make_gaussians  # noqa: E402
from gaussianprediction_amd.training import default_training_args, kmeans as training_kmeans  # noqa: E402

DEV = "cuda"
IDS = [f"N{n}-K{k}-D{d}" for n, k, d, _ in R.SHAPES]


@functools.lru_cache(maxsize=None)
def case(n, k, d, kind):
    """One input and its float64 reference, computed once and shared (read-only)."""
    X, centres = R.make_input(n, k, d, kind)
    ids, d2 = R.assign(X, centres)
    amb = R.ambiguous_rows(X, centres)
    return SimpleNamespace(X=X, centres=centres, Xd=X.to(DEV), cd=centres.to(DEV), ids=ids, d2=d2, clear=~amb, left_out=float(amb.double().mean()))


def close(got, want, tol):
    """|got - want| <= tol * max(1, |want|), elementwise, against a float64 reference."""
    got, want = got.detach().double().cpu(), want.double().cpu()
    err = ((got - want).abs() / want.abs().clamp_min(1.0)).max() if want.numel() else torch.tensor(0.0)
    return float(err) <= tol, float(err)


# ---- assign ----
@pytest.mark.parametrize("n,k,d,kind", R.SHAPES, ids=IDS)
def test_assign_equals_the_float64_argmin(n, k, d, kind):
    c = case(n, k, d, kind)
    assert c.left_out <= R.AMBIGUOUS_CAP, c.left_out
    ids, d2 = KM.assign(c.Xd, c.cd, return_d2=True)
    assert ids.dtype == torch.int64 and ids.shape == (n,) and d2.shape == (n,)
    ids = ids.cpu()
    print(f"rows left out {c.left_out:.5f}; ids that differ on the others: {int((ids != c.ids)[c.clear].sum())}")
    assert torch.equal(ids[c.clear], c.ids[c.clear])
    assert bool(((ids >= 0) & (ids < k)).all())
    ok, err = close(d2, c.d2, 1e-5)
    print(f"d2: largest error {err:.3e}")
    assert ok, err
    assert torch.equal(KM.assign(c.Xd, c.cd), ids.to(DEV))             # without d2: the same ids


def test_assign_duplicate_centres_go_to_the_lower_index():
    c = case(5000, 150, 35, "model")
    twice = torch.cat([c.cd, c.cd])                                      # centre k + 150 equals centre k
    ids = KM.assign(c.Xd, twice)
    assert int(ids.max()) < 150 and torch.equal(ids, KM.assign(c.Xd, c.cd))
    many = c.cd[:1].repeat(1100, 1).contiguous()                         # across the LDS tiles of the centres, too
    assert int(KM.assign(c.Xd, many).max()) == 0


def test_assign_accepts_more_centres_than_rows_and_nan_rows():
    X, centres = R.make_input(5, 40, 3, "uniform")
    ids = KM.assign(X.to(DEV), centres.to(DEV)).cpu()
    assert torch.equal(ids, R.assign(X, centres)[0])
    X[2] = float("nan")
    ids = KM.assign(X.to(DEV), centres.to(DEV)).cpu()
    assert int(ids[2]) == 0 and torch.equal(ids[[0, 1, 3, 4]], R.assign(X, centres)[0][[0, 1, 3, 4]])


# ---- cluster_mean ----
@pytest.mark.parametrize("n,k,d,kind", R.SHAPES, ids=IDS)
def test_cluster_mean_against_float64(n, k, d, kind):
    c = case(n, k, d, kind)
    g = torch.Generator().manual_seed(n + k)
    ids = torch.randint(0, k, (n,), generator=g)
    for what in ("all clusters", "empty clusters and ids outside [0, K)"):
        if what != "all clusters":
            ids = torch.randint(-3, k + 3, (n,), generator=g)
            ids[ids == k // 2] = k + 7                                    # cluster k // 2 stays empty
            if n > 2:
                ids[0], ids[1] = -(2 ** 40), 2 ** 40                      # beyond 32 bits
        mean, counts = KM.cluster_mean(c.Xd, ids.to(DEV), k)
        want, want_counts = R.cluster_mean(c.X, ids, k)
        assert counts.dtype == torch.int64 and torch.equal(counts.cpu(), want_counts), what
        ok, err = close(mean, want, 1e-6)
        print(f"{what}: largest error of a mean {err:.3e}")
        assert ok, (what, err)
        assert not mean[counts == 0].any(), what
        if what != "all clusters":
            assert int(counts[k // 2]) == 0
        again = KM.cluster_mean(c.Xd, ids.to(DEV).int(), k) if what == "all clusters" else KM.cluster_mean(c.Xd, ids.to(DEV), k)
        assert torch.equal(again[0], mean) and torch.equal(again[1], counts), what            # the same bits again (and from int32 ids)


def test_cluster_mean_with_one_cluster():
    c = case(5000, 150, 35, "model")
    mean, counts = KM.cluster_mean(c.Xd, torch.zeros(5000, dtype=torch.int64, device=DEV), 1)
    assert counts.tolist() == [5000]
    ok, err = close(mean, c.X.double().mean(0, keepdim=True), 1e-6)
    assert ok, err


# ---- run ----
@pytest.mark.parametrize("n,k,d,kind", [R.SHAPES[4], R.SHAPES[7]], ids=[IDS[4], IDS[7]])
def test_one_iteration_teacher_forced(n, k, d, kind):
    c = case(n, k, d, kind)
    aux = c.X[:, :3].contiguous()
    res = KM.kmeans(c.Xd, k, iters=1, tol=0.0, init=c.cd, aux=aux.to(DEV))
    first = KM.assign(c.Xd, c.cd)                                         # the device's own first assignment
    want, _, s2 = R.update(c.X, first.cpu(), c.centres)
    ok, err = close(res.centres, want, 1e-6)
    print(f"centres: largest error {err:.3e}")
    assert ok, err
    assert torch.equal(res.ids, KM.assign(c.Xd, res.centres))             # the assignment to the centres RETURNED
    assert torch.equal(res.counts, torch.bincount(res.ids, minlength=k))
    ok, err = close(res.aux_mean, R.cluster_mean(aux, res.ids, k)[0], 1e-6)
    assert ok, err
    assert res.iterations == 1 and not res.converged
    assert abs(res.shift2 - s2) <= 1e-5 * max(s2, 1e-30)
    assert torch.equal(c.cd.cpu(), c.centres)                             # init is not written


def test_blobs_converge_and_later_launches_change_nothing():
    X, labels, init = R.blobs()
    Xd, aux = X.to(DEV), X[:, :3].contiguous().to(DEV)
    res = KM.kmeans(Xd, 20, iters=3, tol=1e-8, init=init.to(DEV), aux=aux)
    assert res.converged and res.iterations <= 3 and res.shift2 <= 1e-8
    assert torch.equal(res.ids.cpu(), labels)
    want, counts = R.cluster_mean(X, labels, 20)
    ok, err = close(res.centres, want, 1e-6)
    assert ok, err
    assert torch.equal(res.counts.cpu(), counts)
    long = KM.kmeans(Xd, 20, iters=50, tol=1e-8, init=init.to(DEV), aux=aux)
    assert long.iterations == res.iterations and long.converged
    for a, b in ((long.ids, res.ids), (long.centres, res.centres), (long.counts, res.counts), (long.aux_mean, res.aux_mean)):
        assert torch.equal(a, b)
    ref_ids, ref_centres, _, ran, conv = R.kmeans(X, init, 3, tol=1e-8)
    assert conv and ran == res.iterations and torch.equal(ref_ids, labels)


def test_an_empty_cluster_keeps_its_centre():
    X, labels, init = R.blobs()
    init = torch.cat([init, torch.full((1, 35), 50.0)])                   # far from every row
    res = KM.kmeans(X.to(DEV), 21, iters=5, init=init.to(DEV), aux=X[:, :3].contiguous().to(DEV))
    assert int(res.counts[20]) == 0 and torch.equal(res.centres[20].cpu(), init[20])
    assert not res.aux_mean[20].any() and torch.equal(res.ids.cpu(), labels)


def test_two_runs_give_the_same_bits():
    c = case(5000, 150, 35, "model")
    aux = c.Xd[:, :3].contiguous()
    a = KM.kmeans(c.Xd, 150, iters=10, seed=3, aux=aux)
    b = KM.kmeans(c.Xd, 150, iters=10, seed=3, aux=aux)
    for x, y in ((a.ids, b.ids), (a.centres, b.centres), (a.counts, b.counts), (a.aux_mean, b.aux_mean)):
        assert torch.equal(x, y)
    rows = torch.randperm(5000, generator=torch.Generator().manual_seed(3))[:150]        # the rows training.kmeans starts from
    assert torch.equal(KM.kmeans(c.Xd, 150, iters=10, init=c.Xd[rows.to(DEV)].contiguous(), aux=aux).centres, a.centres)
    assert int(a.counts.sum()) == 5000


def test_inertia_does_not_rise():
    c = case(5000, 150, 35, "model")
    prev = None
    for iters in range(1, 7):
        res = KM.kmeans(c.Xd, 150, iters=iters, init=c.cd)
        now = R.inertia(c.X, res.ids, res.centres)
        print(f"{iters} iterations: inertia {now:.9e}")
        assert prev is None or now <= prev * (1 + 1e-6), (iters, prev, now)
        prev = now


# ---- the model and the shims ----
def _model():
    X, labels, _ = R.blobs(n=3000, k=20, d=35, sigma=0.01, seed=5)
    raw = make_gaussians(SceneSpec(n_gaussians=3000, extent=(1.3, 1.3, 1.3), scale_lo=0.01, scale_hi=0.08, seed=11), device=DEV)
    args = SimpleNamespace(beta=0.1, d=4, w=256, feature_dim=32, second_stage_iteration=30000, third_stage_iteration=40000, jointly_iteration=1000,
                           nearest_num=6, norm_rotation=True, step_opacity=False, step_opacity_iteration=5000, opacity_type="implicit",
                           xyz_noise_iteration=0, max_points=20, adaptive_points_num=0)
    pc = gpa.GaussianModel(3, args)
    pc.set_inputDim(12, 60)
    pc.create_from_tensors((0.5 * X[:, :3]).to(DEV), raw["features_dc"], raw["features_rest"], raw["scaling"], raw["rotation"], raw["opacity"],
                           (1e-3 * X[:, 3:]).to(DEV), with_weights_model=True)
    pc.training_setup(default_training_args())
    return pc


def test_model_opt_in_and_the_path_as_it_stands():
    pc = _model()
    xyz = pc.get_xyz.detach().contiguous()
    feature = torch.cat([xyz, pc.motion_feature.detach()], dim=-1).contiguous()
    res = KM.kmeans(feature, 20, iters=20, tol=0.0, seed=0, aux=xyz)
    pc.set_superKeypoints(device_kmeans=True)
    assert pc.super_gaussians.shape == (20, 3) and pc.super_gaussians_feature.shape == (20, 32)
    assert pc.super_gaussians.requires_grad and pc.super_gaussians_feature.requires_grad
    assert torch.equal(pc.super_gaussians_feature.detach(), res.centres[:, 3:])
    assert torch.equal(pc.super_gaussians.detach(), torch.where(res.counts[:, None] > 0, res.aux_mean, res.centres[:, :3]))
    want, counts = R.cluster_mean(xyz, res.ids, 20)
    keep = counts > 0
    ok, err = close(pc.super_gaussians[keep.to(DEV)], want[keep], 1e-6)
    assert ok, err
    pc.training2stage_setup()                                            # the optimizer is rebuilt as today
    assert pc.second_stage and [g["name"] for g in pc.optimizer.param_groups] == ["s_xyz", "s_motion_feature", "weight_mlp", "df_mlp"]
    assert pc.optimizer.param_groups[0]["params"][0] is pc.super_gaussians
    # args.kmeans_device / kmeans_iters / kmeans_tol select it, too
    pc2 = _model()
    pc2.args.kmeans_device, pc2.args.kmeans_iters, pc2.args.kmeans_tol = True, 2, 0.0
    pc2.set_superKeypoints()
    two = KM.kmeans(feature, 20, iters=2, aux=xyz)
    assert torch.equal(pc2.super_gaussians_feature.detach(), two.centres[:, 3:])
    # off (the default): the composition as it stands -- training.kmeans and index_add_ (float atomics: compared to a tolerance)
    for kw in ({}, {"device_kmeans": False}):
        pc3 = _model()
        pc3.set_superKeypoints(**kw)
        ids, centres = training_kmeans(feature, 20, seed=0)
        pos, cnt = R.cluster_mean(xyz, ids, 20)
        pos = torch.where(cnt[:, None] > 0, pos, centres[:, :3].double().cpu())
        assert close(pc3.super_gaussians_feature, centres[:, 3:], 1e-5)[0] and close(pc3.super_gaussians, pos, 1e-5)[0]


def test_shims_reproduce_the_reference_feature_kmeans_body():
    from kmeans_pytorch import kmeans
    from torch_scatter import scatter
    c = case(5000, 150, 35, "model")
    xyzs, features = c.Xd[:, :3].contiguous(), c.Xd
    cluster_ids_x, cluster_centers = kmeans(X=features, num_clusters=150, device=features.device)
    xyzs_means = scatter(xyzs, cluster_ids_x.to(xyzs.device), dim=0, reduce="mean")
    res = KM.kmeans(c.Xd, 150, iters=1000, tol=1e-4, seed=0, aux=xyzs)
    assert torch.equal(cluster_ids_x, res.ids) and torch.equal(cluster_centers, res.centres)
    rows = xyzs_means.shape[0]                                           # index.max() + 1: clusters without rows may end the list
    assert rows == int(res.ids.max()) + 1 and torch.equal(xyzs_means, res.aux_mean[:rows]) and not res.counts[rows:].any()
    assert res.converged and res.iterations < 1000
    sums = scatter(xyzs, cluster_ids_x, dim=0, reduce="sum", dim_size=152)
    assert sums.shape == (152, 3) and not sums[150:].any()
    assert close(sums[:150], R.cluster_mean(xyzs, res.ids, 150)[0] * res.counts[:, None].cpu(), 1e-6)[0]
