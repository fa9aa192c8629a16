"""Densify / reset / prune on the device (include/gp_densify.h; GaussianModel.densify_prune_device, densify.track_view_device,
densify.densification_step_device) against the restatement of the existing sequence (tests/densify_ref.py, pinned to the existing
methods by tests/test_densify_plan_host.py) and against the existing methods themselves.

Row counts straddle the plan's block size B.  Selections are set by writing statistics, scalings and opacities so that every compared
quantity sits at <= 0.5 x or >= 2 x its threshold (asserted in float64): no selection can flip on an ulp.  Copied fields, moments and
statistics must be bit-identical.  The computed fields (split xyz, split scaling, reset opacity) come from the device's own exp / log:
per field, the kernel's largest distance from the float64 shadow may be at most 4 x the float32 restatement's own distance from it on
the same inputs (a different but correct exp / log and FMA contraction); both distances are printed (pytest -s)."""
import math
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

import densify_ref as R  # noqa: E402
import gaussianprediction_amd as gpa  # noqa: E402
from gaussianprediction_amd import densify as dn, densify_ops as D  # noqa: E402
from gaussianprediction_amd.cameras import orbit_cameras  # noqa: E402
from gaussianprediction_amd.renderer import render  # noqa: E402
from gaussianprediction_amd.scene_synth import SceneSpec, make_gaussians, make_keypoints  # noqa: E402
from gaussianprediction_amd.train_step import TrainStep  # noqa: E402
from gaussianprediction_amd.training import default_training_args  # noqa: E402

DEV = "cuda"
B = D.BLOCK
BIG = 3 * B + 37
SIZES = [1, B - 1, B, B + 1, BIG]
ITERATION = 5000
EXTENT, PERCENT_DENSE, GRAD_T, SCREEN = 5.0, 0.01, 0.0002, 20
MARGS = SimpleNamespace(beta=0.1, d=4, w=256, feature_dim=32, second_stage_iteration=30000, third_stage_iteration=40000,
                        jointly_iteration=1000, nearest_num=6, norm_rotation=True, step_opacity=False, step_opacity_iteration=5000,
                        opacity_type="implicit", xyz_noise_iteration=0)


def _knn_and_weights(pc):
    _, _, idx, rw = make_keypoints(pc._xyz.detach(), pc.motion_feature.detach(), 48, 6)
    pc.set_keypoint_weights(rw, idx)


def _new_model(raw, kp=None, kpf=None):
    # (a model without keypoints sizes its keypoint statistics by args.max_points)
    pc = gpa.GaussianModel(3, MARGS if kp is not None else SimpleNamespace(max_points=8, adaptive_points_num=6, **vars(MARGS)))
    pc.set_inputDim(12, 60)
    pc.create_from_tensors(raw["xyz"], raw["features_dc"], raw["features_rest"], raw["scaling"], raw["rotation"], raw["opacity"],
                           raw["motion_feature"], kp, kpf)
    return pc


@pytest.fixture(scope="module")
def trained():
    """N = 3B+37, stage 1, three TrainStep steps with tracked statistics: non-zero moments of every group.  Read-only: tests copy it."""
    raw = make_gaussians(SceneSpec(n_gaussians=BIG, extent=(1.3, 1.3, 1.3), scale_lo=0.01, scale_hi=0.08, seed=11), device=DEV)
    kp, kpf, _, _ = make_keypoints(raw["xyz"], raw["motion_feature"], 48, 6)
    pc = _new_model(raw, kp, kpf)
    cams = orbit_cameras(4, 4.0, 0.69, 160, 128, device=DEV)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    _knn_and_weights(pc)
    with torch.no_grad():
        gts = [render(c, pc, pipe, torch.zeros(3, device=DEV), time=torch.tensor([0.3], device=DEV), it=ITERATION)["render"] * 0.9
               for c in cams]
    ts = TrainStep(pc, cams, gts, ITERATION, schedule=True)
    for i in range(3):
        _, pkg = ts.step(i)
        dn.track_view(pc, pkg["viewspace_points"], pkg["visibility_filter"], pkg["radii"])
    torch.cuda.synchronize()
    assert pc.motion_feature.shape == (BIG, 32) and "motion_feature" in {g["name"] for g in pc.optimizer.param_groups}
    assert all(float(m.abs().sum()) > 0 for m, _ in pc.adam_moments().values())
    return SimpleNamespace(pc=pc, cams=cams, gts=gts)


def _copy(pc):
    """A second model in the state of `pc`: parameters, MLP, keypoints, every Adam moment, step counts, rates, statistics."""
    per = {k: v.detach() for k, v in pc._per_gaussian().items()}
    has_kp = isinstance(getattr(pc, "super_gaussians", None), torch.nn.Parameter)
    q = gpa.GaussianModel(3, MARGS)
    q.set_inputDim(12, 60)
    q.create_from_tensors(per["xyz"], per["f_dc"], per["f_rest"], per["scaling"], per["rotation"], per["opacity"], per["motion_feature"],
                          pc.super_gaussians.detach() if has_kp else None, pc.super_gaussians_feature.detach() if has_kp else None)
    q.df_model.load_state_dict(pc.df_model.state_dict())
    if getattr(pc, "knn_idx", None) is not None:
        q.set_keypoint_weights(pc.raw_weights, pc.knn_idx)
    q.training_setup(pc.training_args)
    mom = pc.adam_moments()
    assert len(pc.bucket.params) == len(q.bucket.params)
    for a, b in zip(pc.bucket.params, q.bucket.params):
        assert a.shape == b.shape
        q.optimizer.load_full_moments(b, mom[id(a)][0].clone(), mom[id(a)][1].clone())
    q.optimizer.step_count, q.optimizer.lag = pc.optimizer.step_count, dict(pc.optimizer.lag)
    for ga, gb in zip(pc.optimizer.param_groups, q.optimizer.param_groups):
        assert ga["name"] == gb["name"]
        gb["lr"] = ga["lr"]
    q.xyz_gradient_accum, q.denom = pc.xyz_gradient_accum.clone(), pc.denom.clone()
    q.xyz_gradient_accum_max, q.max_radii2D = pc.xyz_gradient_accum_max.clone(), pc.max_radii2D.clone()
    return q


def _model(n, trained):
    """N = 3B+37: a copy of the trained model; elsewhere a fresh stage-1 model whose moments are filled with random values."""
    if n == BIG:
        return _copy(trained.pc)
    raw = make_gaussians(SceneSpec(n_gaussians=n, extent=(1.3, 1.3, 1.3), scale_lo=0.01, scale_hi=0.08, seed=100 + n), device=DEV)
    pc = _new_model(raw)
    pc.training_setup(default_training_args())
    g = torch.Generator(device=DEV).manual_seed(n)
    for p in pc.bucket.params:
        pc.optimizer.load_full_moments(p, torch.randn(p.shape, generator=g, device=DEV), torch.rand(p.shape, generator=g, device=DEV))
    pc.optimizer.step_count = 3
    assert pc.motion_feature.shape == (n, 32)
    return pc


# ---- selection patterns: the kind of every row, written into statistics, scalings and opacities -----------------------------------
KEEP, CLONE, SPLIT, PRUNE, WORLD, SPLIT_GONE, CLONE_GONE, SCREEN_BIG = range(8)
HOT = {CLONE, SPLIT, SPLIT_GONE, CLONE_GONE}               # mean gradient 5 x the threshold, else 0.25 x
SCALE = {KEEP: 0.02, CLONE: 0.02, PRUNE: 0.02, CLONE_GONE: 0.02, SCREEN_BIG: 0.02,      # x [0.6, 0.95]: <= 0.4 x percent_dense * extent
         SPLIT: 0.25,                                      # 3 .. 4.75 x percent_dense * extent, <= 0.475 x 0.1 * extent
         WORLD: 4.0, SPLIT_GONE: 4.0}                      # >= 4.8 x 0.1 * extent, shrunk by 1.6 still >= 3 x
PATTERNS = ["nothing", "all cloned", "all split", "alternating", "split run across a block boundary", "all but one pruned",
            "prune alone, live radii"]


def _kinds(pattern, n):
    i = torch.arange(n)
    if pattern == "nothing":
        return torch.full((n,), KEEP)
    if pattern == "all cloned":
        return torch.full((n,), CLONE)
    if pattern == "all split":
        return torch.full((n,), SPLIT)
    if pattern == "alternating":
        return torch.tensor([CLONE, SPLIT, PRUNE, KEEP, WORLD, SPLIT_GONE, CLONE_GONE])[i % 7]
    if pattern == "split run across a block boundary":
        return torch.where((i >= B - 5) & (i < B + 7), SPLIT, KEEP)
    if pattern == "all but one pruned":
        return torch.where(i == n // 2, KEEP, PRUNE)
    return torch.tensor([KEEP, PRUNE, SCREEN_BIG, WORLD])[i % 4]


def _write_pattern(pc, pattern):
    n = pc._xyz.shape[0]
    kinds = _kinds(pattern, n)
    g = torch.Generator().manual_seed(n)
    views = torch.randint(1, 4, (n,), generator=g).float()
    views[kinds == KEEP] *= (torch.arange(n)[kinds == KEEP] % 3 != 0)            # some kept rows were never seen: denom 0
    hot = torch.tensor([int(k) in HOT for k in kinds])
    grad = torch.where(hot, 5.0 * GRAD_T, 0.25 * GRAD_T)
    scale = torch.tensor([SCALE[int(k)] for k in kinds])[:, None] * (0.6 + 0.35 * torch.rand(n, 3, generator=g))
    gone = (kinds == PRUNE) | (kinds == CLONE_GONE)
    opacity = torch.where(gone, -10.0, -2.0 + 4.0 * torch.rand(n, generator=g))   # sigmoid 4.5e-5, or 0.12 .. 0.88
    with torch.no_grad():
        pc._scaling.copy_(scale.log().to(DEV))
        pc._opacity.copy_(opacity[:, None].to(DEV))
    pc.denom = views[:, None].to(DEV)
    pc.xyz_gradient_accum = (grad * views)[:, None].to(DEV)
    pc.xyz_gradient_accum_max = torch.rand(n, 1, generator=g).to(DEV)
    pc.max_radii2D = torch.where(kinds == SCREEN_BIG, 50.0, 5.0 * torch.rand(n, generator=g)).to(DEV)
    return kinds


def _snapshot(pc):
    per, mom = pc._per_gaussian(), pc.adam_moments()
    state = {k: v.detach().clone() for k, v in per.items()}
    moments = {k: tuple(t.clone() for t in mom[id(p)]) for k, p in per.items() if id(p) in mom}
    stats = dict(accum=pc.xyz_gradient_accum.clone(), denom=pc.denom.clone(), accum_max=pc.xyz_gradient_accum_max.clone(),
                 max_radii2D=pc.max_radii2D.clone())
    return state, moments, stats


def _normals(n, seed):
    return torch.randn(2, n, 3, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV)


def _computed_rows(want, do_reset):
    """field -> mask over the output rows of the values the kernel computes rather than copies."""
    new = want.segment >= 2
    return {"xyz": new, "scaling": new, "opacity": torch.full_like(new, bool(do_reset))}


def _check_against(got_state, got_mom, got_stats, want, shadow, do_reset, tag):
    """Copied values bit-identical; computed fields within 4 x the float32 restatement's own distance from the float64 shadow."""
    assert set(got_state) == set(want.state) and set(got_mom) == set(want.moments)
    assert torch.equal(want.source, shadow.source) and torch.equal(want.segment, shadow.segment)
    computed = _computed_rows(want, do_reset)
    for k, t in got_state.items():
        assert t.shape == want.state[k].shape, (tag, k, t.shape, want.state[k].shape)
        rows = computed.get(k)
        if rows is None:
            assert torch.equal(t, want.state[k]), (tag, k)
            continue
        assert torch.equal(t[~rows], want.state[k][~rows]), (tag, k)
        if bool(rows.any()):
            d_kernel = float((t[rows].double() - shadow.state[k][rows]).abs().max())
            d_torch = float((want.state[k][rows].double() - shadow.state[k][rows]).abs().max())
            print(f"[densify {tag}] {k}: kernel - float64 {d_kernel:.3e}   float32 torch - float64 {d_torch:.3e}   rows {int(rows.sum())}")
            assert d_kernel <= 4 * d_torch, (tag, k, d_kernel, d_torch)
    for k, (m, v) in got_mom.items():          # every moment, the zeroed ones of new rows and of the reset opacities included
        assert torch.equal(m, want.moments[k][0]) and torch.equal(v, want.moments[k][1]), (tag, k)
    for k in R.STATS:
        assert got_stats[k].shape == want.stats[k].shape and torch.equal(got_stats[k], want.stats[k]), (tag, k)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_device_surgery_equals_the_restatement(n, pattern, trained):
    do_densify = pattern != "prune alone, live radii"
    for do_reset in (False, True):
        tag = f"N={n} {pattern} reset={int(do_reset)}"
        pc = _model(n, trained)
        kinds = _write_pattern(pc, pattern)
        th = dict(grad_threshold=GRAD_T, percent_dense=PERCENT_DENSE, extent=EXTENT, max_screen_size=SCREEN, do_densify=do_densify,
                  do_reset=do_reset, min_opacity=0.004 if do_reset else 0.005)     # (reset opacities are 0.01: 2.5 x / 2 x away)
        state, moments, stats = _snapshot(pc)
        ratio = R.margins(state, stats, **th)
        assert bool(((ratio <= 0.5) | (ratio >= 2.0)).all()), (tag, ratio[((ratio > 0.5) & (ratio < 2.0)).any(dim=1)])
        normals = _normals(n, 77)
        want = R.densify_reset_prune(state, moments, stats, normals, **th)
        shadow = R.densify_reset_prune(state, moments, stats, normals, dtype=torch.float64, **th)
        epoch, step, lag = pc.optimizer_epoch, pc.optimizer.step_count, dict(pc.optimizer.lag)
        lrs = {g["name"]: g["lr"] for g in pc.optimizer.param_groups}
        out = pc.densify_prune_device(GRAD_T, th["min_opacity"], EXTENT, SCREEN, do_densify, do_reset,
                                      generator=torch.Generator(device=DEV).manual_seed(77))
        # counts and what the pattern says they must be
        assert out == (want.n_clone, want.n_src, want.n_pruned), (tag, out)
        if do_densify:
            assert out[0] == int(((kinds == CLONE) | (kinds == CLONE_GONE)).sum()) and out[1] == int(((kinds == SPLIT) | (kinds == SPLIT_GONE)).sum())
            assert out[2] == int(((kinds == PRUNE) | (kinds == WORLD)).sum()) + 2 * int((kinds == CLONE_GONE).sum() + (kinds == SPLIT_GONE).sum())
        else:
            assert out == (0, 0, int((kinds != KEEP).sum()))
        assert pc._xyz.shape[0] == want.source.numel() == n + out[0] + out[1] - out[2]
        got_state, got_mom, got_stats = _snapshot(pc)
        _check_against(got_state, got_mom, got_stats, want, shadow, do_reset, tag)
        if pattern == "nothing" and not do_reset:          # the output is the input, bit for bit
            assert all(torch.equal(got_state[k], state[k]) for k in state)
            assert all(torch.equal(got_mom[k][0], moments[k][0]) and torch.equal(got_mom[k][1], moments[k][1]) for k in moments)
        # ONE optimizer rebuild; step count, lag and rates as they were; fresh Parameters wired to the new bucket
        assert pc.optimizer_epoch == epoch + 1 and pc.optimizer.step_count == step and pc.optimizer.lag == lag
        assert {g["name"]: g["lr"] for g in pc.optimizer.param_groups} == lrs and pc.optimizer.pending_hold == set()
        assert pc._xyz.grad is not None and pc._xyz.grad.shape == pc._xyz.shape and all(p.requires_grad for p in pc._per_gaussian().values())


def test_two_calls_give_the_same_bits(trained):
    outs = []
    for _ in range(2):
        pc = _copy(trained.pc)
        _write_pattern(pc, "alternating")
        pc.densify_prune_device(GRAD_T, 0.005, EXTENT, SCREEN, True, True, generator=torch.Generator(device=DEV).manual_seed(5))
        outs.append(_snapshot(pc))
    (s0, m0, t0), (s1, m1, t1) = outs
    assert all(torch.equal(s0[k], s1[k]) for k in s0) and all(torch.equal(t0[k], t1[k]) for k in t0)
    assert all(torch.equal(m0[k][j], m1[k][j]) for k in m0 for j in (0, 1))


def test_sharded_optimizer_is_refused_and_the_model_untouched(trained):
    pc = _copy(trained.pc)
    _write_pattern(pc, "alternating")
    before, params, opt, no = _snapshot(pc), dict(pc._per_gaussian()), pc.optimizer, pc._surgery_no
    pc.optimizer_shard = (0, 2)
    with pytest.raises(NotImplementedError, match=r"densify\(\)"):
        pc.densify_prune_device(GRAD_T, 0.005, EXTENT, SCREEN, True, False)
    with pytest.raises(NotImplementedError):
        dn.densification_step_device(pc, 3100, default_training_args(), EXTENT)
    after = _snapshot(pc)
    assert all(pc._per_gaussian()[k] is p for k, p in params.items()) and pc.optimizer is opt and pc._surgery_no == no
    assert all(torch.equal(before[0][k], after[0][k]) for k in before[0]) and all(torch.equal(before[2][k], after[2][k]) for k in R.STATS)


# ---- the loop-side entry against the existing one, on two copies of the trained model --------------------------------------------
def _threshold(pc):
    """A gradient threshold that selects about half of the rows the three tracked views saw."""
    g = (pc.xyz_gradient_accum / pc.denom.clamp_min(1)).squeeze(-1)
    return float(g[g > 0].median()) * 1.001


def _run_both(trained, iteration, monkeypatch, before=None):
    old, new = _copy(trained.pc), _copy(trained.pc)
    opt = default_training_args(densify_grad_threshold=_threshold(old))
    for pc in (old, new):
        if before is not None:
            before(pc)
    state, moments, stats = _snapshot(old)
    screen = 20 if iteration > opt.opacity_reset_interval else None
    do_reset = iteration % opt.opacity_reset_interval == 0
    th = dict(grad_threshold=opt.densify_grad_threshold, percent_dense=old.percent_dense, extent=EXTENT, min_opacity=0.005,
              max_screen_size=screen, do_densify=True, do_reset=do_reset)
    normals = _normals(BIG, 9)
    want = R.densify_reset_prune(state, moments, stats, normals, **th)
    shadow = R.densify_reset_prune(state, moments, stats, normals, dtype=torch.float64, **th)
    with monkeypatch.context() as mp:        # the old path draws torch.normal(std=stds[sel]): the same draws, copy c of source i from normals[c, i]
        mp.setattr(torch, "normal", lambda mean, std, generator=None: normals[:, want.split].reshape(-1, 3) * std)
        out_old = dn.densification_step(old, iteration, opt, EXTENT)
    out_new = dn.densification_step_device(new, iteration, opt, EXTENT, generator=torch.Generator(device=DEV).manual_seed(9))
    return old, new, out_old, out_new, want, shadow, do_reset


@pytest.mark.parametrize("iteration", [3100, 6000])
def test_densification_step_device_equals_densification_step(iteration, trained, monkeypatch):
    old, new, out_old, out_new, want, shadow, do_reset = _run_both(trained, iteration, monkeypatch)
    assert out_old == out_new == (want.n_clone, want.n_src, want.n_pruned) and min(out_new[:2]) > 0
    s_old, m_old, t_old = _snapshot(old)
    assert all(torch.equal(s_old[k], want.state[k]) for k in s_old)           # the restatement IS the old path, on the device too
    s_new, m_new, t_new = _snapshot(new)
    _check_against(s_new, m_new, t_new, want, shadow, do_reset, f"step {iteration}")
    assert all(torch.equal(m_old[k][j], m_new[k][j]) for k in m_old for j in (0, 1)) and all(torch.equal(t_old[k], t_new[k]) for k in t_old)
    # every OTHER optimized tensor (MLP) kept its moments; counters and holds agree
    for a, b in zip(old.bucket.params, new.bucket.params):
        ma, mb = old.adam_moments()[id(a)], new.adam_moments()[id(b)]
        assert torch.equal(ma[0], mb[0]) and torch.equal(ma[1], mb[1])
    assert old.optimizer.step_count == new.optimizer.step_count == trained.pc.optimizer.step_count
    assert old.optimizer.lag == new.optimizer.lag and old.optimizer.pending_hold == new.optimizer.pending_hold == set()
    # training goes on.  The bar is the one tests/test_gpu_densify.py sets for a run across a surgery: finite losses, finite parameters,
    # outputs of the new row count (it sets none between two runs; the difference of the two paths' losses is printed)
    losses = []
    for pc in (old, new):
        _knn_and_weights(pc)
        ts = TrainStep(pc, trained.cams, trained.gts, ITERATION, schedule=True)
        run = []
        for i in range(3):
            loss, pkg = ts.step(i)
            run.append(float(loss))
            assert pkg["radii"].shape[0] == pc._xyz.shape[0]
        assert all(math.isfinite(v) for v in run) and torch.isfinite(pc._xyz).all() and torch.isfinite(pc._features_rest).all()
        losses.append(run)
    print(f"[densify step {iteration}] losses old {losses[0]} device {losses[1]}")


def test_reference_order_holds_the_same_groups(trained, monkeypatch):
    """backward -> surgery -> optimizer.step() [REF train.py:164-197]: the replaced per-Gaussian groups sit this step out, the MLP is
    updated from the carried gradient -- on both paths alike."""
    def backward(pc):
        g = torch.Generator(device=DEV).manual_seed(1)
        sum((p * torch.randn(p.shape, generator=g, device=DEV)).sum() for p in pc.bucket.params).backward()
        assert pc._unconsumed_gradient()

    old, new, out_old, out_new, want, shadow, _ = _run_both(trained, 3100, monkeypatch, before=backward)
    assert out_old == out_new
    per = set(new._per_gaussian())
    assert old.optimizer.pending_hold == new.optimizer.pending_hold == per
    before = {k: v.detach().clone() for k, v in new._per_gaussian().items()}
    mlp_before = [p.detach().clone() for p in new.df_model.parameters()]
    for a, b in zip(old.df_model.parameters(), new.df_model.parameters()):
        assert torch.equal(old.bucket.segment(a), new.bucket.segment(b)) and float(new.bucket.segment(b).abs().sum()) > 0
    for pc in (old, new):
        pc.optimizer.step()
    assert all(torch.equal(before[k], new._per_gaussian()[k].detach()) for k in before)          # held
    assert all(torch.equal(a, b) for a, b in zip(old.df_model.parameters(), new.df_model.parameters()))
    assert any(not torch.equal(a, b) for a, b in zip(mlp_before, new.df_model.parameters()))      # updated
    assert old.optimizer.lag == new.optimizer.lag and all(new.optimizer.lag.get(k) == 1 for k in per)
    assert old.optimizer.pending_hold == new.optimizer.pending_hold == set()


# ---- per-view statistics -------------------------------------------------------------------------------------------------------
def _ulp(x):
    """Spacing of float32 at the magnitude of x (float64 tensor)."""
    return torch.where(x > 0, torch.exp2(torch.floor(torch.log2(x.clamp_min(1e-300))) - 23), torch.full_like(x, 2.0 ** -149))


def _with_stats(pc, start):
    pc.xyz_gradient_accum, pc.denom = start["accum"].clone(), start["denom"].clone()
    pc.xyz_gradient_accum_max, pc.max_radii2D = start["accum_max"].clone(), start["radii"].clone()
    return pc


def _stats_of(pc):
    return dict(accum=pc.xyz_gradient_accum, denom=pc.denom, accum_max=pc.xyz_gradient_accum_max, radii=pc.max_radii2D)


def test_track_view_device_equals_track_view(trained):
    n, NAN_ROW = BIG, 7
    g = torch.Generator(device=DEV).manual_seed(3)
    start = dict(accum=torch.rand(n, 1, generator=g, device=DEV), denom=torch.randint(0, 3, (n, 1), generator=g, device=DEV).float(),
                 accum_max=torch.rand(n, 1, generator=g, device=DEV) * 0.5, radii=torch.randint(0, 30, (n,), generator=g, device=DEV).float())
    old, new, two = (_with_stats(_copy(trained.pc), start) for _ in range(3))
    views = []      # a view that sees nothing, one that sees about half, one that sees everything
    for v, vis in enumerate([torch.zeros(n, dtype=torch.bool, device=DEV), torch.rand(n, generator=g, device=DEV) < 0.5,
                             torch.ones(n, dtype=torch.bool, device=DEV)]):
        vs = torch.zeros(n, 3, device=DEV, requires_grad=True)
        vs.grad = torch.randn(n, 3, generator=g, device=DEV) * 10.0 ** torch.randint(-6, 1, (n, 1), generator=g, device=DEV).float()
        if v == 2:
            vs.grad[NAN_ROW, 0] = float("nan")
        views.append({"viewspace_points": vs, "visibility_filter": vis,
                      "radii": torch.randint(0, 60, (n,), generator=g, device=DEV, dtype=torch.int32)})
    seen = views[1]["visibility_filter"]
    torch.cuda.synchronize()
    # no host wait: where the sync debug mode makes a plain .item() raise (the positive control), track_view_device must not raise
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=DEV).item()
            control = False
        except RuntimeError:
            control = True
        if control:
            for pkg in views:
                dn.track_view_device(new, pkg)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not control:
        print("[densify] set_sync_debug_mode('error') does not catch .item() on this build: the no-host-wait assertion is skipped")
        for pkg in views:
            dn.track_view_device(new, pkg)
    for pkg in views:
        dn.track_view(old, pkg["viewspace_points"], pkg["visibility_filter"], pkg["radii"])
    for pkg in views[:2]:
        dn.track_view_device(two, pkg)
    got, ref, part = _stats_of(new), _stats_of(old), _stats_of(two)
    assert torch.equal(got["radii"], ref["radii"]) and torch.equal(got["denom"], ref["denom"])
    assert torch.equal((got["denom"] - start["denom"]).squeeze(-1), 1 + seen.float())
    # rows that no view saw keep their bits in all four tensors (after the first two views: those outside the second one's filter)
    for k in start:
        assert torch.equal(part[k][~seen], start[k][~seen]) and not torch.equal(part[k][seen], start[k][seen]), k
    # float64 restatement of sum and maximum.  Each float32 increment sqrt(gx^2 + gy^2) is within 2 ulp of its float64 value and every
    # addition rounds once, so after v views the sum is within 2 v ulp at the largest running magnitude; the maximum within 2 ulp
    acc, top = start["accum"].double().squeeze(-1), start["accum_max"].double().squeeze(-1)
    biggest, count = acc.clone(), torch.zeros(n, dtype=torch.double, device=DEV)
    for pkg in views:
        vis = pkg["visibility_filter"]
        size = pkg["viewspace_points"].grad[:, :2].double().pow(2).sum(-1).sqrt()
        acc = torch.where(vis, acc + size, acc)
        top = torch.where(vis & (size > top), size, top)           # a NaN never replaces a number
        biggest = torch.maximum(biggest, torch.nan_to_num(acc, nan=0.0))
        count += vis
    rest = torch.ones(n, dtype=torch.bool, device=DEV)
    rest[NAN_ROW] = False
    for name, m in (("device", got), ("torch", ref)):
        a, t = m["accum"].squeeze(-1).double(), m["accum_max"].squeeze(-1).double()
        assert bool(torch.isnan(a[NAN_ROW])) and not bool(torch.isnan(a[rest]).any()) and not bool(torch.isnan(t).any()), name
        assert bool(((a - acc).abs()[rest] <= (2 * count * _ulp(biggest))[rest]).all()), name
        assert bool(((t - top).abs() <= 2 * _ulp(top)).all()), name
    # the NaN row's running maximum is what the first two views left, to the bit
    assert torch.equal(got["accum_max"][NAN_ROW], part["accum_max"][NAN_ROW])
