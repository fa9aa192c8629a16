"""-m gpu: the GCN keypoint motion predictor on the device (include/gp_gcn.h, gaussianprediction_amd/gcn_ops.py, motion.py) against the
float64 restatement of tests/gcn_ref.py, which tests/test_gcn_host.py holds to the values recorded from the reference's own classes.

The bar of every compared tensor is gcn_ref.bar: max(8 x the float32 restatement's own distance from the float64 one, for that same
tensor, 8 * 2^-23 * max|float64 tensor|); every measured distance is printed beside its bar.  One exclusion: the biases of the graph
convolutions that train-mode BatchNorm follows (true gradient exactly zero: rounding noise in any implementation) are only checked to be
finite, and their count is asserted."""
import functools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gcn_ref as R  # noqa: E402
from gaussianprediction_amd import gcn_ops as G, motion  # noqa: E402

DEV = "cuda"
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gcn.npz"))
KIND = {G.ACT_NONE: "none", G.ACT_TANH: "tanh", G.ACT_RELU: "relu"}


def _check(name, got, f32, f64):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    f64 = np.asarray(f64, dtype=np.float64)
    bar, dist = R.bar(f32, f64), float(np.abs(got.reshape(f64.shape) - f64).max())
    print(f"{name}: distance {dist:.3e}  bar {bar:.3e}")
    assert np.isfinite(got).all() and dist <= bar, (name, dist, bar)


@functools.lru_cache(maxsize=None)
def _ref_train(name):
    c = R.cfg_of(name)
    return R.train_pass(c, torch.float64), R.train_pass(c, torch.float32)


@functools.lru_cache(maxsize=None)
def _ref_rollout(name, nr):
    c = R.cfg_of(name)
    return R.rollout_pass(c, torch.float64, nr), R.rollout_pass(c, torch.float32, nr)


def _model(c, train=True):
    m = motion.GCN_xyzr(c.T, c.H, c.out, 0, num_stage=c.num_stage, node_n=c.K, no_mapping=c.no_mapping)
    m.load_state_dict(R.to_torch(R.seeded_state(c), torch.float32), strict=True)
    m = m.to(DEV)
    return m.train() if train else m.eval()


def _batch(c, grad=False):
    b = R.to_torch(R.seeded_batch(c), torch.float32, DEV)
    if grad:
        b["xyz_inputs"].requires_grad_(True), b["rotation_inputs"].requires_grad_(True)
    return b


# ---- one layer --------------------------------------------------------------------------------------------------------------------------
# (B, M, Fin, Fout, att, act, residual, w_transposed): below one tile; ragged rows with an odd Fin; Fout = 3; more than one 256-wide k-chunk
# and more than one 64-row block; nn.Linear's form
LAYERS = [(2, 15, 10, 16, True, G.ACT_TANH, False, False), (3, 148, 7, 48, True, G.ACT_TANH, True, False), (3, 111, 48, 3, True, G.ACT_NONE, False, False),
          (4, 360, 32, 32, True, G.ACT_TANH, True, False), (3, 111, 48, 48, False, G.ACT_RELU, False, True), (1, 270, 10, 32, True, G.ACT_TANH, False, False)]


def _layer_inputs(shape, seed):
    B, M, Fin, Fout, att, act, res, wt = shape
    rng = np.random.default_rng(seed)
    u = lambda *s: rng.uniform(-1, 1, size=s)
    d = {"x": u(B, M, Fin), "W": u(Fin, Fout) / np.sqrt(Fout), "bias": u(Fout) * 0.2}
    if att:
        d["att"] = u(M, M) / np.sqrt(Fout)
    if res:
        d["res"] = u(B, M, Fout)
    d.update(gamma=rng.uniform(0.5, 1.5, size=M * Fout), beta=rng.uniform(-0.3, 0.3, size=M * Fout), rm=rng.uniform(-0.5, 0.5, size=M * Fout),
             rv=rng.uniform(0.5, 2.0, size=M * Fout))
    return d


def _ref_layer(d, shape, dtype, mode):
    act = KIND[shape[5]]
    t = {k: torch.tensor(v, dtype=dtype) for k, v in d.items()}
    stats = {}
    bn = None if mode == "off" else (t["gamma"], t["beta"], t["rm"], t["rv"])
    y = R.layer(t["x"], t["W"], t.get("att"), t["bias"], bn, mode == "train", act, t.get("res"), stats, "bn")
    out = {"y": y}
    out.update(stats)
    return {k: v.double().numpy() for k, v in out.items()}


# (train-mode BatchNorm needs B >= 2; B = 1 is refused: tests/test_gcn_host.py)
LAYER_CASES = [(s, mode) for s in LAYERS for mode in ("off", "eval", "train") if not (mode == "train" and s[0] < 2)]


@pytest.mark.parametrize("shape,mode", LAYER_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(str(int(q)) for q in v))
def test_layer_forward(shape, mode):
    B, M, Fin, Fout, att, act, res, wt = shape
    d = _layer_inputs(shape, 5)
    f64, f32 = _ref_layer(d, shape, torch.float64, mode), _ref_layer(d, shape, torch.float32, mode)
    t = {k: torch.tensor(v, dtype=torch.float32, device=DEV) for k, v in d.items()}
    W = t["W"].t().contiguous() if wt else t["W"]
    bn = None if mode == "off" else (t["gamma"], t["beta"], t["rm"], t["rv"])
    with torch.no_grad():
        y = G.layer(t["x"], W, t.get("att"), t["bias"], bn=bn, training=mode == "train", act=act, residual=t.get("res"), w_transposed=wt)
    _check("y", y, f32["y"], f64["y"])
    if mode == "train":
        _check("running_mean", t["rm"], f32["bn.running_mean"], f64["bn.running_mean"])
        _check("running_var", t["rv"], f32["bn.running_var"], f64["bn.running_var"])
    else:
        assert np.array_equal(t["rm"].cpu().numpy(), d["rm"].astype(np.float32))         # eval mode leaves the statistics alone


# ---- the whole network --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_network_train_forward_and_every_gradient(name):
    c = R.cfg_of(name)
    f64, f32 = _ref_train(name)
    m, b = _model(c), _batch(c, grad=True)
    args = SimpleNamespace(norm_rotation=True)
    xp, xg, rp, rg = motion.operate(args, b, m)
    loss = motion.gcn_loss(xp, xg, rp, rg)
    loss.backward()
    _check("xyz_pred", xp, f32["xyz_pred"], f64["xyz_pred"])
    _check("r_pred", rp, f32["r_pred"], f64["r_pred"])
    _check("loss", loss, f32["loss"], f64["loss"])
    _check("grad_xyz_inputs", b["xyz_inputs"].grad, f32["grad_xyz_inputs"], f64["grad_xyz_inputs"])
    _check("grad_rotation_inputs", b["rotation_inputs"].grad, f32["grad_rotation_inputs"], f64["grad_rotation_inputs"])
    excluded = 0
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        if R.excluded_bias(k, c):
            excluded += 1
            continue
        _check("grad." + k, p.grad, f32["grad." + k], f64["grad." + k])
    assert excluded == 2 * (1 + 2 * c.num_stage)
    sd = m.state_dict()
    stats = [k for k in sd if k.endswith("running_mean") or k.endswith("running_var")]
    assert len(stats) == 4 * (1 + 2 * c.num_stage)
    for k in stats:
        _check("stat." + k, sd[k], f32["stat." + k], f64["stat." + k])
    assert all(int(v) == 1 for k, v in sd.items() if k.endswith("num_batches_tracked"))


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_network_eval_forward(name):
    c = R.cfg_of(name)
    out = {}
    for dtype in (torch.float64, torch.float32):
        s, b = R.to_torch(R.seeded_state(c), dtype), R.to_torch(R.seeded_batch(c), dtype)
        with torch.no_grad():
            out[dtype] = [v.double().numpy() for v in R.operate(s, c, b["xyz_inputs"], b["rotation_inputs"], False, True)]
    m, b = _model(c, train=False), _batch(c)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        xp, _, rp, _ = motion.operate(SimpleNamespace(norm_rotation=True), b, m)
    _check("xyz_pred", xp, out[torch.float32][0], out[torch.float64][0])
    _check("r_pred", rp, out[torch.float32][1], out[torch.float64][1])
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    with pytest.raises(RuntimeError, match="eval mode"):            # a gradient through the running statistics is refused
        motion.operate(SimpleNamespace(norm_rotation=True), b, m)


# ---- the rollout ------------------------------------------------------------------------------------------------------------------------
def _window(c):
    b = _batch(c)
    return b["xyz_inputs"][0].contiguous(), b["rotation_inputs"][0].contiguous()


@pytest.mark.parametrize("norm_rotation", [False, True])
@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_rollout(name, norm_rotation):
    c = R.cfg_of(name)
    (x64, r64), (x32, r32) = _ref_rollout(name, norm_rotation)
    m = _model(c, train=False)
    xyz, rot = _window(c)
    base = torch.tensor(np.random.default_rng(3).uniform(-1, 1, size=(c.K, 3)), dtype=torch.float32, device=DEV)
    F = R.ROLLOUT_FRAMES
    kx, kr, delta = m.rollout(xyz, rot, F, c.out, norm_rotation, base_xyz=base)
    assert kx.shape == (F * c.out, c.K, 3) and kr.shape == (F * c.out, c.K, 4) and delta.shape == (F * c.out, c.K, 7)
    for f in (0, 5, 11):
        rows = slice(f * c.out, (f + 1) * c.out)
        _check(f"frame {f} xyz", kx[rows], x32[rows], x64[rows])
        _check(f"frame {f} rot", kr[rows], r32[rows], r64[rows])
    assert torch.equal(delta, torch.cat([kx - base, kr], dim=-1))
    # the same numbers as 12 successive eval-mode forwards composed as [REF train_GCN.py:133-138], bit for bit
    args = SimpleNamespace(norm_rotation=norm_rotation)
    batch = {"xyz_inputs": xyz[None].clone(), "rotation_inputs": rot[None].clone(), "xyz_gt": None, "rotation_gt": None}
    sx, sr = [], []
    with torch.no_grad():
        for _ in range(F):
            xp, _, rp, _ = motion.operate(args, batch, m)
            sx += [xp[0][-c.out:, ...]]
            sr += [rp[0][-c.out:, ...]]
            batch["xyz_inputs"] = torch.cat([batch["xyz_inputs"][:, c.out:], xp[:, -c.out:, ...]], dim=1)
            batch["rotation_inputs"] = torch.cat([batch["rotation_inputs"][:, c.out:], rp[:, -c.out:, ...]], dim=1)
    sx, sr = torch.cat(sx, dim=0), torch.cat(sr, dim=0)
    print("rollout vs successive forwards: xyz", float((sx - kx).abs().max()), "rot", float((sr - kr).abs().max()))
    assert torch.equal(sx, kx) and torch.equal(sr, kr)
    # frame f of a rollout of F frames equals frame f of a rollout of f + 1 frames
    for f in (0, 5):
        px, pr = m.rollout(xyz, rot, f + 1, c.out, norm_rotation)
        assert torch.equal(px, kx[:(f + 1) * c.out]) and torch.equal(pr, kr[:(f + 1) * c.out])
    # and a second call gives the same bits
    kx2, kr2, delta2 = m.rollout(xyz, rot, F, c.out, norm_rotation, base_xyz=base)
    assert torch.equal(kx, kx2) and torch.equal(kr, kr2) and torch.equal(delta, delta2)


def test_train_pass_is_bit_reproducible():
    c = R.cfg_of("c1")
    runs = []
    for _ in range(2):
        m, b = _model(c), _batch(c, grad=True)
        xp, xg, rp, rg = motion.operate(SimpleNamespace(norm_rotation=True), b, m)
        motion.gcn_loss(xp, xg, rp, rg).backward()
        runs.append([xp.detach(), rp.detach(), b["xyz_inputs"].grad, b["rotation_inputs"].grad] + [p.grad for p in m.parameters()]
                    + [v for k, v in m.state_dict().items() if "running" in k])
    assert len(runs[0]) == len(runs[1]) and all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_three_adam_steps(name):
    c = R.cfg_of(name)
    a64, a32 = R.adam_losses(c, torch.float64), R.adam_losses(c, torch.float32)
    args = SimpleNamespace(norm_rotation=True, epoch=10)
    m, b = _model(c), _batch(c)
    optimizer, _ = motion.make_optimizer(args, m)
    assert optimizer.defaults["lr"] == 0.01 and optimizer.defaults["eps"] == 1e-15
    losses = [float(motion.train_iteration(args, m, optimizer, b)) for _ in range(3)]
    _check("adam losses", np.array(losses), a32, GOLD[f"{name}/adam_losses"])
    assert np.abs(a64 - GOLD[f"{name}/adam_losses"]).max() <= 1e-10 * np.abs(a64).max()
    assert all(int(v) == 3 for k, v in m.state_dict().items() if k.endswith("num_batches_tracked"))


def test_checkpoint_round_trip(tmp_path):
    c = R.cfg_of("c1")
    m = _model(c, train=False)
    xyz, rot = _window(c)
    a = m.rollout(xyz, rot, 4, c.out, True)
    path = os.path.join(tmp_path, "ckpt.pth")
    torch.save(m.state_dict(), path)
    fresh = motion.GCN_xyzr(c.T, c.H, c.out, 0, num_stage=c.num_stage, node_n=c.K, no_mapping=c.no_mapping).to(DEV)
    fresh.load_state_dict(torch.load(path), strict=True)
    b = fresh.eval().rollout(xyz, rot, 4, c.out, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- with the Gaussian model ---------------------------------------------------------------------------------------------------------------
W, H, IT = 96, 80, 100


def _stage3_model():
    """A small model past its third stage, built as eval.py restores one (create_from_pcd; no training set-up), with keypoints placed
    on the cloud and the hash-grid weights model + kNN evaluated inside forward."""
    from gaussian_renderer import GaussianModel
    from gaussianprediction_amd.cameras import orbit_cameras
    args = SimpleNamespace(beta=0.1, d=4, w=256, feature_dim=32, jointly_iteration=10, second_stage_iteration=40, third_stage_iteration=60,
                           nearest_num=6, norm_rotation=True, step_opacity=False, step_opacity_iteration=5000, opacity_type="implicit",
                           xyz_noise_iteration=0, max_points=24, adaptive_points_num=8, adaptive_from_iter=5, adaptive_end_iter=18,
                           adaptive_interval=5, densify_from_grad="True", densify_from_teaching=False, teaching_threshold=0.2,
                           knn_type="hybird", feature_amplify=5.0, max_gaussian_size=3000)
    rng = np.random.default_rng(2)
    pts = rng.uniform(-1.0, 1.0, size=(1500, 3)).astype(np.float32)
    cols = rng.uniform(0.1, 0.9, size=(1500, 3)).astype(np.float32)
    torch.manual_seed(0)
    g = GaussianModel(3, args)
    g.set_inputDim(2 * 6, 6 * 10)
    g.create_from_pcd(SimpleNamespace(points=pts, colors=cols, normals=np.zeros_like(pts)), 2.0)
    with torch.no_grad():
        g.super_gaussians.copy_(torch.tensor(pts[::60][:24], device=DEV))
        g.super_gaussians_feature.copy_(torch.tensor(rng.uniform(-0.1, 0.1, size=(24, 32)).astype(np.float32), device=DEV))
        g._rotation.copy_(torch.tensor(rng.normal(size=(1500, 4)).astype(np.float32), device=DEV))
    cams = orbit_cameras(6, 4.0, 0.69, W, H, device=DEV)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    return g, cams, pipe, torch.tensor([0, 0, 0], dtype=torch.float32, device=DEV)


def test_keypoint_motion_equals_the_side_outputs_of_forward():
    g, cams, pipe, bg = _stage3_model()
    for t in (0.0, 0.37):
        time_ = torch.tensor([t], dtype=torch.float32, device=DEV)
        with torch.no_grad():
            g(time_, IT)
            want_xyz, want_r = g.get_superGaussians + g.kpts_xyz_motion, g.kpts_rotation_motion
        got_xyz, got_r = g.keypoint_motion(time_, IT)
        assert got_xyz.shape == (24, 3) and got_r.shape == (24, 4) and float(g.kpts_xyz_motion.abs().max()) > 0
        assert torch.equal(got_xyz, want_xyz) and torch.equal(got_r, want_r)


def test_end_to_end_trajectories_training_rollout_render(tmp_path):
    from gaussian_renderer import render
    g, cams, pipe, bg = _stage3_model()
    times = [i / 20 for i in range(20)]                  # 16 training times below max_time = 0.8, 4 test times
    json.dump({"frames": [{"time": t} for t in times]}, open(tmp_path / "transforms_train.json", "w"))
    args = SimpleNamespace(input_size=5, linear_size=16, output_size=1, dropout=0, num_stage=1, no_mapping=False, batch_size=4, epoch=3,
                           noise_init=0.01, noise_step=2, norm_rotation=True, model_path=str(tmp_path), exp_name="gcn")
    kw = dict(iteration=IT, model_path=str(tmp_path), source_path=str(tmp_path), max_time=0.8, input_size=5, output_size=1)
    train, test = motion.GCN3DDataset(g, 6, split="train", **kw), motion.GCN3DDataset(g, 6, split="test", **kw)
    assert len(train.train_times) == 16 and len(train) == 10 and train.nodes_num == 24 and len(test) == 4
    log = []
    model = motion.train_gcn(args, train, generator=torch.Generator().manual_seed(0), log=log)
    assert len(log) == 3 and np.isfinite(log).all() and os.path.exists(tmp_path / "gcn" / "ckpt.pth")
    batch = test[0]
    kx, kr, delta = model.eval().rollout(batch["xyz_inputs"], batch["rotation_inputs"], 3, 1, True, base_xyz=g.super_gaussians)
    images = motion.render_kpts(cams, g, pipe, bg, kx, kr, IT, view_id=1, delta=delta)
    assert len(images) == 3 and all(im.shape == (3, H, W) and torch.isfinite(im).all() for im in images)
    again = motion.render_kpts(cams, g, pipe, bg, kx, kr, IT, view_id=1, out_dir=str(tmp_path / "pred"))
    assert all(torch.equal(a, b) for a, b in zip(images, again)) and os.path.exists(tmp_path / "pred" / "renders" / "view1" / "00002.png")
    # a frame rendered from the model's OWN keypoint motion equals render() of that time
    view = cams[2]
    time_ = torch.from_numpy(view.time).to(torch.float32).to(DEV)
    own_x, own_r = g.keypoint_motion(time_, IT)
    mine = motion.render_kpts([view], g, pipe, bg, own_x[None], own_r[None], IT, view_id=0)[0]
    with torch.no_grad():
        want = render(view, g, pipe, bg, time=time_, it=IT)["render"]
    print("render_kpts vs render:", float((mine - want).abs().max()))
    assert float(want.max()) > 0.05 and torch.allclose(mine, want, atol=1e-6)
