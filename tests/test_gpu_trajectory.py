"""The trajectory drawing on the device against the numpy restatement tests/trajectory_ref.py, bit for bit: every case of
tests/trajectory_cases.py through TrajectoryCanvas (the pixels after each step, the owner image, the picture over zero and over a
base, two runs), a multi-workgroup regime, and project_trajectory / keypoint_trails / render_trajectories on a small model."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import png_cases as P
import trajectory_cases as cases
import trajectory_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
H, W, IT = 163, 178, 50000


def same(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def draw(c, check_px=None):
    """(owner, image over zero [3, H, W], image over the base [H, W, 3]) of case c through a TrajectoryCanvas."""
    from gaussianprediction_amd.trajectory_ops import TrajectoryCanvas
    canvas = TrajectoryCanvas(c.view, c.P, DEV, H=c.H, W=c.W, colors=torch.from_numpy(c.colors), min_depth=c.min_depth)
    idx = None if c.idx is None else torch.from_numpy(c.idx).to(DEV)
    for s, xyz in enumerate(c.steps):
        canvas.step(torch.from_numpy(xyz).to(DEV), idx)
        if check_px is not None:
            assert same(canvas.px, check_px[s]), (c.name, s)
    assert canvas.steps == len(c.steps) and canvas.owner.dtype == torch.uint32
    return canvas.owner.cpu().numpy(), canvas.image(layout="chw"), canvas.image(torch.from_numpy(c.base).to(DEV))


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_case_equals_the_restatement_and_itself(name):
    c = cases.CASES[name]
    want_px, want_owner, want_plain, want_over = cases.reference(name)
    owner, plain, over = draw(c, check_px=want_px)
    assert same(owner, want_owner) and same(plain, want_plain)
    assert over.shape == (c.H, c.W, 3) and same(over.permute(2, 0, 1).contiguous(), want_over)
    again = draw(c)
    assert same(again[0], owner) and torch.equal(again[1], plain) and torch.equal(again[2], over)
    # the overlay leaves exactly the untouched pixels equal to the base
    base, touched = torch.from_numpy(c.base).to(DEV), torch.from_numpy(want_owner != 0).to(DEV)
    equal = (over.permute(2, 0, 1) == base).all(dim=0)
    assert torch.equal(equal, ~touched)


def test_many_workgroups_of_random_walks():
    c = cases.random_walks()
    assert c.P == 70000 and len(c.steps) == 4 and (c.H, c.W) == (240, 320)
    want_px, want_owner = ref.run(c.view, c.H, c.W, c.steps, None, c.P)
    owner, plain, _ = draw(c, check_px=want_px)
    assert same(owner, want_owner) and same(plain, ref.resolve(want_owner, c.colors, c.P))
    assert (want_owner != 0).mean() > 0.9 and want_owner.max() > 3 * c.P + 69000 and any((p == ref.NOT_DRAWABLE).sum() == 0 for p in want_px)


def test_step_and_image_refuse_what_they_cannot_draw():
    from gaussianprediction_amd import _lib
    from gaussianprediction_amd.trajectory_ops import TrajectoryCanvas
    view = cases.camera(True)
    canvas = TrajectoryCanvas(view, 4, DEV)
    assert (canvas.H, canvas.W) == (cases.H, cases.W) and canvas.colors.shape == (4, 3) and canvas.device == torch.device("cuda", torch.cuda.current_device())
    xyz = torch.zeros(6, 3, device=DEV)
    for bad_xyz, bad_idx, word in ((xyz.double(), None, "float32"), (xyz[:, :2], None, "float32"), (xyz.cpu(), None, "no CPU fallback"),
                                   (xyz, torch.zeros(4, dtype=torch.int64, device=DEV), "int32"), (xyz, torch.zeros(5, dtype=torch.int32, device=DEV), "int32"),
                                   (xyz, torch.zeros(4, dtype=torch.int32), "no CPU fallback")):
        with pytest.raises(RuntimeError, match=word):
            canvas.step(bad_xyz, bad_idx)
    with pytest.raises(_lib.GpHipError, match="at least P rows"):
        canvas.step(xyz[:3])
    assert canvas.steps == 0 and not canvas.owner.cpu().numpy().any()
    with pytest.raises(RuntimeError, match="base must be"):
        canvas.image(torch.zeros(3, cases.H, cases.W + 1, device=DEV))
    with pytest.raises(ValueError, match="layout"):
        canvas.image(layout="whc")
    with pytest.raises(RuntimeError, match="colors"):
        TrajectoryCanvas(view, 4, DEV, colors=torch.zeros(5, 3))
    canvas.steps = (2 ** 32 - 1) // 4                                     # the next step's keys would not fit 32 bits
    with pytest.raises(_lib.GpHipError, match=r"2\^32 - 1"):
        canvas.step(xyz)


@pytest.fixture(scope="module")
def scene():
    from test_gpu_render import build
    from gaussianprediction_amd.cameras import orbit_cameras
    pc = build(N=3000, K=60, W=W, H=H)[0]
    cams = orbit_cameras(5, 4.0, 0.6911, W, H, device=DEV)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    return SimpleNamespace(pc=pc, cams=cams, pipe=pipe, bg=torch.zeros(3, device=DEV))


def _render(scene, cam):
    import gaussianprediction_amd as gpa
    with torch.no_grad():
        return gpa.render(cam, scene.pc, scene.pipe, scene.bg, time=torch.from_numpy(cam.time).to(DEV), it=IT)


def test_project_trajectory_equals_the_restatement_on_the_models_own_positions(scene, monkeypatch):
    from gaussianprediction_amd import eval_render as ER
    cam = scene.cams[3]
    out = _render(scene, cam)
    tidx = out["tidx"]
    flat = tidx.reshape(-1).cpu().numpy()
    idx = flat[flat != -1].astype(np.int32)
    assert 500 < len(idx) <= H * W and len(np.unique(idx)) < len(idx)
    recorded, times, forward = [], [], scene.pc.forward

    def recording(t, iteration, *a, **kw):
        res = forward(t, iteration, *a, **kw)
        recorded.append(scene.pc._last_xyz_t.cpu().numpy().copy())
        times.append(float(t))
        return res

    monkeypatch.setattr(scene.pc, "forward", recording)
    got = ER.project_trajectory(scene.pc, cam, tidx, 6, IT, steps=5, seed=7)
    over = ER.project_trajectory(scene.pc, cam, tidx, 6, IT, steps=5, seed=7, base=out["render"], min_depth=0.2)
    monkeypatch.undo()
    assert len(recorded) == 10 and times[:5] == torch.linspace(0, float(cam.time[0]), 5).tolist() == times[5:] and times[4] > 0.5
    assert got.shape == (H, W, 3) and got.dtype == torch.float32 and got.is_cuda
    from gaussianprediction_amd.trajectory_ops import default_colors
    colors = default_colors(len(idx), 7).numpy()
    _, owner = ref.run(cam, H, W, recorded[:5], idx, len(idx))
    assert (owner != 0).sum() > 100 and owner.max() > 4 * len(idx)
    assert same(got.permute(2, 0, 1).contiguous(), ref.resolve(owner, colors, len(idx)))
    _, owner = ref.run(cam, H, W, recorded[5:], idx, len(idx), min_depth=0.2)
    assert same(over.permute(2, 0, 1).contiguous(), ref.resolve(owner, colors, len(idx), out["render"].cpu().numpy()))
    # one step, or a view that sees nothing: the base, or zero
    assert torch.equal(ER.project_trajectory(scene.pc, cam, tidx, 6, IT, steps=1, base=out["render"]), out["render"].permute(1, 2, 0))
    assert not ER.project_trajectory(scene.pc, cam, torch.full_like(tidx, -1), 6, IT, steps=5).any()


def test_keypoint_trails_equals_the_restatement(scene):
    from gaussianprediction_amd import eval_render as ER
    cam = scene.cams[1]
    steps = [scene.pc.keypoint_motion(torch.tensor([t], dtype=torch.float32, device=DEV), IT)[0] for t in (0.0, 0.2, 0.5, 0.7, 1.0)]
    kx = torch.stack(steps)
    K = kx.shape[1]
    colors = torch.rand(K, 3, generator=torch.Generator().manual_seed(1))
    got = ER.keypoint_trails(cam, kx, colors=colors)
    want_px, owner = ref.run(cam, H, W, [s.cpu().numpy() for s in steps], None, K)
    assert kx.shape == (5, 60, 3) and (owner != 0).sum() >= 10
    assert same(got.permute(2, 0, 1).contiguous(), ref.resolve(owner, colors.numpy(), K))


def test_render_trajectories_writes_its_directory_and_nothing_else(scene, tmp_path):
    from PIL import Image
    from gaussianprediction_amd import eval_render as ER
    root = str(tmp_path / "model")
    views = [scene.cams[2], scene.cams[4]]
    eval_path, stats = ER.render_trajectories(root, "test", IT, views, scene.pc, scene.pipe, scene.bg, steps=5)
    assert eval_path == os.path.join(root, "eval", "test") and stats["frames"] == 2 and stats["seconds"] > 0
    tree = sorted(os.path.relpath(os.path.join(d, f), root) for d, _, files in os.walk(root) for f in files)
    assert tree == [os.path.join("eval", "test", f"ours_{IT}", "trajectories", f"{i:05d}.png") for i in range(2)]
    assert sorted(os.listdir(os.path.join(eval_path, f"ours_{IT}"))) == ["trajectories"] and os.listdir(root) == ["eval"]
    for i, cam in enumerate(views):
        out = _render(scene, cam)
        want = ER.project_trajectory(scene.pc, cam, out["tidx"], None, IT, steps=5, base=out["render"])
        assert not torch.equal(want, out["render"].permute(1, 2, 0))
        got = np.array(Image.open(os.path.join(root, tree[i])))
        assert np.array_equal(got, P.quantise(want.permute(2, 0, 1).cpu().numpy()).transpose(1, 2, 0)), i
