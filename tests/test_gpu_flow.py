"""The optical-flow entries on the device against the numpy restatement tests/flow_ref.py on every case of tests/flow_cases.py: bit for
bit for screen_flow, resolve, warp, valid, the count column and the derived max_flow; the colours within 1e-5 (atan2f is not
correctly rounded on either side); the float64 columns within 1e-12 relative (at most 3072 non-negative terms at 2^-53 each, about
3.4e-13); every entry twice with equal bytes; the multi-workgroup regimes; the physics of a plane of Gaussians that moves rigidly in
front of a static camera, and of a camera that moves instead; render_flows on three views."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import flow_cases as cases
import flow_ref as ref
import png_cases as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
COLOUR_BAR, F64_BAR = 1e-5, 1e-12
IT = 50000


def same(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def close64(got, want):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    fin = np.isfinite(want)
    return same(got[~fin], want[~fin]) and bool((np.abs(got[fin] - want[fin]) <= F64_BAR * np.abs(want[fin])).all())


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_view(v):
    """flow_ops' view of a case's view: the same float32 matrices, on the device."""
    from gaussianprediction_amd import flow_ops as FO
    return FO.view_constants(SimpleNamespace(world_view_transform=dev(v.vm.reshape(4, 4)), full_proj_transform=dev(v.pm.reshape(4, 4)),
                                             image_width=v.W, image_height=v.H))


# ---- every case against the restatement ----
@pytest.mark.parametrize("name", list(cases.PROJECT))
def test_screen_flow_equals_the_restatement_and_itself(name):
    from gaussianprediction_amd import flow_ops as FO
    v0, v1, xyz0, xyz1 = cases.PROJECT[name]
    d0 = device_view(v0)
    d1 = d0 if v1 is v0 else device_view(v1)
    got = FO.screen_flow(dev(xyz0), dev(xyz1), d0, None if v1 is v0 else d1)
    assert got.shape == (len(xyz0), 3) and same(got, cases.reference_project(name))
    assert torch.equal(FO.screen_flow(dev(xyz0), dev(xyz1), d0, d1).view(torch.int32), got.view(torch.int32))


def check_fields(c, want, FO):
    flow, valid, gt, mask = dev(c.flow), dev(c.valid), dev(c.gt), dev(c.mask)
    for mode, max_flow, bg in cases.COLOUR_MODES:
        for masked in (False, True):
            image, scale = FO.colorize(flow, valid if masked else None, max_flow, bg, return_scale=True)
            want_image, want_scale = want.colour[(mode, masked)]
            assert same(scale, np.array([want_scale], np.float32)), (mode, masked)           # the derived max_flow, bit for bit
            err = float(np.abs(image.cpu().numpy() - want_image).max())
            print(c.name, mode, masked, "colour error", err)
            assert err <= COLOUR_BAR and float(image.min()) >= 0.0 and float(image.max()) <= 1.0
            again = FO.colorize(flow, valid.view(torch.bool) if masked else None, max_flow, bg)
            assert torch.equal(again, image)
    for masked in (False, True):
        table = FO.flow_metrics(flow, gt, mask if masked else None)
        assert table.shape == (1, 8) and table.dtype == torch.float64
        row = table[0].cpu().numpy()
        assert same(row[:1], want.metrics[masked][:1]) and close64(row, want.metrics[masked]), (masked, row, want.metrics[masked])
        assert same(FO.flow_metrics(flow[None], gt[None], (mask[None] != 0) if masked else None), table.cpu().numpy())
    for image, wanted in ((c.image, want.warp), (c.flow, want.warp_flow)):
        got = FO.warp(dev(image), flow)
        assert same(got, wanted) and same(FO.warp(dev(image), flow), wanted)


@pytest.mark.parametrize("name", list(cases.FIELDS))
def test_fields_equal_the_restatement_and_themselves(name):
    from gaussianprediction_amd import flow_ops as FO
    c, want = cases.FIELDS[name], cases.reference_fields(name)
    res = FO.resolve(dev(c.composite), c.alpha_min)
    assert isinstance(res, FO.FlowResult) and res.valid.dtype == torch.bool
    assert same(res.flow, want.resolve[0]) and same(res.alpha, want.resolve[1]) and same(res.valid.view(torch.uint8), want.resolve[2])
    again = FO.resolve(dev(c.composite), c.alpha_min)
    assert all(same(a, b.cpu().numpy()) for a, b in zip(again, res))
    check_fields(c, want, FO)


# ---- the multi-workgroup regimes ----
def test_screen_flow_on_many_workgroups():
    from gaussianprediction_amd import flow_ops as FO
    rng = np.random.default_rng(31)
    v0, v1 = cases.view(True, 64, 48), cases.view(False, 64, 48)
    N = 70000
    cam = np.stack([rng.uniform(-2, 2, N), rng.uniform(-2, 2, N), rng.uniform(-0.5, 5, N)], axis=1)
    xyz0 = cases.world(v0, cam)
    xyz1 = xyz0 + rng.normal(0, 0.05, (N, 3)).astype(np.float32)
    want = ref.project(v0, v1, xyz0, xyz1)
    got = FO.screen_flow(dev(xyz0), dev(xyz1), device_view(v0), device_view(v1))
    assert same(got, want) and 0.3 < want[:, 2].mean() < 0.95 and want[-100:, 2].sum() > 10      # (the last workgroup's rows too)


def test_metrics_and_colour_on_many_workgroups_and_on_one_pixel():
    from gaussianprediction_amd import flow_ops as FO
    c = cases.big_field()
    assert (c.H, c.W) == (240, 320)
    want = SimpleNamespace(colour={(m, k): ref.colorize(c.flow, c.valid if k else None, mf, bg) for m, mf, bg in cases.COLOUR_MODES for k in (False, True)},
                           metrics={k: ref.metrics(c.flow[None], c.gt[None], c.mask[None] if k else None)[0] for k in (False, True)},
                           warp=ref.warp(c.image, c.flow), warp_flow=ref.warp(c.flow, c.flow))
    check_fields(c, want, FO)
    one = cases.one_pixel()
    want = SimpleNamespace(colour={(m, k): ref.colorize(one.flow, one.valid if k else None, mf, bg) for m, mf, bg in cases.COLOUR_MODES for k in (False, True)},
                           metrics={k: ref.metrics(one.flow[None], one.gt[None], one.mask[None] if k else None)[0] for k in (False, True)},
                           warp=ref.warp(one.image, one.flow), warp_flow=ref.warp(one.flow, one.flow))
    assert want.metrics[True].tolist() == [1.0, float(np.sqrt(np.float32(0.25 + 16.0))), 1.0, 1.0, 0.0, 1.0, float(np.sqrt(np.float32(5.0))), 0.0]
    check_fields(one, want, FO)


def test_a_batch_gives_the_single_rows_and_an_all_masked_image_a_nan_row():
    from gaussianprediction_amd import flow_ops as FO
    for x in (cases.FIELDS["64x48"], cases.big_field()):
        flow = np.stack([x.flow, x.gt, x.flow * np.float32(0.5)])
        gt = np.stack([x.gt, x.flow, x.gt])
        mask = np.stack([x.mask, np.zeros_like(x.mask), x.valid])
        table = FO.flow_metrics(dev(flow), dev(gt), dev(mask))
        assert table.shape == (3, 8) and torch.isnan(table[1]).all() and not torch.isnan(table[[0, 2]]).any()
        for k in range(3):
            single = FO.flow_metrics(dev(flow[k]), dev(gt[k]), dev(mask[k]))
            assert torch.equal(single.view(torch.int64), table[k:k + 1].view(torch.int64)), k
        want = ref.metrics(flow, gt, mask)
        assert same(table[:, 0], want[:, 0]) and close64(table, want)
        assert torch.equal(FO.flow_metrics(dev(flow), dev(gt), dev(mask)).view(torch.int64), table.view(torch.int64))


def test_the_device_refusals():
    from gaussianprediction_amd import _lib, flow_ops as FO
    flow, image = torch.zeros(2, 13, 17, device=DEV), torch.zeros(3, 13, 17, device=DEV)
    view = device_view(cases.view(True, 17, 13))
    for call, word in ((lambda: FO.screen_flow(torch.zeros(5, 3, device=DEV), torch.zeros(6, 3, device=DEV), view), r"\[5, 3\]"),
                       (lambda: FO.colorize(flow, torch.ones(13, 16, dtype=torch.bool, device=DEV)), "bool or uint8"),
                       (lambda: FO.colorize(flow, torch.ones(13, 17)), "bool or uint8"),
                       (lambda: FO.colorize(flow, torch.ones(13, 17, dtype=torch.bool)), "no CPU fallback"),
                       (lambda: FO.colorize(flow, background=(0, 0)), "three numbers"),
                       (lambda: FO.flow_metrics(flow, flow[:, :12]), "gt must be"), (lambda: FO.flow_metrics(flow, flow, torch.ones(1, 13, 17, device=DEV)), "bool or uint8"),
                       (lambda: FO.warp(image, flow[:, :12]), "flow must be")):
        with pytest.raises(RuntimeError, match=word):
            call()
    for call, word in ((lambda: FO.colorize(flow, max_flow=float("nan")), "NaN"), (lambda: FO.resolve(image, float("nan")), "NaN"),
                       (lambda: FO.flow_metrics(torch.zeros(0, 2, 13, 17, device=DEV), torch.zeros(0, 2, 13, 17, device=DEV)), "B must be > 0"),
                       (lambda: FO.resolve(torch.zeros(3, 0, 17, device=DEV)), "H and W must be > 0")):
        with pytest.raises(_lib.GpHipError, match=word):
            call()
    assert FO.screen_flow(torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, device=DEV), view).shape == (0, 3)


# ---- physics: a plane that moves rigidly in front of a static camera ----
W, H, FOVX, Z0, DX = 64, 48, 0.9, 3.0, 0.2


def _plain_camera(T=(0.0, 0.0, 0.0), time=0.0):
    from gaussianprediction_amd.cameras import Camera, focal2fov, fov2focal
    return Camera(R=np.eye(3), T=np.asarray(T, dtype=np.float64), FoVx=FOVX, FoVy=focal2fov(fov2focal(FOVX, W), H), width=W, height=H, time=time, device=DEV)


@pytest.fixture(scope="module")
def plane():
    """A model whose forward is a stub: its Gaussians lie on the plane z = Z0, facing the camera, at x + DX * t."""
    from test_gpu_render import build
    pc = build(N=432, K=20, W=W, H=H)[0]
    N = pc.get_xyz.shape[0]
    assert N == 432
    half_x, half_y = math.tan(FOVX / 2) * Z0 * 0.75, math.tan(FOVX / 2) * Z0 * 0.75 * H / W      # (a border of the image stays empty)
    gx, gy = np.meshgrid(np.linspace(-half_x, half_x, 24), np.linspace(-half_y, half_y, 18))
    base = torch.from_numpy(np.stack([gx.reshape(-1), gy.reshape(-1), np.full(N, Z0)], axis=1).astype(np.float32)).to(DEV)
    rot = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=DEV).repeat(N, 1)
    scales = torch.full((N, 3), 0.07, device=DEV)
    opacity = torch.full((N, 1), 0.7, device=DEV)
    shift = torch.tensor([DX, 0.0, 0.0], device=DEV)
    calls = []

    def forward(t, iteration, *a, raw_activations=False, **kw):
        pc._forward_raw = False
        calls.append(float(t))
        xyz = base + shift * t.to(DEV, torch.float32).reshape(-1)[:1]
        pc._last_xyz_t = xyz
        return xyz, rot, scales, opacity

    pc.forward = forward
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    return SimpleNamespace(pc=pc, pipe=pipe, calls=calls, N=N)


EXPECTED = (W / (2 * math.tan(FOVX / 2))) * DX / Z0          # px for one unit of time


def test_a_rigid_shift_gives_the_pinhole_flow_at_every_valid_pixel(plane):
    import gaussianprediction_amd as gpa
    from gaussianprediction_amd import flow_ops as FO
    cam = _plain_camera()
    del plane.calls[:]
    res = FO.render_flow(cam, plane.pc, plane.pipe, IT, 0.0, 1.0)
    assert plane.calls == [0.0, 1.0, 0.0]                               # three deformation passes, the render at time0
    assert res.flow.shape == (2, H, W) and res.alpha.shape == (H, W) and res.valid.shape == (H, W) and res.valid.dtype == torch.bool
    valid = res.valid
    share = float(valid.float().mean())
    err_x = float((res.flow[0][valid] - EXPECTED).abs().max())
    err_y = float(res.flow[1][valid].abs().max())
    print("expected", EXPECTED, "valid share", share, "errors", err_x, err_y)
    assert abs(EXPECTED) <= 10 and 0.5 < share < 1.0
    # all contributors carry the same displacement: about 50 accumulations x 2^-24 x 10 = 3e-5
    assert err_x <= 1e-4 and err_y <= 1e-4
    assert (res.flow[:, ~valid] == 0).all()
    # valid is false wherever the render's alpha is below alpha_min -- the alpha of an ordinary render of ones
    with torch.no_grad():
        ones = gpa.render(cam, plane.pc, plane.pipe, torch.zeros(3, device=DEV), time=torch.zeros(1, device=DEV), it=IT,
                          override_color=torch.ones(plane.N, 3, device=DEV))["render"]
    assert torch.equal(res.alpha, ones[2]) and torch.equal(valid, ones[2] >= 1e-3)
    strict = FO.render_flow(cam, plane.pc, plane.pipe, IT, 0.0, 1.0, alpha_min=0.5)
    assert torch.equal(strict.valid, ones[2] >= 0.5) and 0 < int(strict.valid.sum()) < int(valid.sum())
    # half the time, half the flow; backwards, the opposite
    half = FO.render_flow(cam, plane.pc, plane.pipe, IT, 0.0, 0.5)
    assert float((half.flow[0][half.valid] - EXPECTED / 2).abs().max()) <= 1e-4
    back = FO.render_flow(cam, plane.pc, plane.pipe, IT, 1.0, 0.0)
    assert float((back.flow[0][back.valid] + EXPECTED).abs().max()) <= 1e-4 and float(back.flow[1][back.valid].abs().max()) <= 1e-4
    # the photometric check the warp is for: frame 1 pulled back by the flow is frame 0, where the flow is valid and stays inside
    colours = torch.rand(plane.N, 3, generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        f0, f1 = (gpa.render(cam, plane.pc, plane.pipe, torch.zeros(3, device=DEV), time=torch.full((1,), t, device=DEV), it=IT,
                             override_color=colours)["render"] for t in (0.0, 1.0))
    pulled = FO.warp(f1, res.flow)
    inside = valid.clone()
    inside[:, W - 6:] = False
    left, moved = float((pulled - f0)[:, inside].abs().mean()), float((f1 - f0)[:, inside].abs().mean())
    print("photometric: mean |warp(f1) - f0|", left, "against mean |f1 - f0|", moved)
    assert left < 0.25 * moved


def test_a_camera_that_moves_instead_gives_the_opposite_sign(plane):
    from gaussianprediction_amd import flow_ops as FO
    cam0, cam1 = _plain_camera(), _plain_camera(T=(-DX, 0.0, 0.0))      # the camera moves by +DX along x: the world moves by -DX before it
    res = FO.render_flow(cam0, plane.pc, plane.pipe, IT, 0.0, 0.0, view1=cam1)
    valid = res.valid
    err_x, err_y = float((res.flow[0][valid] + EXPECTED).abs().max()), float(res.flow[1][valid].abs().max())
    print("camera motion: errors", err_x, err_y)
    assert float(valid.float().mean()) > 0.5 and err_x <= 1e-4 and err_y <= 1e-4
    still = FO.render_flow(cam0, plane.pc, plane.pipe, IT, 0.3, 0.3)
    assert still.valid.any() and not still.flow.any()                   # nothing moves: exact zeros


# ---- render_flows ----
@pytest.fixture(scope="module")
def scene():
    from test_gpu_render import build
    from gaussianprediction_amd.cameras import orbit_cameras
    w, h = 178, 163
    pc = build(N=3000, K=60, W=w, H=h)[0]
    cams = orbit_cameras(5, 4.0, 0.6911, w, h, device=DEV)[1:4]
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    return SimpleNamespace(pc=pc, cams=cams, pipe=pipe, bg=torch.zeros(3, device=DEV), white=torch.ones(3, device=DEV))


def _time(cam):
    return torch.from_numpy(cam.time).to(DEV)


def test_render_flows_writes_pictures_flo_files_and_a_video(scene, tmp_path):
    from gaussianprediction_amd import eval_render as ER, flow_ops as FO, jpeg_decode, png_decode, png_ops
    root = str(tmp_path / "scene" / "model")
    # neighbouring views: V - 1 frames, each scaled by itself
    out_dir, stats = ER.render_flows(root, "test", IT, scene.cams, scene.pc, scene.pipe, scene.white, save_flo=True)
    assert out_dir == os.path.join(root, "eval", "test", f"ours_{IT}", "flows") and stats["frames"] == 2 and stats["seconds"] > 0 and "video" not in stats
    assert sorted(os.listdir(out_dir)) == ["00000.flo", "00000.png", "00001.flo", "00001.png"]
    assert sorted(os.listdir(os.path.dirname(out_dir))) == ["flows"]
    for i in range(2):
        res = FO.render_flow(scene.cams[i], scene.pc, scene.pipe, IT, _time(scene.cams[i]), _time(scene.cams[i + 1]), view1=scene.cams[i + 1])
        assert float(res.valid.float().mean()) > 0.05 and float(res.flow.abs().max()) > 1.0
        assert torch.equal(FO.read_flo(os.path.join(out_dir, f"{i:05d}.flo")).view(torch.int32), res.flow.cpu().view(torch.int32))
        want = P.quantise(FO.colorize(res.flow, res.valid).cpu().numpy())
        got = png_decode.decode_files([os.path.join(out_dir, f"{i:05d}.png")], device=DEV)[0]
        assert same(got, want) and np.unique(want.reshape(3, -1), axis=1).shape[1] > 50
    # one camera over a time step: V frames, one scale, a caller's writer, the video
    w = png_ops.PngWriter()
    out_dir, stats = ER.render_flows(root, "step", IT, [{"cam": c} for c in scene.cams], scene.pc, scene.pipe, scene.bg, dt=0.1, max_flow=5.0, writer=w, video=True)
    w.close()
    assert w.files == 3 and stats["frames"] == 3 and sorted(os.listdir(out_dir)) == [f"{i:05d}.png" for i in range(3)]
    assert stats["video"] == os.path.join(os.path.dirname(out_dir), "scene_flows.avi")
    assert len(jpeg_decode.avi_frames(open(stats["video"], "rb").read(), "v.avi")[2]) == 3
    for i, cam in enumerate(scene.cams):
        res = FO.render_flow(cam, scene.pc, scene.pipe, IT, _time(cam), _time(cam) + 0.1)
        want = P.quantise(FO.colorize(res.flow, res.valid, 5.0).cpu().numpy())
        assert same(png_decode.decode_files([os.path.join(out_dir, f"{i:05d}.png")], device=DEV)[0], want), i


def test_the_scenes_background_does_not_reach_the_flow(scene, tmp_path):
    from gaussianprediction_amd import eval_render as ER
    a, _ = ER.render_flows(str(tmp_path / "a"), "t", IT, scene.cams[:2], scene.pc, scene.pipe, scene.bg, dt=0.2, save_flo=True)
    b, _ = ER.render_flows(str(tmp_path / "b"), "t", IT, scene.cams[:2], scene.pc, scene.pipe, scene.white, dt=0.2, save_flo=True)
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) == ["00000.flo", "00000.png", "00001.flo", "00001.png"]
    for n in names:
        assert open(os.path.join(a, n), "rb").read() == open(os.path.join(b, n), "rb").read(), n
