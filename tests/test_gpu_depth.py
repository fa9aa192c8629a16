"""The depth entries on the device against the numpy restatement tests/depth_ref.py on every case of tests/depth_cases.py: bit for bit for
resolve, valid, the derived range, the LUT rows, normals and nvalid, points, colours, index and count, and the metric counts; the
float64 columns without a logf within 1e-12 relative; RMSE-log and SIlog within max(8 x |float32 restatement - float64 restatement|, 1e-9)
(logf is correctly rounded on neither side; the bar comes from the restatement, never from the device; the device's distances are
printed); every entry twice with equal bytes; a batch against its single rows; the physics of a fronto-parallel plane of Gaussians;
render_depths on two views.

Measured on an MI355X: see DESIGN section 25."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import depth_cases as cases
import depth_ref as ref
import png_cases as P
from test_depth_host import check_row
from test_gpu_flow import H, IT, W, Z0, _plain_camera, plane      # noqa: F401  (the 432-Gaussian plane at depth 3 and its camera)

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = np.float32


def same(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_view(v):
    """depth_ops' view of a case's view: the same float32 matrix and constants, on the device."""
    from gaussianprediction_amd import depth_ops as DO
    m = dev(v.c2w.reshape(4, 4))
    return DO.DepthView(m, v.tanfovx, v.tanfovy, v.W, v.H, DO.DepthViewC(m.data_ptr(), v.tanfovx, v.tanfovy, v.W, v.H))


# ---- every case against the restatement, and twice ----
@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_entry_equals_the_restatement_and_itself(name):
    from gaussianprediction_amd import depth_ops as DO
    c, want = cases.CASES[name], cases.reference(name)
    view, lut = device_view(c.view), dev(cases.lut())
    res = DO.resolve(dev(c.accum), dev(c.alpha), c.alpha_min)
    assert isinstance(res, DO.DepthResult) and res.valid.dtype == torch.bool
    assert same(res.depth, want.resolve[0]) and same(res.valid.view(torch.uint8), want.resolve[1]) and same(res.alpha, c.alpha)
    again = DO.resolve(dev(c.accum), dev(c.alpha), c.alpha_min)
    assert torch.equal(again.depth.view(torch.int32), res.depth.view(torch.int32)) and torch.equal(again.valid, res.valid)
    depth, valid, image = dev(c.depth), dev(c.valid), dev(c.image)
    for mname, mode, lo, hi in cases.COLOUR_MODES:
        for masked in (False, True):
            near, far = (None, None) if (lo, hi) == (0.0, 0.0) else (lo, hi)
            out, rng = DO.colorize(depth, valid if masked else None, "disparity" if mode == 1 else "depth", near, far, lut, cases.BG, return_range=True)
            w_out, w_rng, _ = want.colour[(mname, masked)]
            assert same(rng, w_rng), (mname, masked, rng, w_rng)                          # the range used, bit for bit
            assert same(out, w_out), (mname, masked)                                      # the LUT rows: every row of the table differs
            twice = DO.colorize(depth, (valid != 0) if masked else None, "disparity" if mode == 1 else "depth", near, far, lut, cases.BG)
            assert torch.equal(twice.view(torch.int32), out.view(torch.int32))
    for masked in (False, True):
        n, nvalid = DO.normals(depth, valid if masked else None, view)
        assert nvalid.dtype == torch.bool and same(n, want.normals[masked][0]) and same(nvalid.view(torch.uint8), want.normals[masked][1]), masked
        if masked:
            assert same(DO.normals_image(n, nvalid, cases.BG), want.picture)
        points, colors, index = DO.unproject(depth, valid if masked else None, view, image=image, return_index=True)
        w_points, w_colors, w_index, count = want.unproject[masked]
        assert points.shape == (count, 3) and same(points, w_points) and same(colors, w_colors) and same(index, w_index), masked
        alone = DO.unproject(depth, valid if masked else None, view)
        assert torch.is_tensor(alone) and torch.equal(alone.view(torch.int32), points.view(torch.int32))
    pred, gt, mask = dev(c.pred), dev(c.gt), dev(c.mask)
    for (masked, scaled), row in want.metrics.items():
        # (a scale comes in only through align; the entry's own scale argument is reached with a table whose column 9 holds it)
        table = _metrics_with_scale(DO, pred, gt, mask if masked else None, c.scale if scaled else None, c.gt_min, c.gt_max)
        assert table.shape == (1, 12) and table.dtype == torch.float64
        check_row(table[0].cpu().numpy(), row, want.metrics64[(masked, scaled)], ("device", name, masked, scaled))
        twice = _metrics_with_scale(DO, pred[None], gt[None], (mask[None] != 0) if masked else None, c.scale if scaled else None, c.gt_min, c.gt_max)
        assert torch.equal(twice.view(torch.int64), table.view(torch.int64))


def _metrics_with_scale(DO, pred, gt, mask, scale, gt_min, gt_max):
    """depth_metrics, or the entry itself with a given float32 scale per image (what align="scale" does with the scale it found)."""
    import ctypes as C
    from gaussianprediction_amd import _lib
    if scale is None:
        return DO.depth_metrics(pred, gt, mask, gt_min=gt_min, gt_max=gt_max)
    pred, gt = (t[None] if t.dim() == 2 else t for t in (pred, gt))
    B, Hh, Ww = pred.shape
    if mask is not None:
        mask = mask.reshape(B, Hh, Ww).contiguous().view(torch.uint8)
    s = torch.full((B,), float(scale), dtype=torch.float32, device=DEV)
    table = torch.empty(B, 12, dtype=torch.float64, device=DEV)
    scratch = _lib.scratch(DO.lib().gp_depth_metrics_scratch_bytes, B, Hh, Ww, device=pred.device)
    _lib.check(DO.lib().gp_depth_metrics(pred.contiguous(), gt.contiguous(), mask, s, gt_min, gt_max, B, Hh, Ww, scratch, table, _lib.stream_ptr(pred.device)),
               "gp_depth_metrics")
    return table


def test_a_batch_gives_the_single_rows_and_an_all_masked_image_a_nan_row():
    from gaussianprediction_amd import depth_ops as DO
    for x in (cases.CASES["37x53_random"], cases.CASES["240x320_random"]):
        pred, gt = np.stack([x.pred, x.gt, x.pred * F(0.5)]), np.stack([x.gt, x.pred, x.gt])
        mask = np.stack([x.mask, np.zeros_like(x.mask), x.valid])
        table = DO.depth_metrics(dev(pred), dev(gt), dev(mask), gt_min=x.gt_min, gt_max=x.gt_max)
        assert table.shape == (3, 12) and torch.isnan(table[1]).all() and not torch.isnan(table[[0, 2]]).any()
        for k in range(3):
            single = DO.depth_metrics(dev(pred[k]), dev(gt[k]), dev(mask[k]), gt_min=x.gt_min, gt_max=x.gt_max)
            assert torch.equal(single.view(torch.int64), table[k:k + 1].view(torch.int64)), k
        want, want64 = ref.metrics(pred, gt, mask, None, x.gt_min, x.gt_max), ref.metrics64(pred, gt, mask, None, x.gt_min, x.gt_max)
        for k in range(3):
            check_row(table[k].cpu().numpy(), want[k], want64[k], ("device batch", x.name, k))
        assert torch.equal(DO.depth_metrics(dev(pred), dev(gt), dev(mask), gt_min=x.gt_min, gt_max=x.gt_max).view(torch.int64), table.view(torch.int64))


def test_align_scale_finds_the_factor_without_a_read():
    from gaussianprediction_amd import depth_ops as DO
    x = cases.CASES["240x320_random"]
    gt = np.where(np.isfinite(x.gt) & (x.gt > 0), x.gt, F(2.0)).astype(F)
    pred = (F(0.5) * gt).astype(F)                                   # exact halves: 2 * pred is gt again, bit for bit
    plain = DO.depth_metrics(dev(pred), dev(gt)).cpu().numpy()[0]
    assert abs(plain[9] - 2.0) <= 1e-6 and abs(plain[1] - 0.5) <= 1e-6 and plain[5] == 0.0          # the scale column says 2; AbsRel is a half
    table = DO.depth_metrics(dev(pred), dev(gt), align="scale").cpu().numpy()[0]
    print("align=scale on pred = gt / 2: AbsRel", table[1], "scale of the first pass", plain[9])
    assert table[0] == gt.size and abs(table[1]) <= 1e-12 and table[5] == 1.0 and abs(table[9] - 1.0) <= 1e-6
    with pytest.raises(RuntimeError, match="align"):
        DO.depth_metrics(dev(pred), dev(gt), align="median")


def test_unproject_counts_and_orders_as_torch_does():
    from gaussianprediction_amd import depth_ops as DO
    for name in ("37x53_straddle", "240x320_tile_gap", "520x512_random"):
        c = cases.CASES[name]
        valid = dev(c.valid) != 0
        points, index = DO.unproject(dev(c.depth), valid, device_view(c.view), return_index=True)
        assert index.dtype == torch.int32 and points.shape[0] == index.shape[0] == int(valid.sum())
        assert torch.equal(index.long(), valid.flatten().nonzero().flatten())


def test_the_device_refusals():
    from gaussianprediction_amd import _lib, depth_ops as DO
    d, image = torch.ones(13, 17, device=DEV), torch.zeros(3, 13, 17, device=DEV)
    view = device_view(cases.view(True, 17, 13))
    for call, word in ((lambda: DO.resolve(d, d[:12]), "alpha must be"), (lambda: DO.colorize(d, torch.ones(13, 16, dtype=torch.bool, device=DEV)), "bool or uint8"),
                       (lambda: DO.colorize(d, torch.ones(13, 17, dtype=torch.bool)), "no CPU fallback"), (lambda: DO.colorize(d, background=(0, 0)), "three numbers"),
                       (lambda: DO.colorize(d, mode="inverse"), "mode"), (lambda: DO.colorize(d, near=1.0), "go together"),
                       (lambda: DO.colorize(d, lut=torch.zeros(255, 3, device=DEV)), r"\[256, 3\]"),
                       (lambda: DO.normals(d[:12], None, view), "the view is"), (lambda: DO.unproject(d, None, view, image=image[:, :12]), r"\[3, 13, 17\]"),
                       (lambda: DO.normals_image(image, None), "bool or uint8"), (lambda: DO.depth_metrics(d, d[:12]), "gt must be"),
                       (lambda: DO.depth_metrics(d, d, torch.ones(1, 13, 16, device=DEV)), "bool or uint8")):
        with pytest.raises(RuntimeError, match=word):
            call()
    for call, word in ((lambda: DO.colorize(d, near=float("nan"), far=1.0), "NaN"), (lambda: DO.resolve(d, d, float("nan")), "NaN"),
                       (lambda: DO.depth_metrics(d, d, gt_min=float("nan")), "NaN"),
                       (lambda: DO.depth_metrics(torch.zeros(0, 13, 17, device=DEV), torch.zeros(0, 13, 17, device=DEV)), "B must be > 0"),
                       (lambda: DO.resolve(torch.zeros(0, 17, device=DEV), torch.zeros(0, 17, device=DEV)), "H and W must be > 0")):
        with pytest.raises(_lib.GpHipError, match=word):
            call()
    jet = DO.colorize(d * 2.0, mode="depth", near=1.0, far=3.0)      # the default table: feature_vis.jet_lut, its row int(0.5 * 256)
    from gaussianprediction_amd import feature_vis
    assert torch.equal(jet[:, 0, 0], feature_vis.jet_lut(DEV)[128]) and torch.equal(jet, jet[:, :1, :1].expand(3, 13, 17))


# ---- physics: the fronto-parallel plane of test_gpu_flow.py at depth 3 ----
def test_a_fronto_parallel_plane_has_its_depth_its_normal_and_the_flows_alpha(plane):
    from gaussianprediction_amd import depth_ops as DO, flow_ops as FO
    cam = _plain_camera()
    del plane.calls[:]
    res = DO.render_depth(cam, plane.pc, plane.pipe, IT, time=0.0)
    assert plane.calls == [0.0]                                      # ONE render, one deformation pass
    assert res.depth.shape == (H, W) and res.alpha.shape == (H, W) and res.valid.dtype == torch.bool
    share = float(res.valid.float().mean())
    err = float((res.depth[res.valid] - Z0).abs().max())
    print("valid share", share, "largest |depth - 3| over the valid pixels", err)
    assert 0.5 < share < 1.0 and err <= 1e-4                         # DESIGN section 24's bound for the same composite and quotient
    assert (res.depth[~res.valid] == 0).all()
    flow = FO.render_flow(cam, plane.pc, plane.pipe, IT, 0.0, 0.0)
    assert torch.equal(res.alpha.view(torch.int32), flow.alpha.view(torch.int32)) and torch.equal(res.valid, flow.alpha >= 1e-3)
    n, nvalid = DO.normals(res.depth, res.valid, cam)
    inner = nvalid.clone()
    assert int(inner.sum()) > 0.4 * H * W
    nz = n[2][inner]
    print("interior normals: largest n_z", float(nz.max()))
    assert float(nz.max()) < -0.99
    points, index = DO.unproject(res.depth, res.valid, cam, return_index=True)
    assert points.shape[0] == int(res.valid.sum()) and float((points[:, 2] - Z0).abs().max()) <= 1e-4      # the camera is the world's frame
    assert DO.view_constants(cam) is DO.view_constants(cam)          # formed once per camera
    strict = DO.render_depth(cam, plane.pc, plane.pipe, IT, time=0.0, alpha_min=0.5)
    assert 0 < int(strict.valid.sum()) < int(res.valid.sum()) and torch.equal(strict.valid, res.alpha >= 0.5)


# ---- render_depths ----
@pytest.fixture(scope="module")
def scene():
    from test_gpu_render import build
    from gaussianprediction_amd.cameras import orbit_cameras
    w, h = 64, 48
    pc = build(N=3000, K=60, W=w, H=h)[0]
    cams = orbit_cameras(5, 4.0, 0.6911, w, h, device=DEV)[1:3]
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    return SimpleNamespace(pc=pc, cams=cams, pipe=pipe, bg=torch.zeros(3, device=DEV), white=torch.ones(3, device=DEV))


def _time(cam):
    return torch.from_numpy(cam.time).to(DEV)


def test_render_depths_writes_pictures_normals_pfm_and_ply_files(scene, tmp_path):
    from gaussianprediction_amd import depth_ops as DO, eval_render as ER, io_formats, png_decode
    root = str(tmp_path / "scene" / "model")
    out_dir, stats = ER.render_depths(root, "test", IT, scene.cams, scene.pc, scene.pipe, scene.white)
    top = os.path.dirname(out_dir)
    assert out_dir == os.path.join(root, "eval", "test", f"ours_{IT}", "depths") and stats["frames"] == 2 and stats["seconds"] > 0 and "video" not in stats
    assert sorted(os.listdir(out_dir)) == ["00000.png", "00001.png"] and sorted(os.listdir(top)) == ["depths"]
    out_dir, stats = ER.render_depths(root, "all", IT, [{"cam": c} for c in scene.cams], scene.pc, scene.pipe, scene.bg, mode="depth", near=2.0, far=6.0,
                                      normals=True, save_pfm=True, save_ply=True)
    top = os.path.dirname(out_dir)
    assert sorted(os.listdir(top)) == ["depths", "normals", "points"] and stats["frames"] == 2
    assert sorted(os.listdir(out_dir)) == ["00000.pfm", "00000.png", "00001.pfm", "00001.png"]
    assert sorted(os.listdir(os.path.join(top, "normals"))) == ["00000.png", "00001.png"] and sorted(os.listdir(os.path.join(top, "points"))) == ["00000.ply", "00001.ply"]
    for i, cam in enumerate(scene.cams):
        res = DO.render_depth(cam, scene.pc, scene.pipe, IT, time=_time(cam))
        assert 0.05 < float(res.valid.float().mean()) and 1.0 < float(res.depth[res.valid].mean()) < 8.0
        want = P.quantise(DO.colorize(res.depth, res.valid, "depth", 2.0, 6.0).cpu().numpy())
        got = png_decode.decode_files([os.path.join(out_dir, f"{i:05d}.png")], device=DEV)[0]
        assert same(got, want) and np.unique(want.reshape(3, -1), axis=1).shape[1] > 10
        own = P.quantise(DO.colorize(res.depth, res.valid).cpu().numpy())        # the first call: disparity, the frame's own range
        assert same(png_decode.decode_files([os.path.join(root, "eval", "test", f"ours_{IT}", "depths", f"{i:05d}.png")], device=DEV)[0], own)
        n, nvalid = DO.normals(res.depth, res.valid, cam)
        want = P.quantise(DO.normals_image(n, nvalid).cpu().numpy())
        assert same(png_decode.decode_files([os.path.join(top, "normals", f"{i:05d}.png")], device=DEV)[0], want) and bool(nvalid.any())
        assert torch.equal(DO.read_pfm(os.path.join(out_dir, f"{i:05d}.pfm")).view(torch.int32), res.depth.cpu().view(torch.int32))
        cloud = io_formats.read_ply_vertices(os.path.join(top, "points", f"{i:05d}.ply"))
        points = DO.unproject(res.depth, res.valid, cam)
        assert len(cloud) == int(res.valid.sum()) == points.shape[0] and set(cloud.dtype.names) == {"x", "y", "z", "red", "green", "blue"}
        assert np.array_equal(np.stack([cloud["x"], cloud["y"], cloud["z"]], axis=1), points.cpu().numpy().astype(np.float64))


def test_render_depths_video_and_a_callers_writer(scene, tmp_path):
    from gaussianprediction_amd import eval_render as ER, jpeg_decode, png_ops
    root = str(tmp_path / "scene" / "model")
    w = png_ops.PngWriter()
    out_dir, stats = ER.render_depths(root, "v", IT, scene.cams, scene.pc, scene.pipe, scene.bg, near=0.1, far=0.5, normals=True, writer=w, video=True)
    w.close()
    assert w.files == 4 and stats["frames"] == 2 and stats["video"] == os.path.join(os.path.dirname(out_dir), "scene_depths.avi")
    assert len(jpeg_decode.avi_frames(open(stats["video"], "rb").read(), "v.avi")[2]) == 2
