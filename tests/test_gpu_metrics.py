"""GPU: gp_image_metrics (csrc/metric_kernels.hip) through gaussianprediction_amd.metrics and the pytorch_msssim shim, against the
float64 torch restatement of tests/metrics_ref.py and the reference's own numbers in tests/golden/metrics.npz.

Bars (test 1, 163 x 178, the smallest shape that still runs five pyramid levels: sizes (163,178), (82,89), (41,45), (21,23),
(11,12), odd and even on both axes, last valid map 1 x 2):
  SSIM, MS-SSIM, every per-level term: max(8 x |restatement32 - restatement64| of that quantity, 2e-6) from the float64 restatement
      (8: another summation order and a separable filter, both sides float32; 2e-6: the project's bar between two float32 summation
      orders of SSIM sums, test_gpu_loss_adam.py);
  L1, MSE: relative 5e-6 (float32 differences and squares, a 10-step float32 tree per 1 024-pixel tile at <= 6e-7 relative, then
      doubles; 8 x margin);  PSNR, PSNR_CH: 2e-5 dB (the same error x 10 / ln 10)."""
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import metrics_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIXED = 2e-6


@pytest.fixture(scope="module")
def probe():
    """The 163 x 178 pair, B = 2, and its restatement in both precisions (computed once on the CPU, never modified)."""
    render, gt = R.probe_pair(163, 178, 2, seed=0)
    r64 = R.all_metrics(render.double(), gt.double())
    r32 = {k: v.double() for k, v in R.all_metrics(render, gt).items()}
    return SimpleNamespace(render=render.cuda(), gt=gt.cuda(), r64=r64, r32=r32)


def _bar(probe, key):
    """Elementwise: every image's value (every term of "levels") has its OWN bar, max(8 x |ref32 - ref64| of that quantity, 2e-6)."""
    return torch.clamp(8.0 * (probe.r32[key] - probe.r64[key]).abs(), min=FIXED)


def _within(got, want, bar):
    return bool(((got - want).abs() <= bar).all())


def test_five_levels_against_the_restatement(probe):
    from gaussianprediction_amd import metrics as M
    r = M.image_metrics(probe.render, probe.gt, levels=True)
    assert r.names[:7] == ("L1", "MSE", "PSNR", "PSNR_CH", "SSIM", "MS_SSIM", "D_SSIM") and r.table.shape == (2, 8) and r.table.dtype == torch.float64
    t, lv = r.table.cpu(), r.levels.cpu()
    assert float(probe.r64["levels"].min()) > 0.6            # no ReLU active here
    got = {k: t[:, getattr(M, k)] for k in R.NAMES}
    got["levels"] = lv
    dist = {k: (got[k] - probe.r64[k]).abs() for k in got}
    for k in ("SSIM", "MS_SSIM", "levels"):
        d32 = (probe.r32[k] - probe.r64[k]).abs()
        print(f"[metrics] {k}: max |kernel - ref64| = {float(dist[k].max()):.3e}   |ref32 - ref64| = {float(d32.min()):.3e} .. {float(d32.max()):.3e}   "
              f"bars = {float(_bar(probe, k).min()):.3e} .. {float(_bar(probe, k).max()):.3e}   largest distance / its bar = {float((dist[k] / _bar(probe, k)).max()):.3f}")
    print("[metrics] levels, max |kernel - ref64| per scale: " + " ".join(f"{float(dist['levels'][:, l].max()):.2e}" for l in range(5)))
    for k in ("L1", "MSE"):
        print(f"[metrics] {k}: relative distance = {float((dist[k] / probe.r64[k]).max()):.3e}   bar = 5e-6")
    for k in ("PSNR", "PSNR_CH"):
        print(f"[metrics] {k}: |kernel - ref64| = {float(dist[k].max()):.3e} dB   bar = 2e-5")
    for k in ("SSIM", "MS_SSIM", "levels"):
        assert _within(got[k], probe.r64[k], _bar(probe, k)), (k, dist[k], _bar(probe, k))
    assert _within(got["D_SSIM"], probe.r64["D_SSIM"], _bar(probe, "MS_SSIM"))
    for k in ("L1", "MSE"):
        assert float((dist[k] / probe.r64[k]).max()) <= 5e-6, k
    for k in ("PSNR", "PSNR_CH"):
        assert float(dist[k].max()) <= 2e-5, (k, dist[k])
    assert torch.equal(t[:, 6], (1 - t[:, 5]) / 2) and torch.equal(t[:, 7], torch.zeros(2, dtype=torch.float64))
    # the conveniences are columns of the same call
    assert torch.equal(M.psnr(probe.render, probe.gt).cpu(), t[:, M.PSNR]) and torch.equal(M.ms_ssim(probe.render[1], probe.gt[1]).cpu(), t[1, M.MS_SSIM])


def test_partial_tiles_against_the_reference_vectors():
    from gaussianprediction_amd import metrics as M
    gold = np.load(os.path.join(HERE, "golden", "metrics.npz"))
    img, gt = (torch.from_numpy(x) for x in R.golden_pair(0))          # 37 x 45: one tile partial in both axes
    # three images with the same L1 / PSNR / PSNR_CH / SSIM: as recorded, mirrored (the window is symmetric), channels rolled
    a = torch.stack([img, img.flip(2), img.roll(1, 0)]).cuda()
    b = torch.stack([gt, gt.flip(2), gt.roll(1, 0)]).cuda()
    t = M.image_metrics(a, b, ms_ssim=False).table.cpu()
    assert bool(torch.isnan(t[:, 5:7]).all()) and not bool(torch.isnan(t[:, :5]).any())
    for row in range(3):
        assert abs(float(t[row, M.L1]) - float(gold["p0_l1"])) <= 2e-6 + 5e-6 * float(gold["p0_l1"])
        assert abs(float(t[row, M.SSIM]) - float(gold["p0_ssim"])) <= 2e-6 + FIXED
        assert abs(float(t[row, M.PSNR]) - float(gold["p0_psnr_13hw"])) <= 2e-5 + 2e-5
        assert abs(float(t[row, M.PSNR_CH]) - float(gold["p0_psnr_3hw"].mean())) <= 2e-5 + 2e-5
    img, gt = (torch.from_numpy(x).cuda() for x in R.golden_pair(1))   # 64 x 64: whole tiles, [3,H,W] accepted
    t = M.image_metrics(img, gt, ms_ssim=False).table.cpu()
    assert t.shape == (1, 8)
    assert abs(float(t[0, M.L1]) - float(gold["p1_l1"])) <= 2e-6 + 5e-6 * float(gold["p1_l1"])
    assert abs(float(t[0, M.SSIM]) - float(gold["p1_ssim"])) <= 2e-6 + FIXED
    assert abs(float(t[0, M.PSNR]) - float(gold["p1_psnr_13hw"])) <= 4e-5 and abs(float(t[0, M.PSNR_CH]) - float(gold["p1_psnr_3hw"].mean())) <= 4e-5


def test_too_small_for_five_scales_fails_before_any_launch():
    from gaussianprediction_amd import _lib, metrics as M
    x = torch.rand(1, 3, 160, 200, device="cuda")
    out = torch.full((1, 8), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.GpHipError, match=r"160.*200"):
        M.image_metrics(x, x, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((1, 8), 7.0, dtype=torch.float64))
    assert not bool(torch.isnan(M.image_metrics(x, x, ms_ssim=False, out=out).table[:, :5]).any())
    with pytest.raises(RuntimeError):
        M.image_metrics(torch.rand(1, 4, 170, 170, device="cuda"), torch.rand(1, 4, 170, 170, device="cuda"))


def test_entry_refuses_bad_arguments(probe):
    """The C entry's own validation, with real device memory behind every pointer (shapes and flags alone: test_metrics_host.py,
    through gp_image_metrics_scratch_bytes, which cannot launch)."""
    import ctypes as C
    from gaussianprediction_amd import _lib, metrics as M
    l = _lib.lib()
    a, b = probe.render[:1].contiguous(), probe.gt[:1].contiguous()
    out = torch.full((1, 8), 7.0, dtype=torch.float64, device="cuda")
    lv = torch.full((1, 5, 3), 7.0, dtype=torch.float64, device="cuda")
    q = torch.zeros(1, 3, 163, 178, dtype=torch.uint8, device="cuda")
    scratch = M.metrics_scratch(a.device, 1, 163, 178, 4)
    sp = (scratch.data_ptr() + 255) & ~255

    def call(channels=3, flags=4, levels=None, quant=None, scratch_ptr=sp, render=a):
        return l.gp_image_metrics(_lib.ptr(render), _lib.ptr(b), C.c_int32(1), C.c_int32(channels), C.c_int32(163), C.c_int32(178), C.c_uint32(flags),
                                  C.c_void_p(scratch_ptr) if scratch_ptr else None, None, _lib.ptr(out), _lib.ptr(levels), _lib.ptr(quant), None,
                                  _lib.stream_ptr(a.device))

    assert call(channels=4) == 1 and b"C=4" in l.gp_last_error()
    assert call(flags=0, levels=lv) == 1 and b"levels_out" in l.gp_last_error()
    assert call(flags=4, quant=q) == 1 and b"quant_out" in l.gp_last_error()
    assert call(scratch_ptr=0) == 1 and b"null" in l.gp_last_error()
    assert call(render=None) == 1 and b"null" in l.gp_last_error()
    assert call(scratch_ptr=sp + 4) == 1 and b"aligned" in l.gp_last_error()
    assert call(flags=16) == 1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((lv == 7.0).all())          # nothing ran
    assert call(levels=lv) == 0 and not bool(torch.isnan(out).any())


def test_relu_before_the_powers_and_the_perfect_image(probe):
    from gaussianprediction_amd import metrics as M
    r = M.image_metrics(1 - probe.gt, probe.gt, levels=True)
    t = r.table.cpu()
    assert float(r.levels.max()) < 0                         # all fifteen terms negative ...
    assert torch.equal(t[:, M.MS_SSIM], torch.zeros(2, dtype=torch.float64))     # ... exactly 0.0, not NaN
    assert torch.equal(t[:, M.D_SSIM], torch.full((2,), 0.5, dtype=torch.float64))
    t = M.image_metrics(probe.gt, probe.gt).table.cpu()
    one = torch.ones(2, dtype=torch.float64)
    assert _within(t[:, M.SSIM], one, _bar(probe, "SSIM")) and _within(t[:, M.MS_SSIM], one, _bar(probe, "MS_SSIM"))
    assert bool(torch.isinf(t[:, M.PSNR]).all()) and bool((t[:, M.PSNR] > 0).all()) and bool(torch.isinf(t[:, M.PSNR_CH]).all())
    assert torch.equal(t[:, :2], torch.zeros(2, 2, dtype=torch.float64))


def test_quantisation_and_error_image(probe):
    from gaussianprediction_amd import metrics as M
    g = torch.Generator().manual_seed(5)
    x = (probe.gt.cpu() + 0.3 * torch.randn(2, 3, 163, 178, generator=g)).contiguous()      # values below 0 and above 1
    assert float(x.min()) < 0 and float(x.max()) > 1
    want_q = (x * 255 + 0.5).clamp(0, 255).to(torch.uint8)          # float32: one multiply, one add
    r = M.image_metrics(x.cuda(), probe.gt, quantize8=True, quantized=True, deltas=True)
    assert r.quantized.dtype == torch.uint8 and torch.equal(r.quantized.cpu(), want_q)
    back = (want_q.to(torch.float32) / 255.0).contiguous()          # what loading the 8-bit file gives (a true division)
    plain = M.image_metrics(back.cuda(), probe.gt, deltas=True)
    assert torch.equal(r.table.cpu(), plain.table.cpu())
    want_d = ((back - probe.gt.cpu()).abs() * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    assert r.deltas.shape == (2, 163, 178, 3) and torch.equal(r.deltas.cpu(), want_d) and torch.equal(plain.deltas.cpu(), want_d)
    # clamp: both images, as loaded
    c = M.image_metrics(x.cuda(), probe.gt, clamp=True, ms_ssim=False).table.cpu()
    p = M.image_metrics(x.clamp(0, 1).cuda(), probe.gt, ms_ssim=False).table.cpu()
    assert torch.equal(c[:, :5], p[:, :5])
    with pytest.raises(RuntimeError):
        M.image_metrics(x.cuda(), probe.gt, quantized=True)


def test_reproducible_batched_rows_out_rows_and_invalid_flag(probe):
    from gaussianprediction_amd import metrics as M
    g = torch.Generator().manual_seed(9)
    render = torch.cat([probe.render.cpu(), (probe.gt.cpu()[:1] + 0.1 * torch.randn(1, 3, 163, 178, generator=g)).clamp(0, 1)]).cuda()
    gt = torch.cat([probe.gt, probe.gt[:1]])
    a = M.image_metrics(render, gt, levels=True)
    b = M.image_metrics(render, gt, levels=True)
    ta = a.table.cpu()
    assert not bool(torch.isnan(ta).any())
    assert torch.equal(ta, b.table.cpu()) and torch.equal(a.levels.cpu(), b.levels.cpu())
    for i in range(3):
        one = M.image_metrics(render[i], gt[i], levels=True)
        assert torch.equal(one.table.cpu()[0], ta[i]) and torch.equal(one.levels.cpu()[0], a.levels.cpu()[i])
    table = torch.full((4, 8), -3.0, dtype=torch.float64, device="cuda")
    r = M.image_metrics(render[:2], gt[:2], out=table[1:3])
    assert r.table.data_ptr() == table[1:3].data_ptr()
    h = table.cpu()
    assert torch.equal(h[1:3], ta[:2]) and torch.equal(h[0], torch.full((8,), -3.0, dtype=torch.float64)) and torch.equal(h[3], h[0])
    flag = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    f = M.image_metrics(render[:2], gt[:2], invalid_flag=flag, levels=True)
    assert torch.equal(f.table.cpu()[0], ta[0]) and bool(torch.isnan(f.table.cpu()[1]).all()) and bool(torch.isnan(f.levels.cpu()[1]).all())
    assert torch.equal(f.levels.cpu()[0], a.levels.cpu()[0])


def test_evaluate_views_equals_per_view_calls_and_survives_overflow(probe):
    from test_gpu_render import build
    import gaussianprediction_amd as gpa
    from gaussianprediction_amd import metrics as M
    from gaussianprediction_amd.cameras import orbit_cameras
    from gaussianprediction_amd.renderer import SpeculativeRenderer
    pc = build(N=3000, K=60, W=178, H=163)[0]
    cams = orbit_cameras(5, 4.0, 0.6911, 178, 163, device="cuda")[:4]
    times = [torch.tensor([0.1 + 0.2 * v], device="cuda") for v in range(len(cams))]
    gts = [probe.gt[v % 2] for v in range(len(cams))]
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    bg = torch.zeros(3, device="cuda")
    with torch.no_grad():
        want = torch.cat([M.image_metrics(gpa.render(cams[v], pc, pipe, bg, time=times[v], it=50000)["render"], gts[v], quantize8=True).table
                          for v in range(len(cams))]).cpu()
    assert not bool(torch.isnan(want).any())
    exact = M.evaluate_views(pc, cams, gts, pipe, bg, 50000, speculative=False, times=times)
    assert torch.equal(exact["per_view"].cpu(), want) and exact["rerendered"] == 0
    assert set(exact["summary"]) == {"SSIM", "PSNR", "MS-SSIM", "D-SSIM", "L1"}
    assert exact["summary"]["PSNR"] == float(want[:, M.PSNR].mean()) and exact["summary"]["MS-SSIM"] == float(want[:, M.MS_SSIM].mean())
    spec = M.evaluate_views(pc, cams, gts, pipe, bg, 50000, times=times)
    assert torch.equal(spec["per_view"].cpu(), want)
    # a capacity too small for every later frame: their rows come back NaN, the frames are re-rendered in place at flush(), the rows redone
    sr = SpeculativeRenderer(pc, pipe, bg)
    with torch.no_grad():
        sr(cams[0], time=times[0], it=50000)
    assert sr.last_status is None
    sr.capacity = 1024
    tight = M.evaluate_views(pc, cams, gts, pipe, bg, 50000, times=times, renderer=sr)
    assert tight["rerendered"] > 0 and sr.rerendered == tight["rerendered"] and sr.last_status is not None
    assert torch.equal(tight["per_view"].cpu(), want) and tight["summary"] == exact["summary"]
    rep = M.report_views(pc, cams, gts, pipe, bg, 50000, times=times)
    with torch.no_grad():
        cl = torch.cat([M.image_metrics(gpa.render(cams[v], pc, pipe, bg, time=times[v], it=50000)["render"], gts[v], clamp=True, ms_ssim=False).table
                        for v in range(len(cams))]).cpu()
    assert rep["L1"] == float(cl[:, M.L1].mean()) and rep["PSNR"] == float(cl[:, M.PSNR_CH].mean())


def test_evaluate_dirs_writes_the_reference_layout(probe, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from gaussianprediction_amd import metrics as M
    root = tmp_path / "run"
    (root / "ours" / "renders").mkdir(parents=True)
    (root / "ours" / "gt").mkdir()
    (root / "notes.txt").write_text("not a method")
    g = torch.Generator().manual_seed(3)
    names, pairs = [], []
    for i in range(3):
        gt8 = (probe.gt[i % 2].cpu() * 255).round().to(torch.uint8)
        r8 = ((probe.gt[i % 2].cpu() + 0.04 * (i + 1) * torch.randn(3, 163, 178, generator=g)).clamp(0, 1) * 255).round().to(torch.uint8)
        name = f"{i:05d}.png"
        Image.fromarray(r8.permute(1, 2, 0).numpy()).save(root / "ours" / "renders" / name)
        Image.fromarray(gt8.permute(1, 2, 0).numpy()).save(root / "ours" / "gt" / name)
        names.append(name)
        pairs.append((r8, gt8))
    Image.fromarray(pairs[0][0][0].numpy()).save(root / "ours" / "renders" / "00000_depth.png")       # skipped, as the reference does
    got = M.evaluate_dirs(str(root))
    want = torch.cat([M.image_metrics((r.float() / 255.0).cuda(), (t.float() / 255.0).cuda()).table for r, t in pairs]).cpu()
    res = json.load(open(root / "results.json"))
    per = json.load(open(root / "per_view.json"))
    cols = {"SSIM": M.SSIM, "PSNR": M.PSNR, "MS-SSIM": M.MS_SSIM, "D-SSIM": M.D_SSIM}
    assert set(res) == set(per) == set(cols)                 # (no LPIPS keys: documented)
    for k, c in cols.items():
        assert res[k] == float(want[:, c].mean()) == got["ours"]["summary"][k]
        assert per[k] == {n: float(want[i, c]) for i, n in enumerate(names)}
    assert sorted(os.listdir(root / "ours" / "deltas")) == ["00000.jpg", "00001.jpg", "00002.jpg"]
    assert Image.open(root / "ours" / "deltas" / "00001.jpg").size == (178, 163)


def test_pytorch_msssim_shim(probe):
    from gaussianprediction_amd import metrics as M
    from pytorch_msssim import ms_ssim
    col = M.image_metrics(probe.render, probe.gt).table[:, M.MS_SSIM]
    v = ms_ssim(probe.render, probe.gt, data_range=1, size_average=True)
    assert v.dim() == 0 and torch.equal(v.cpu(), col.mean().cpu())
    assert torch.equal(ms_ssim(probe.render, probe.gt, data_range=1, size_average=False).cpu(), col.cpu())
    w = ms_ssim(probe.render * 255, probe.gt * 255)          # data_range = 255 is the package's default
    per = ms_ssim(probe.render * 255, probe.gt * 255, size_average=False).cpu()
    assert _within(per, col.cpu(), _bar(probe, "MS_SSIM")) and _within(per, probe.r64["MS_SSIM"], _bar(probe, "MS_SSIM"))
    assert torch.equal(w.cpu(), per.mean())
    assert math.isfinite(float(w))
