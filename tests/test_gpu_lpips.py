"""GPU: the LPIPS kernels (csrc/lpips_kernels.hip) against the float64 torch restatement of tests/lpips_ref.py on the seeded
recipe -- the convolution and the max-pool below the networks' own sizes, then both networks end to end, and the evaluation loops.

The bar of every comparison with float64 is relative and COMPUTED HERE on the CPU: 8 x the largest distance, over all of that
test's cases, of the float32 CPU run of the same restatement from its float64 run -- the reference's own arithmetic in its own
precision, pooled so that one lucky case cannot shrink it; 8 x is the margin test_gpu_metrics.py gives a kernel whose summation
order differs.  For a feature map the distance is max |a - b| / max |b| (ReLU zeros rule out an element-wise ratio)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R
from gaussianprediction_amd import _lib, lpips as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 8.0

# (Cin, Cout, k, stride, pad, N, H, W): the three kernel shapes of the nets, channel counts that are no multiple of 4 (the scalar
# staging path) or of the 64 / 128 column tile, a 1 x 1 kernel, K tails (K = 363, 125, 27, 45); 2 x 131 x 67 = 17554 output pixels
# span 274 row tiles of 64 plus a ragged one, with Cout = 130 = one column tile and two columns.  Those are all on the 64-row side of
# the kernel's tile choice (at most 512 workgroups of 128 rows); the last three are on the 128-row side, one per remaining variant:
# 128 x 128 with float4 staging (269 x 2 workgroups), 128 x 64 scalar and 128 x 64 float4 (518 workgroups), ragged last tiles.
CONV_CASES = [(3, 64, 11, 4, 2, 2, 19, 23), (5, 7, 5, 1, 2, 2, 19, 23), (64, 192, 3, 1, 1, 2, 19, 23), (3, 7, 3, 1, 1, 2, 19, 23),
              (192, 64, 1, 1, 0, 2, 19, 23), (5, 130, 3, 1, 1, 2, 131, 67),
              (8, 130, 3, 1, 1, 2, 131, 131), (5, 7, 3, 2, 1, 2, 365, 361), (4, 64, 1, 1, 0, 2, 183, 181)]


def _maxrel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max())


@pytest.fixture(scope="module")
def conv_ref():
    out = []
    for n, (cin, cout, k, s, p, N, H, W) in enumerate(CONV_CASES):
        g = torch.Generator().manual_seed(40 + n)
        x = torch.randn(N, cin, H, W, generator=g)
        w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        b = 0.05 * torch.randn(cout, generator=g)
        y64 = F.relu(F.conv2d(x.double(), w.double(), b.double(), stride=s, padding=p))
        y32 = F.relu(F.conv2d(x, w, b, stride=s, padding=p))
        out.append(SimpleNamespace(x=x, w=w, b=b, y64=y64, d32=_maxrel(y32, y64)))
    worst = max(c.d32 for c in out)
    return SimpleNamespace(cases=out, worst=worst, bar=MARGIN * worst)


def _conv(x, w, b, s, p):
    N, cin, H, W = x.shape
    cout, _, k, _ = w.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    wd, bd = w.contiguous().to(DEV), b.to(DEV)
    packed = torch.empty(cout * k * k * cin, device=DEV)
    y = torch.full((N, Ho, Wo, cout), float("nan"), device=DEV)
    _lib.check(L.lib().gp_lpips_conv2d_relu(xd, wd, bd, packed, y, N, H, W, cin, cout, k, s, p, _lib.stream_ptr(torch.device(DEV, 0))),
               "gp_lpips_conv2d_relu")
    return y.permute(0, 3, 1, 2).cpu()


@pytest.mark.parametrize("n", range(len(CONV_CASES)))
def test_conv2d_relu_against_float64(conv_ref, n):
    c = conv_ref.cases[n]
    _, _, k, s, p, _, _, _ = CONV_CASES[n]
    y = _conv(c.x, c.w, c.b, s, p)
    assert y.shape == c.y64.shape and not bool(torch.isnan(y).any())
    d = _maxrel(y, c.y64)
    print(f"conv case {CONV_CASES[n]}: gpu {d:.3e}  cpu float32 {c.d32:.3e}  pooled {conv_ref.worst:.3e}  bar {conv_ref.bar:.3e}")
    assert d <= conv_ref.bar, (d, conv_ref.bar)
    assert bool(((y == 0) == (c.y64 <= 0))[(c.y64.abs() > 1e-5)].all())          # the ReLU, away from the rounding at zero


@pytest.mark.parametrize("k,s,C,H,W", [(3, 2, 5, 19, 23), (2, 2, 5, 19, 23), (3, 2, 64, 15, 7), (2, 2, 64, 15, 7), (3, 2, 8, 3, 3)])
def test_maxpool_is_exact(k, s, C, H, W):
    x = torch.randn(2, C, H, W, generator=torch.Generator().manual_seed(7))
    want = F.max_pool2d(x, k, s)
    y = torch.full((2, want.shape[2], want.shape[3], C), float("nan"), device=DEV)
    _lib.check(L.lib().gp_lpips_maxpool(x.permute(0, 2, 3, 1).contiguous().to(DEV), y, 2, H, W, C, k, s, _lib.stream_ptr(torch.device(DEV, 0))),
               "gp_lpips_maxpool")
    assert torch.equal(y.permute(0, 3, 1, 2).cpu(), want)


def test_building_blocks_refuse_bad_arguments():
    l = L.lib()
    t = torch.zeros(4096, device=DEV)
    assert l.gp_lpips_maxpool(t, t, 1, 2, 5, 4, 3, 2, None) != 0 and b"empty output" in l.gp_last_error()
    assert l.gp_lpips_conv2d_relu(t, t, t, t, t, 1, 2, 2, 4, 4, 5, 1, 0, None) != 0 and b"empty output" in l.gp_last_error()
    assert l.gp_lpips_conv2d_relu(t, t, t, t, None, 1, 2, 2, 4, 4, 1, 1, 0, None) != 0 and b"null" in l.gp_last_error()


# ---- both networks end to end ------------------------------------------------------------------
FULL_CASES = [("alex", 67, 83), ("alex", 31, 50), ("vgg", 67, 83), ("vgg", 16, 40)]       # (the second of each: the minimum size)


@pytest.fixture(scope="module")
def models():
    out = {}
    for net in ("alex", "vgg"):
        w = R.seeded_weights(net)
        out[net] = SimpleNamespace(w=w, m=L.LPIPS(net, w["backbone"], w["lin"], device=DEV))
    return out


@pytest.fixture(scope="module")
def full_ref():
    out = {}
    for n, (net, H, W) in enumerate(FULL_CASES):
        w = R.seeded_weights(net)
        pairs = [R.image_pair(H, W, 200 + 2 * n + b) for b in range(2)]
        x = torch.from_numpy(np.stack([p[0] for p in pairs]))
        y = torch.from_numpy(np.stack([p[1] for p in pairs]))
        with torch.no_grad():
            r64 = R.lpips_terms(x, y, net, w, torch.float64)
            r32 = R.lpips_terms(x, y, net, w, torch.float32)
        out[(net, H, W)] = SimpleNamespace(x=x, y=y, r64=r64, r32=r32)
    bar, worst = R.pooled_bar([(c.r32, c.r64) for c in out.values()], MARGIN)
    return SimpleNamespace(cases=out, bar=bar, worst=worst)


@pytest.mark.parametrize("net,H,W", FULL_CASES)
def test_lpips_against_float64(models, full_ref, net, H, W):
    c, m = full_ref.cases[(net, H, W)], models[net].m
    x, y = c.x.to(DEV), c.y.to(DEV)
    r = m(x, y)
    t = r.table.cpu()
    assert t.shape == (2, 8) and t.dtype == torch.float64 and r.names[0] == "LPIPS"
    rel = ((t[:, :6] - c.r64).abs() / c.r64.abs())
    print(f"lpips {net} {H}x{W}: gpu rel distance LPIPS {float(rel[:, 0].max()):.3e} terms {[f'{float(v):.2e}' for v in rel[:, 1:].max(0).values]}"
          f"  cpu float32 pooled {full_ref.worst:.3e}  bar {full_ref.bar:.3e}")
    assert bool((c.r64[:, 1:] > 1e-5).all())                     # all five layers contribute
    assert float(rel.max()) <= full_ref.bar, (rel, full_ref.bar)
    assert torch.equal(t[:, 6:], torch.zeros(2, 2, dtype=torch.float64))
    # LPIPS is the sum of the five terms, in double
    assert torch.equal(t[:, 0], ((((t[:, 1] + t[:, 2]) + t[:, 3]) + t[:, 4]) + t[:, 5]))
    # two calls are bit-identical; a batched row is the single call's row; [3,H,W] is accepted
    assert torch.equal(m(x, y).table.cpu(), t)
    for b in range(2):
        assert torch.equal(m(x[b], y[b]).table.cpu()[0], t[b])
    # an identical pair: exactly 0.0
    assert torch.equal(m(x, x).table.cpu(), torch.zeros(2, 8, dtype=torch.float64))
    # invalid_flag: a NaN row, the other row untouched; out= rows of a caller's table
    big = torch.full((4, 8), -1.0, dtype=torch.float64, device=DEV)
    m(x, y, out=big[1:3], invalid_flag=torch.tensor([0, 3], dtype=torch.int32, device=DEV))
    big = big.cpu()
    assert torch.equal(big[1], t[0]) and bool(torch.isnan(big[2]).all()) and bool((big[0] == -1).all()) and bool((big[3] == -1).all())
    # quantize8=True == a pre-quantised first image
    g = torch.Generator().manual_seed(5)
    xf = (c.x + 0.3 / 255.0 * torch.randn(c.x.shape, generator=g) + 0.02).to(DEV)       # (off the 8-bit grid, some values beyond 1)
    xq = torch.floor(xf * 255.0 + 0.5).clamp(0.0, 255.0) / torch.tensor(255.0, device=DEV)      # (a tensor divisor: a true division)
    assert not torch.equal(xq, xf)
    tq = m(xf, y, quantize8=True).table.cpu()
    assert torch.equal(tq, m(xq, y).table.cpu()) and not torch.equal(tq, m(xf, y).table.cpu())


def test_sizes_below_the_minimum_fail_before_any_launch(models):
    x = torch.zeros(1, 3, 30, 50, device=DEV)
    with pytest.raises(_lib.GpHipError, match="H=30 W=50"):
        models["alex"].m(x, x)
    x = torch.zeros(1, 3, 40, 15, device=DEV)
    with pytest.raises(_lib.GpHipError, match="H=40 W=15"):
        models["vgg"].m(x, x)
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        models["vgg"].m(x.cpu(), x.cpu())


def _save_weights(d):
    for net in ("alex", "vgg"):
        w = R.seeded_weights(net)
        torch.save({f"features.{k}": v for k, v in w["backbone"].items()}, os.path.join(d, L.BACKBONE_FILES[net]))
        torch.save({f"lin{k}.model.1.weight": w["lin"][f"{k}.1.weight"] for k in range(5)}, os.path.join(d, L.LIN_FILES[net]))


def test_evaluate_dirs_with_lpips_writes_the_reference_keys(models, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from gaussianprediction_amd import metrics as M
    wdir = tmp_path / "weights"
    wdir.mkdir()
    _save_weights(str(wdir))
    root = tmp_path / "run"
    (root / "ours" / "renders").mkdir(parents=True)
    (root / "ours" / "gt").mkdir()
    names, pairs = [], []
    for i in range(3):
        r, g = R.image_pair(163, 178, 300 + i)
        r8, g8 = (torch.from_numpy(r) * 255).round().to(torch.uint8), (torch.from_numpy(g) * 255).round().to(torch.uint8)
        name = f"{i:05d}.png"
        Image.fromarray(r8.permute(1, 2, 0).numpy()).save(root / "ours" / "renders" / name)
        Image.fromarray(g8.permute(1, 2, 0).numpy()).save(root / "ours" / "gt" / name)
        names.append(name)
        pairs.append(((r8.float() / 255.0).to(DEV), (g8.float() / 255.0).to(DEV)))
    got = M.evaluate_dirs(str(root), lpips_weights=str(wdir))
    res, per = json.load(open(root / "results.json")), json.load(open(root / "per_view.json"))
    order = ["SSIM", "PSNR", "LPIPS-vgg", "LPIPS-alex", "MS-SSIM", "D-SSIM"]         # [REF metrics.py:157-162]
    assert list(res) == list(per) == list(got["ours"]["summary"]) == order
    for net in ("vgg", "alex"):
        want = torch.cat([models[net].m(r, g).table[:, 0] for r, g in pairs]).cpu()
        assert 0.005 < float(want.min())
        assert res[f"LPIPS-{net}"] == float(want.mean()) == got["ours"]["summary"][f"LPIPS-{net}"]
        assert per[f"LPIPS-{net}"] == {n: float(want[i]) for i, n in enumerate(names)}
    base = torch.cat([M.image_metrics(r, g).table for r, g in pairs]).cpu()
    assert res["SSIM"] == float(base[:, M.SSIM].mean()) and res["D-SSIM"] == float(base[:, M.D_SSIM].mean())
    # a dict names the nets; the reference's call shape finds the same files
    only = M.evaluate_dirs(str(root), write=False, lpips_weights={"alex": str(wdir)})
    assert list(only["ours"]["summary"]) == ["SSIM", "PSNR", "LPIPS-alex", "MS-SSIM", "D-SSIM"]
    assert only["ours"]["summary"]["LPIPS-alex"] == res["LPIPS-alex"]
    assert float(M.lpips(pairs[0][0], pairs[0][1], net_type="vgg", weights=str(wdir))) == per["LPIPS-vgg"][names[0]]
    # the defaults still write the four keys only
    M.evaluate_dirs(str(root))
    assert list(json.load(open(root / "results.json"))) == ["SSIM", "PSNR", "MS-SSIM", "D-SSIM"]


def test_evaluate_views_with_lpips_equals_per_view_calls(models):
    from test_gpu_render import build
    import gaussianprediction_amd as gpa
    from gaussianprediction_amd import metrics as M
    from gaussianprediction_amd.cameras import orbit_cameras
    from gaussianprediction_amd.renderer import SpeculativeRenderer
    pc = build(N=3000, K=60, W=178, H=163)[0]
    cams = orbit_cameras(5, 4.0, 0.6911, 178, 163, device=DEV)[:4]
    times = [torch.tensor([0.1 + 0.2 * v], device=DEV) for v in range(len(cams))]
    gts = [torch.from_numpy(R.image_pair(163, 178, 400 + v % 2)[1]).to(DEV) for v in range(len(cams))]
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    bg = torch.zeros(3, device=DEV)
    nets = [models["vgg"].m, models["alex"].m]
    with torch.no_grad():
        imgs = [gpa.render(cams[v], pc, pipe, bg, time=times[v], it=50000)["render"] for v in range(len(cams))]
        want = {m.net_type: torch.cat([m(imgs[v], gts[v], quantize8=True).table for v in range(len(cams))]).cpu() for m in nets}
        base = torch.cat([M.image_metrics(imgs[v], gts[v], quantize8=True).table for v in range(len(cams))]).cpu()
    assert not any(bool(torch.isnan(t).any()) for t in want.values())
    plain = M.evaluate_views(pc, cams, gts, pipe, bg, 50000, times=times)
    assert set(plain["summary"]) == {"SSIM", "PSNR", "MS-SSIM", "D-SSIM", "L1"} and "per_view_lpips" not in plain
    for kw in (dict(speculative=False), dict()):
        got = M.evaluate_views(pc, cams, gts, pipe, bg, 50000, times=times, lpips=nets, **kw)
        assert torch.equal(got["per_view"].cpu(), base)
        for net, t in want.items():
            assert torch.equal(got["per_view_lpips"][net].cpu(), t)
            assert got["summary"][f"LPIPS-{net}"] == float(t[:, 0].mean())
    # after an overflow the NaN rows are redone for LPIPS too
    sr = SpeculativeRenderer(pc, pipe, bg)
    with torch.no_grad():
        sr(cams[0], time=times[0], it=50000)
    sr.capacity = 1024
    tight = M.evaluate_views(pc, cams, gts, pipe, bg, 50000, times=times, renderer=sr, lpips=nets)
    assert tight["rerendered"] > 0
    for net, t in want.items():
        assert torch.equal(tight["per_view_lpips"][net].cpu(), t)
