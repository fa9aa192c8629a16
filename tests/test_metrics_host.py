"""No GPU: the float64 restatement of the image metrics (tests/metrics_ref.py) against the reference's own numbers
(tests/golden/metrics.npz, recorded by tests/golden/make_metrics_vectors.py), the pytorch_msssim import shim's surface, the CPU
refusal of gaussianprediction_amd.metrics, and the new kernels' load batching."""
import importlib
import inspect
import os
import shutil
import sys

import numpy as np
import pytest
import torch

import metrics_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = np.load(os.path.join(HERE, "golden", "metrics.npz"))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.parametrize("k", range(len(R.GOLDEN_SIZES)))
def test_restatement_matches_the_reference_functions(k):
    img, gt = R.golden_pair(k)
    tag = f"p{k}_"
    assert tuple(GOLD[tag + "size"]) == img.shape[1:]
    # the seeded images are the ones the vectors were recorded on
    assert img.sum(dtype=np.float64) == float(GOLD[tag + "render_sum"]) and gt.sum(dtype=np.float64) == float(GOLD[tag + "gt_sum"])
    a, b = torch.from_numpy(img).double()[None], torch.from_numpy(gt).double()[None]
    m = R.all_metrics(a, b, with_ms=False)
    # 2e-6: the bar test_gpu_loss_adam.py holds the same reference functions to (they run in float32)
    assert abs(float(m["L1"]) - float(GOLD[tag + "l1"])) < 2e-6
    assert abs(float(m["SSIM"]) - float(GOLD[tag + "ssim"])) < 2e-6
    # both call shapes of psnr(): [1,3,H,W] -> one number over all channels; [3,H,W] -> one per channel, then .mean()
    assert abs(float(m["PSNR"]) - float(GOLD[tag + "psnr_13hw"])) < 2e-5
    assert abs(float(m["PSNR_CH"]) - float(GOLD[tag + "psnr_3hw"].mean())) < 2e-5
    per_ch = 20 * torch.log10(1.0 / torch.sqrt(((a - b) ** 2).flatten(2).mean(2)))[0]
    assert np.abs(per_ch.numpy() - GOLD[tag + "psnr_3hw"]).max() < 2e-5
    assert abs(float(m["PSNR"]) - float(m["PSNR_CH"])) > 1e-7       # the two conventions are different numbers


def test_restatement_ms_ssim_properties():
    render, gt = R.probe_pair()
    lv = R.ms_ssim_levels(render.double(), gt.double())
    assert lv.shape == (2, 5, 3) and float(lv.min()) > 0.6          # no ReLU active on the probe pair
    v = R.ms_ssim(render.double(), gt.double())
    assert 0.95 < float(v.min()) and float(v.max()) < 1.0
    assert torch.allclose(R.ms_ssim(gt.double(), gt.double()), torch.ones(2, dtype=torch.float64), atol=1e-12)
    # the inverted image: every term negative, the ReLU makes the value exactly zero in both precisions
    for dt in (torch.float32, torch.float64):
        inv = (1 - gt).to(dt)
        assert float(R.ms_ssim_levels(inv, gt.to(dt)).max()) < 0
        assert torch.equal(R.ms_ssim(inv, gt.to(dt)), torch.zeros(2, dtype=dt))
    with pytest.raises(AssertionError):
        R.ms_ssim_levels(torch.zeros(1, 3, 160, 200), torch.zeros(1, 3, 160, 200))


def test_shim_resolves_here_and_states_unpinned_parity():
    m = importlib.import_module("pytorch_msssim")
    assert os.path.realpath(m.__file__).startswith(os.path.realpath(ROOT) + os.sep), m.__file__
    assert "unpinned" in (m.__doc__ or "")
    top = [l for l in inspect.getsource(m).splitlines() if l.startswith(("import ", "from "))]
    assert not any("gaussianprediction_amd" in l for l in top), top      # the library loads at the first call, not at import


def test_shim_signature_is_the_published_one():
    from pytorch_msssim import ms_ssim
    sig = inspect.signature(ms_ssim)
    assert list(sig.parameters) == ["X", "Y", "data_range", "size_average", "win_size", "win_sigma", "win", "weights", "K"]
    d = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert d == {"data_range": 255, "size_average": True, "win_size": 11, "win_sigma": 1.5, "win": None, "weights": None, "K": (0.01, 0.03)}
    sig.bind(None, None, data_range=1, size_average=True)           # the reference's call [REF metrics.py:143]


@pytest.mark.parametrize("key,value", [("win_size", 7), ("win_sigma", 1.0), ("win", torch.ones(11)), ("weights", [0.2] * 5), ("K", (0.01, 0.04))])
def test_shim_refuses_other_arguments(key, value):
    from pytorch_msssim import ms_ssim
    x = torch.zeros(1, 3, 170, 170)
    with pytest.raises(ValueError, match=repr(key)):
        ms_ssim(x, x, data_range=1, **{key: value})


def test_cpu_tensors_raise():
    from gaussianprediction_amd import metrics
    x = torch.zeros(1, 3, 170, 170)
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        metrics.image_metrics(x, x)
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        metrics.psnr(x[0], x[0])
    from pytorch_msssim import ms_ssim
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        ms_ssim(x, x, data_range=1)


def test_metrics_module_does_not_import_the_restatement():
    src = open(os.path.join(ROOT, "gaussianprediction_amd", "metrics.py")).read() + open(os.path.join(ROOT, "pytorch_msssim", "__init__.py")).read()
    assert "metrics_ref" not in src and "oracle" not in src


def test_abi_and_column_constants_agree_with_the_header():
    import re
    from gaussianprediction_amd import _lib, metrics
    hdr = open(os.path.join(ROOT, "include", "gp_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_METRICS?_[A-Z0-9_]+) (\d+)u?\b", hdr)}
    assert _lib.GP_ABI_VERSION == 9 and int(re.search(r"#define GP_ABI_VERSION (\d+)", hdr).group(1)) == 9
    for name in ("L1", "MSE", "PSNR", "PSNR_CH", "SSIM", "MS_SSIM", "D_SSIM"):
        assert defs["GP_METRIC_" + name] == getattr(metrics, name) == metrics.NAMES.index(name)
    assert defs["GP_METRIC_COUNT"] == metrics.METRIC_COUNT == len(metrics.NAMES) == 8
    assert (defs["GP_METRICS_QUANTIZE8"], defs["GP_METRICS_CLAMP01"], defs["GP_METRICS_MS_SSIM"]) == (metrics.QUANTIZE8, metrics.CLAMP01, metrics.WITH_MS_SSIM) == (1, 2, 4)
    assert {"gp_image_metrics", "gp_image_metrics_scratch_bytes"} <= set(_lib.EXPORTS)


def test_scratch_size_and_shape_refusal_need_no_gpu():
    import ctypes as C
    from gaussianprediction_amd import _lib
    l = _lib.lib()
    q = lambda B, H, W, f: int(l.gp_image_metrics_scratch_bytes(C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_uint32(f)))   # noqa: E731
    # without MS-SSIM: the level-0 slots only (5 doubles per 32 x 32 tile and plane)
    assert q(1, 37, 45, 0) == 512                            # (3 planes x 4 tiles x 5 doubles = 480 bytes, rounded up to 256)
    n1, n8 = q(1, 163, 178, 4), q(8, 163, 178, 4)
    pyramid = sum(2 * 3 * h * w * 4 for h, w in ((82, 89), (41, 45), (21, 23), (11, 12)))
    assert pyramid < n1 < pyramid + 16 * 1024 and 7 * n1 < n8 <= 8 * n1
    assert q(1, 160, 200, 4) == -1 and b"160" in l.gp_last_error() and b"200" in l.gp_last_error()
    assert q(1, 160, 200, 0) > 0
    assert q(1, 200, 160, 4) == -1 and b"H=200 W=160" in l.gp_last_error()
    assert q(0, 37, 45, 0) == -1 and q(1, 37, 45, 8) == -1
    # sizes beyond what one launch can cover: a message, not a launch error
    assert q(21846, 37, 45, 0) == -1 and b"21845" in l.gp_last_error()
    assert q(1, 32 * 65535 + 1, 45, 0) == -1 and b"2097120" in l.gp_last_error()
    assert q(1, 45, 2**31 - 1, 0) == -1 and b"2097120" in l.gp_last_error()
    assert q(1, 32 * 65535, 32, 0) > 0


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_metric_kernels_keep_their_loads_batched():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from isa_load_audit import CSRC, audit
    stats = audit(os.path.join(CSRC, "metric_kernels.hip"), HIPCC)
    for want in ("gp_metric_level_kernelILb1E", "gp_metric_level_kernelILb0E", "gp_metric_finalize_kernel"):
        hits = [(k, v) for k, v in stats.items() if want in k]
        assert hits, f"{want} not found"
        for k, (loads, waits, tight) in hits:
            assert loads >= 2 and tight <= 2, f"{k}: {tight} of {waits} full waits sit right behind one of its {loads} loads (serialized loads?)"
