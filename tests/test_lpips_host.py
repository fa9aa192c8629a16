"""No GPU: the float64 restatement of LPIPS (tests/lpips_ref.py) against what the reference's own classes return on the seeded
recipe (tests/golden/lpips.npz, recorded by tests/golden/make_lpips_vectors.py); the library's network tables against the
reference's lists; include/gp_lpips.h against the binding's table; the refusals, the weight loader and the weight-file search."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import abi_check
import lpips_ref as R
from gaussianprediction_amd import _lib, lpips as L

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = np.load(os.path.join(HERE, "golden", "lpips.npz"))
NETS = ("alex", "vgg")


@pytest.mark.parametrize("net", NETS)
def test_restatement_matches_the_reference_classes(net):
    w = R.seeded_weights(net)
    assert R.weights_checksum(w) == float(GOLD[f"{net}_weights_sum"])          # the seeded weights the vectors were recorded on
    for k, (H, W) in enumerate(R.SIZES):
        tag = f"{net}_c{k}_"
        render, gt = R.case_pair(k)
        assert tuple(GOLD[tag + "size"]) == (H, W) == render.shape[1:]
        assert render.sum(dtype=np.float64) == float(GOLD[tag + "render_sum"]) and gt.sum(dtype=np.float64) == float(GOLD[tag + "gt_sum"])
        with torch.no_grad():
            t = R.lpips_terms(torch.from_numpy(render)[None], torch.from_numpy(gt)[None], net, w, torch.float64)[0].numpy()
        want = np.concatenate([[float(GOLD[tag + "lpips"])], GOLD[tag + "terms"]])
        # 1e-10 relative: double rounding (1.1e-16) x K <= 4608 x 13 layers is far below it
        assert np.abs(t - want).max() <= 1e-10 * np.abs(want).min(), (tag, t, want)
        assert (want[1:] > 1e-4).all() and 0.01 < want[0] < 0.1                # all five layers contribute


@pytest.mark.parametrize("net", NETS)
def test_library_tables_equal_the_reference_lists(net):
    assert L.target_layers(net) == GOLD[f"{net}_target_layers"].tolist() == R.TARGET_LAYERS[net]
    assert L.n_channels_list(net) == GOLD[f"{net}_n_channels_list"].tolist() == R.N_CHANNELS[net]
    # the z-score constants are the float32 values of the reference's buffers
    assert GOLD[f"{net}_mean"].tolist() == [float(np.float32(v)) for v in R.MEAN]
    assert GOLD[f"{net}_std"].tolist() == [float(np.float32(v)) for v in R.STD]
    # the whole table is torchvision's `features`, entry by entry
    table = L.network_table(net)
    assert len(table) == len(R.FEATURES[net])
    convs = 0
    for e, want in zip(table, R.FEATURES[net]):
        if want[0] == "conv":
            assert (e.kind, e.cin, e.cout, e.k, e.stride, e.pad, e.conv) == (L.CONV,) + want[1:] + (convs,)
            convs += 1
        elif want[0] == "relu":
            assert e.kind == L.RELU and e.conv == -1
        else:
            assert (e.kind, e.k, e.stride, e.pad) == (L.POOL, want[1], want[2], 0) and not e.tap
    with pytest.raises(NotImplementedError, match="squeeze"):
        L.network_table("squeeze")


# ---- one signature per entry point, two statements of it: include/gp_lpips.h and lpips.PROTOTYPES ----
_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "float": C.c_float, "gp_stream_t": _lib.Ptr}
_POINTEES = {"float", "double", "void", "int32_t", "uint32_t"}


def test_prototype_table_equals_the_header():
    abi_check.check_table(L.ABI, 9, _SCALARS, _POINTEES)
    assert L.ABI.prototypes is L.PROTOTYPES and L.ABI.header == "gp_lpips.h"


def test_symbols_are_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gp_lpips.h")).read()
    assert int(re.search(r"#define GP_LPIPS_ABI_VERSION (\d+)", hdr).group(1)) == L.GP_LPIPS_ABI_VERSION == L.ABI.version == 1
    abi_check.check_applied(L.ABI)
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_LPIPS_[A-Z0-9_]+) (\d+)u?\b", hdr)}
    assert (defs["GP_LPIPS_ALEX"], defs["GP_LPIPS_VGG"], defs["GP_LPIPS_SQUEEZE"]) == (L.NETS["alex"], L.NETS["vgg"], L.NETS["squeeze"])
    assert (defs["GP_LPIPS_QUANTIZE8"], defs["GP_LPIPS_TAPS"], defs["GP_LPIPS_COLUMNS"]) == (L.QUANTIZE8, L.TAPS, L.COLUMNS)
    assert (defs["GP_LPIPS_CONV"], defs["GP_LPIPS_RELU"], defs["GP_LPIPS_POOL"]) == (L.CONV, L.RELU, L.POOL)


def test_scratch_size_and_refusals_need_no_gpu():
    l = L.lib()
    q = lambda net, B, H, W: int(l.gp_lpips_scratch_bytes(net, B, H, W))       # noqa: E731
    assert q(0, 1, 30, 50) == -1 and b"H=30 W=50" in l.gp_last_error()
    assert q(0, 1, 50, 30) == -1 and b"H=50 W=30" in l.gp_last_error()
    assert q(0, 1, 31, 50) > 0
    assert q(1, 1, 15, 40) == -1 and b"H=15 W=40" in l.gp_last_error()
    assert q(1, 1, 16, 40) > 0
    assert q(1, 0, 64, 64) == -1 and b"B=0" in l.gp_last_error()
    assert q(7, 1, 64, 64) == -1 and b"unknown net" in l.gp_last_error()
    assert q(2, 1, 64, 64) == -1 and b"squeeze" in l.gp_last_error()
    # the working set is that of ONE pair: two buffers of the largest activation (vgg: 2 x H x W x 64 floats) plus the slots
    one = q(1, 1, 163, 178)
    assert one == q(1, 8, 163, 178)
    act = 2 * 163 * 178 * 64 * 4
    assert 2 * act <= one < 2 * act + 128 * 1024
    assert int(l.gp_lpips_weight_floats(7)) == -1
    n_alex = sum(e[2] * e[1] * e[3] ** 2 + e[2] for e in R.FEATURES["alex"] if e[0] == "conv") + sum(R.N_CHANNELS["alex"])
    assert n_alex <= int(l.gp_lpips_weight_floats(0)) < n_alex + 64 * 15
    # the gp_lpips call itself refuses the same sizes before any launch (no GPU here: a launch would fail differently)
    rc = l.gp_lpips(0, 256, 256, 256, 1, 30, 50, 0, 256, None, 256, None)
    assert rc != 0 and b"H=30 W=50" in l.gp_last_error()


def _renamed(sd, fmt):
    return {fmt.format(k): v for k, v in sd.items()}


@pytest.mark.parametrize("net", NETS)
def test_weight_loader_key_forms_and_shape_refusal(net, tmp_path):
    w = R.seeded_weights(net)
    base = L.load_weights(net, w["backbone"], w["lin"])
    n_conv = sum(e[0] == "conv" for e in R.FEATURES[net])
    assert [len(x) for x in base] == [n_conv, n_conv, 5]
    full = _renamed(w["backbone"], "features.{}")
    full["classifier.1.weight"] = torch.zeros(4, 4)             # a whole torchvision model: other keys are ignored
    published = {f"lin{k}.model.1.weight": w["lin"][f"{k}.1.weight"] for k in range(5)}
    torch.save(full, tmp_path / "bb.pth")
    torch.save(published, tmp_path / "lin.pth")
    for bb, lin in ((full, published), (_renamed(w["backbone"], "layers.{}"), w["lin"]), (str(tmp_path / "bb.pth"), str(tmp_path / "lin.pth"))):
        got = L.load_weights(net, bb, lin)
        assert all(torch.equal(a, b) for x, y in zip(base, got) for a, b in zip(x, y))
    first = next(i for i, e in enumerate(R.FEATURES[net]) if e[0] == "conv")
    last = max(i for i, e in enumerate(R.FEATURES[net]) if e[0] == "conv")
    bad = dict(w["backbone"])
    bad[f"{last}.weight"] = bad[f"{last}.weight"][:, :-1]
    with pytest.raises(ValueError, match=rf"{last}\.weight must have shape"):
        L.load_weights(net, bad, w["lin"])
    bad = dict(full)
    bad[f"features.{first}.bias"] = torch.zeros(3)
    with pytest.raises(ValueError, match=rf"features\.{first}\.bias must have shape"):
        L.load_weights(net, bad, published)
    bad = dict(published)
    bad["lin3.model.1.weight"] = torch.zeros(1, 7, 1, 1)
    with pytest.raises(ValueError, match=r"lin3\.model\.1\.weight must have shape"):
        L.load_weights(net, full, bad)
    missing = {k: v for k, v in w["backbone"].items() if k != f"{last}.bias"}
    with pytest.raises(KeyError, match=rf"features\.{last}\.bias"):
        L.load_weights(net, missing, w["lin"])


def test_find_lpips_weights_lists_what_it_tried(tmp_path, monkeypatch):
    monkeypatch.setenv("GP_LPIPS_WEIGHTS", str(tmp_path / "env"))
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))
    with pytest.raises(FileNotFoundError) as ei:
        L.find_lpips_weights("alex", str(tmp_path))
    msg = str(ei.value)
    for name in ("alexnet-owt-7be5be79.pth", "alex.pth"):
        for d in (tmp_path, tmp_path / "env", tmp_path / "hub" / "checkpoints"):
            assert os.path.join(str(d), name) in msg
    with pytest.raises(FileNotFoundError) as ei:
        L.find_lpips_weights("vgg", str(tmp_path))
    assert "vgg16-397923af.pth" in str(ei.value) and os.path.join(str(tmp_path), "vgg.pth") in str(ei.value)
    # search order: `search` before the environment before the hub cache
    for d in (tmp_path / "env", tmp_path / "hub" / "checkpoints"):
        os.makedirs(d)
        for name in ("vgg16-397923af.pth", "vgg.pth"):
            open(d / name, "w").close()
    assert L.find_lpips_weights("vgg", str(tmp_path)) == (str(tmp_path / "env" / "vgg16-397923af.pth"), str(tmp_path / "env" / "vgg.pth"))
    open(tmp_path / "vgg.pth", "w").close()
    assert L.find_lpips_weights("vgg", str(tmp_path))[1] == str(tmp_path / "vgg.pth")
    monkeypatch.delenv("GP_LPIPS_WEIGHTS")
    assert L.find_lpips_weights("vgg")[0] == str(tmp_path / "hub" / "checkpoints" / "vgg16-397923af.pth")


def test_the_package_never_downloads():
    pkg = os.path.join(ROOT, "gaussianprediction_amd")
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            src = open(os.path.join(pkg, f)).read()
            assert "hub.load" not in src and "load_state_dict_from_url" not in src and "urlopen" not in src, f


def test_cpu_tensors_raise():
    from gaussianprediction_amd import metrics
    assert metrics.LPIPS is L.LPIPS and metrics.lpips is L.lpips and metrics.find_lpips_weights is L.find_lpips_weights
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        L.lpips(x, x)
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        L.LPIPS.__call__(L.LPIPS.__new__(L.LPIPS), x, x)
    w = R.seeded_weights("alex")
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        L.LPIPS("alex", w["backbone"], w["lin"], device="cpu")
    with pytest.raises(NotImplementedError, match="squeeze"):
        L.LPIPS("squeeze", {}, {})


def test_default_arguments_of_the_evaluation_loops_are_unchanged():
    import inspect
    from gaussianprediction_amd import metrics
    assert inspect.signature(metrics.evaluate_views).parameters["lpips"].default is None
    assert inspect.signature(metrics.evaluate_dirs).parameters["lpips_weights"].default is None
    src = open(os.path.join(ROOT, "gaussianprediction_amd", "metrics.py")).read()
    assert "not provided" not in src and "MISSING" not in src
