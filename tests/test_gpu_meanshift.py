"""On the device: meanshift_ops against the numpy restatement tests/meanshift_ref.py BIT FOR BIT on every blob, line and edge case
(both sides perform the same correctly rounded operations in the same order: anything else is a defect in one of them), against
sklearn's recorded output at the bars of tests/test_meanshift_host.py, the independence of a seed's result from the launch shape, an
estimate feeding a run without a host read, and the surface: cluster, label_colors, render_segments, the refusals on device tensors."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import meanshift_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
REF_TO_FIXTURE = 3e-5              # as tests/test_meanshift_host.py: 3 x the 8.58e-6 measured when the fixture was recorded
BANDWIDTH_REL = 1e-6


def same(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else b
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(name):
    from gaussianprediction_amd import meanshift_ops as M
    X, seeds, bw, max_iter, cluster_all = ref.cases()[name]
    return M.mean_shift(dev(X), None if bw is None else float(bw), dev(seeds), max_iter, cluster_all)


def equal_to_the_restatement(got, want):
    assert float(got.bandwidth) == want["bandwidth"] and got.bandwidth.dtype == torch.float64 and got.bandwidth.dim() == 0
    assert same(got.seed_centers, want["seed_centers"])
    assert same(got.seed_counts, want["seed_counts"]) and same(got.seed_iterations, want["seed_iterations"])
    assert same(got.cluster_centers, want["cluster_centers"])                                  # the kept centres, in order
    assert same(got.counts, want["counts"].astype(np.int64)) and got.n_iter == want["n_iter"]
    assert got.labels.dtype == torch.int64 and same(got.labels, want["labels"])


@pytest.mark.parametrize("name", list(ref.cases()))
def test_every_case_equals_the_restatement_bit_for_bit_and_from_run_to_run(name):
    got, again = run(name), run(name)
    equal_to_the_restatement(got, ref.run_case(name))
    for field in ("labels", "cluster_centers", "counts", "bandwidth", "seed_centers", "seed_counts", "seed_iterations"):
        assert same(getattr(got, field), getattr(again, field)), field
    assert got.n_iter == again.n_iter


@pytest.mark.parametrize("name", ref.FIXTURE_RUNS)
def test_fixture_cases_against_sklearns_recorded_output(name):
    g = np.load(ref.GOLDEN)
    got = run(name)
    centres = g[f"centers_{name}"]
    assert tuple(got.cluster_centers.shape) == centres.shape                                  # K
    assert np.array_equal(got.labels.cpu().numpy(), g[f"labels_{name}"])                       # every label
    assert got.n_iter == int(g[f"n_iter_{name}"])
    assert np.abs(got.cluster_centers.cpu().numpy().astype(np.float64) - centres).max() <= REF_TO_FIXTURE
    assert abs(float(got.bandwidth) / float(g[f"bandwidth_{name}"]) - 1) <= BANDWIDTH_REL


@pytest.mark.parametrize("quantile,n_samples", [(0.3, None), (0.1, 300), (0.5, 64), (1.0, None)])
def test_estimate_bandwidth_equals_the_restatement(quantile, n_samples):
    from gaussianprediction_amd import meanshift_ops as M
    X = ref.cases()["blobs_1031_8_est"][0]
    sub = X if n_samples is None else ref.subsample(X, n_samples)
    bw, kth = M.estimate_bandwidth(dev(X), quantile, n_samples, return_kth=True)
    assert same(kth, ref.kth_distances(sub, quantile))                                         # np.partition, exactly
    assert bw.dtype == torch.float64 and bw.dim() == 0 and float(bw) == ref.estimate_bandwidth(sub, quantile)
    assert same(M.estimate_bandwidth(dev(X), quantile, n_samples), bw)


def test_a_quantile_that_clamps_k_to_one_gives_bandwidth_zero_which_mean_shift_refuses():
    from gaussianprediction_amd import _lib, meanshift_ops as M
    x = dev(ref.cases()["blobs_1031_8_est"][0])
    bw = M.estimate_bandwidth(x, 0.0005)
    assert float(bw) == 0.0
    with pytest.raises(_lib.GpHipError, match="bandwidth must be finite and > 0"):
        M.mean_shift(x, bw)                                                                    # (read on the device: the status block says so)
    with pytest.raises(_lib.GpHipError, match="bandwidth must be finite and > 0"):
        M.mean_shift(x, torch.tensor(float("nan"), dtype=torch.float64, device=DEV))


def test_a_seeds_result_does_not_depend_on_the_launch_shape():
    from gaussianprediction_amd import meanshift_ops as M
    X, seeds, bw, _, _ = ref.cases()["subset_2053_32"]
    alone, inside = M.mean_shift(dev(X), bw, dev(seeds)), M.mean_shift(dev(X), bw)
    assert same(alone.seed_centers, inside.seed_centers[::41]) and same(alone.seed_counts, inside.seed_counts[::41])
    assert same(alone.seed_iterations, inside.seed_iterations[::41])
    X3 = ref.cases()["lines1_1031_3_300"][0]                                                  # dozens of steps: a seed alone, a wave of them, all
    whole = M.mean_shift(dev(X3), 1.0)
    for pick in (slice(5, 6), slice(0, 1031, 13), slice(100, 400)):
        part = M.mean_shift(dev(X3), 1.0, dev(X3[pick]))
        assert same(part.seed_centers, whole.seed_centers[pick]) and same(part.seed_counts, whole.seed_counts[pick])
        assert same(part.seed_iterations, whole.seed_iterations[pick])


@pytest.mark.parametrize("N,S", [(257, 1), (1, 33), (1, 1)])
def test_one_seed_one_row(N, S):
    from gaussianprediction_amd import meanshift_ops as M
    X = ref.cases()["blobs_257_3_est"][0][:N]
    seeds = (ref.cases()["blobs_257_3_est"][0][:S] + (np.float32(0.25) if N == 1 else np.float32(0))).astype(np.float32)
    got = M.mean_shift(dev(X), 2.0, dev(seeds))
    equal_to_the_restatement(got, ref.mean_shift(X, 2.0, seeds))


def test_an_estimate_feeds_a_run_without_a_host_read():
    from gaussianprediction_amd import meanshift_ops as M
    x = dev(ref.cases()["blobs_257_3_est"][0])
    bw = M.estimate_bandwidth(x)
    fed, given, default = M.mean_shift(x, bw), M.mean_shift(x, float(bw)), M.mean_shift(x)
    assert fed.bandwidth is not None and fed.bandwidth.data_ptr() == bw.data_ptr()              # the estimate itself, not a copy through the host
    for other in (given, default):
        for field in ("labels", "cluster_centers", "counts", "bandwidth", "seed_centers", "seed_counts", "seed_iterations"):
            assert same(getattr(fed, field), getattr(other, field)), field


def test_cluster_and_label_colors():
    from gaussianprediction_amd import feature_vis as F, kmeans_ops, meanshift_ops as M
    x = dev(ref.cases()["blobs_257_3_est"][0])
    labels = F.cluster(x, "MeanShift")
    assert labels.dtype == torch.int64 and same(labels, M.mean_shift(x).labels) and same(F.cluster(x, "anything else"), labels)
    assert same(F.cluster(x, "KMeans", 4), kmeans_ops.kmeans(x, 4).ids) and same(F.cluster(x), kmeans_ops.kmeans(x, 4).ids)
    orphans = torch.tensor([2, 0, -1, 2, 1, -1, 0], device=DEV)
    colors = F.label_colors(orphans)
    assert colors.dtype == torch.float32 and tuple(colors.shape) == (7, 3)
    assert same(colors[0], colors[3]) and same(colors[1], colors[6]) and not same(colors[0], colors[1]) and not same(colors[1], colors[4])
    assert colors[2].tolist() == [0.5, 0.5, 0.5] == colors[5].tolist()
    assert same(colors[[1, 4, 0]], F.label_palette(3)) and not same(F.label_colors(orphans, seed=1), colors)


def test_render_segments_writes_its_directory_and_a_segment_carries_its_labels_colour(tmp_path):
    from PIL import Image
    import gaussianprediction_amd as gpa
    import png_cases as P
    from gaussianprediction_amd import eval_render as ER, feature_vis as F, meanshift_ops as M
    from gaussianprediction_amd.cameras import orbit_cameras
    from test_gpu_render import build
    W, H, IT = 64, 48, 50000
    pc = build(N=3000, K=60, W=W, H=H)[0]
    views = orbit_cameras(2, 4.0, 0.6911, W, H, device=DEV)
    pipe, bg = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False), torch.zeros(3, device=DEV)
    root = str(tmp_path / "model")
    out_path, result = ER.render_segments(root, "test", IT, views, pc, pipe, bg)
    assert out_path == os.path.join(root, "eval", "test", f"ours_{IT}", "segments") and isinstance(result, M.MeanShiftResult)
    tree = sorted(os.path.relpath(os.path.join(d, f), root) for d, _, files in os.walk(root) for f in files)
    assert tree == [os.path.join("eval", "test", f"ours_{IT}", "segments", f"{i:05d}.png") for i in range(2)]
    feats = pc.motion_feature.detach().contiguous()
    assert same(result.labels, F.cluster(feats, "MeanShift")) and len(result.labels) == 3000
    colors = F.label_colors(result.labels)
    for i, cam in enumerate(views):
        with torch.no_grad():
            want = gpa.render(cam, pc, pipe, bg, time=torch.from_numpy(cam.time).to(DEV), it=IT, override_color=colors)["render"]
        got = np.array(Image.open(os.path.join(root, tree[i])))
        assert float(want.max()) > 0.05 and got.shape == (H, W, 3) and np.array_equal(got, P.quantise(want.cpu().numpy()).transpose(1, 2, 0)), i
    # given labels, all Gaussians in one segment: every pixel is covered by that segment alone and carries its colour, times the coverage
    one = torch.full((3000,), 2, dtype=torch.int64, device=DEV)
    _, none = ER.render_segments(root, "test", IT, views[:1], pc, pipe, bg, labels=one)
    assert none is None
    got = np.array(Image.open(os.path.join(root, tree[0]))).astype(np.float64) / 255.0
    c = F.label_palette(3)[2].astype(np.float64)
    coverage = got.max(axis=-1) / c.max()
    lit = coverage > 0.25
    assert lit.sum() > 50 and np.abs(got[lit] - coverage[lit][:, None] * c[None, :]).max() <= 1.0 / 255.0 + 1e-9


def test_what_the_module_refuses_on_device_tensors():
    from gaussianprediction_amd import _lib, meanshift_ops as M
    far = torch.arange(4200, dtype=torch.float32, device=DEV)[:, None].contiguous()            # 4200 points a unit apart, each its own centre
    with pytest.raises(_lib.GpHipError, match="more than 4096 centres were kept"):
        M.mean_shift(far, 0.1)
    kept = M.mean_shift(far[:4096].contiguous(), 0.1)                                          # exactly 4096 are fine
    assert tuple(kept.cluster_centers.shape) == (4096, 1) and kept.n_iter == 0 and same(kept.labels, 4095 - torch.arange(4096, device=DEV))     # equal counts: the larger centre first
    X, _ = ref.edge_1d()
    with pytest.raises(ValueError, match="No point was within bandwidth=0.800000 of any seed"):
        M.mean_shift(dev(X), 0.8, torch.tensor([[100.0]], device=DEV))
    x = dev(X)
    with pytest.raises(RuntimeError, match="must be float32"):
        M.mean_shift(x.double(), 0.8)
    with pytest.raises(RuntimeError, match="must be contiguous"):
        M.mean_shift(torch.zeros(4, 10, device=DEV).t(), 0.8)
    with pytest.raises(_lib.GpHipError, match="D must be in 1 .. 64"):
        M.mean_shift(torch.zeros(10, 65, device=DEV), 0.8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.mean_shift(x, 0.8, seeds=torch.from_numpy(X))
    with pytest.raises(RuntimeError, match="must hold one float64"):
        M.mean_shift(x, torch.tensor(0.8, device=DEV))
