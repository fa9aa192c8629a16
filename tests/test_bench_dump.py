"""bench.py --dump-outputs (no GPU): dump_outputs() writes what the timed path handed back -- the loss and the render()-shaped dict -- as
float32 / float64 .npy files, per-Gaussian arrays as the same seeded sample of rows in every run, within the size budget."""
import numpy as np
import torch

import bench


def _step_output(n, h=6, w=10, seed=0):
    g = torch.Generator().manual_seed(seed)
    vs = torch.zeros(n, 3, requires_grad=True)
    vs.grad = torch.randn(n, 3, generator=g)
    pkg = {"render": torch.rand(3, h, w, generator=g), "viewspace_points": vs, "visibility_filter": torch.rand(n, generator=g) > 0.5,
           "radii": torch.randint(0, 9, (n,), generator=g, dtype=torch.int32), "depth": torch.rand(1, h, w, generator=g),
           "tidx": torch.randint(0, 1 << 20, (h, w), generator=g, dtype=torch.int32)}
    return torch.tensor(0.25), pkg


def _load(d):
    return {f.name[:-4]: np.load(f) for f in d.iterdir()}


def test_train_step_outputs_are_written_as_floats_with_a_fixed_row_sample(tmp_path):
    n = bench.DUMP_ROWS + 1000
    out = _step_output(n)
    bench.dump_outputs(str(tmp_path / "a"), out, train=True)
    a = _load(tmp_path / "a")
    assert set(a) == {"loss", "render", "viewspace_points_grad", "visibility_filter", "radii", "depth", "tidx"}
    assert all(v.dtype == (np.float64 if k in ("visibility_filter", "radii", "tidx") else np.float32) for k, v in a.items())
    assert a["loss"].shape == () and float(a["loss"]) == 0.25
    np.testing.assert_array_equal(a["render"], out[1]["render"].numpy())                       # image-sized arrays: whole
    np.testing.assert_array_equal(a["tidx"], out[1]["tidx"].numpy().astype(np.float64))
    rows = np.sort(np.random.default_rng(0).choice(n, bench.DUMP_ROWS, replace=False))          # per-Gaussian arrays: the seeded rows
    np.testing.assert_array_equal(a["viewspace_points_grad"], out[1]["viewspace_points"].grad.numpy()[rows])
    np.testing.assert_array_equal(a["radii"], out[1]["radii"].numpy()[rows].astype(np.float64))
    bench.dump_outputs(str(tmp_path / "b"), _step_output(n), train=True)                        # same inputs, same files
    b = _load(tmp_path / "b")
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


def test_render_only_outputs_and_small_scenes_are_written_whole(tmp_path):
    _, pkg = _step_output(100)
    bench.dump_outputs(str(tmp_path), pkg, train=False)
    a = _load(tmp_path)
    assert "loss" not in a
    np.testing.assert_array_equal(a["viewspace_points_grad"], pkg["viewspace_points"].grad.numpy())


def test_files_stay_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 20_000)
    out = _step_output(500, h=40, w=50)                              # render alone: 24 000 bytes
    bench.dump_outputs(str(tmp_path), out, train=True)
    a = _load(tmp_path)
    assert sum(v.nbytes for v in a.values()) <= 20_000
    assert a["render"].size < 3 * 40 * 50 and set(np.unique(a["render"])) <= set(np.unique(out[1]["render"].numpy()))
