"""The geometry metrics on the device against the numpy restatement tests/geometry_ref.py on every case of tests/geometry_cases.py:
the samples, the nearest neighbour under every cell rule and the table bit for bit; every call twice with equal bytes; the inputs
unchanged; nearest against knn_ops.knn_points(K=1) bit for bit; the sampling, sphere and metric facts on the device's own output;
stats as the only device read; mesh_distance of a mesh and its simplification; evaluate_mesh_dirs and mesh_motion on small folders.

Measured on an MI355X: see DESIGN section 30."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import geometry_cases as cases
import geometry_ref as ref
import tsdf_cases

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = np.float32
I = np.int32


def host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else a


def same(a, b):
    a, b = np.ascontiguousarray(host(a)), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def mesh_of(name):
    v, f = cases.MESHES[name]
    return dev(v), dev(f)


@pytest.mark.parametrize("name, n", cases.SAMPLE_RUNS)
def test_sampling_equals_the_restatement_and_itself(name, n):
    from gaussianprediction_amd import geometry_ops as G
    v, f = cases.MESHES[name]
    mesh, attributes, want = mesh_of(name), dev(cases.attributes_of(name)), cases.sample_result(name, n)
    got = G.sample_surface(mesh, n)
    inter = G.interpolate(got, mesh, attributes)
    assert got._stats is None
    print(name, n, got.stats)
    assert got.stats == dict(zip(G.SAMPLE_STAT_NAMES, want.counts[:4].tolist())) and (got.stats["status"] != 0) == (name in cases.REFUSED)
    assert [t.dtype for t in got] == [torch.float32, torch.int32, torch.float32] and [tuple(t.shape) for t in got] == [(n, 3), (n,), (n, 2)]
    assert same(got.points, want.points) and same(got.face, want.face) and same(got.bary, want.bary) and same(inter, want.interpolated)
    again = G.sample_surface(mesh, n)                                            # run to run
    assert all(bytes_equal(a, b) for a, b in zip(got, again)) and bytes_equal(G.interpolate(again, mesh, attributes), inter)
    assert same(mesh[0], v) and same(mesh[1], f)                                  # the inputs are read only
    if name not in cases.REFUSED:                                                # the facts, on the device's own output
        weights = ref.face_weights(v, f)[0]
        print(cases.check_samples(v, f, weights, n, host(got.points), host(got.face), host(got.bary)))
        other = G.sample_surface(mesh, n, seed=12345)
        assert not bytes_equal(other.points, got.points)
        cases.check_samples(v, f, weights, n, host(other.points), host(other.face), host(other.bary))


@pytest.mark.parametrize("name", list(cases.CLOUDS))
def test_the_grid_equals_the_brute_force_under_every_rule(name):
    from gaussianprediction_amd import geometry_ops as G
    p, q = cases.CLOUDS[name]
    dist2, index, bad_points, bad_queries = cases.nearest_result(name)
    points, queries = dev(p), dev(q)
    for rule in cases.RULES:
        cell = cases.cell_of(name, rule)
        grid = G.NearestGrid(points, cell or None)
        got = grid.query(queries)
        assert got._stats is None
        assert same(got.dist2, dist2) and same(got.index, index), (name, rule)
        again = grid.query(queries)                                              # the grid is built once and asked often
        fresh = G.nearest(queries, points, cell or None)
        assert bytes_equal(again.dist2, got.dist2) and bytes_equal(again.index, got.index) and bytes_equal(fresh.dist2, got.dist2) and bytes_equal(fresh.index, got.index)
        print(name, rule, got.stats)
        assert got.stats["excluded_points"] == bad_points and got.stats["excluded_queries"] == bad_queries and got.stats == again.stats == fresh.stats
        assert got.stats["dim_x"] * got.stats["dim_y"] * got.stats["dim_z"] <= ref.MAX_CELLS
    assert same(points, p) and same(queries, q)                                   # the inputs are read only


def test_the_device_grid_is_the_emulators(tmp_path):
    """The grid, the rings and the candidates are integers both sides compute alike: equal stats."""
    from gaussianprediction_amd import geometry_ops as G
    emulator = cases.build_emulator(tmp_path, sanitize=False)          # (plain: sanitizers belong to the host test)
    for name, rule in (("uniform", "auto"), ("shifted", "1024"), ("sphere", "7"), ("far", "1024"), ("coplanar", "1024"), ("nonfinite", "auto")):
        p, q = cases.CLOUDS[name]
        cell = cases.cell_of(name, rule)
        got = G.nearest(dev(q), dev(p), cell or None)
        want = emulator.nearest(p, q, cell)
        assert [got.stats[k] for k in G.STAT_NAMES] == want[2].tolist(), (name, rule)
    assert G.nearest(dev(cases.CLOUDS["uniform"][1]), dev(cases.CLOUDS["uniform"][0])).stats["max_ring"] >= 2


def test_nearest_equals_knn_points():
    from gaussianprediction_amd import geometry_ops as G, knn_ops
    rng = np.random.default_rng(4)
    q, p = dev(rng.normal(size=(3000, 3)).astype(F)), dev(rng.normal(size=(5000, 3)).astype(F))
    got = G.nearest(q, p)
    d, i = knn_ops.knn_points(q[None], p[None], K=1)
    assert bytes_equal(got.dist2, d.reshape(-1)) and torch.equal(got.index.long(), i.reshape(-1))
    print(got.stats)
    assert got.stats["candidates"] < 3000 * 5000 // 20


def test_stats_are_the_only_device_read():
    from gaussianprediction_amd import geometry_ops as G
    mesh, cloud = mesh_of("33_torus"), dev(cases.CLOUDS["uniform"][0])
    G.sample_surface(mesh, 100), G.nearest(cloud, cloud)                          # (first calls: the library loads, the allocator grows)
    torch.cuda.synchronize()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # ("a prototype feature")
        torch.cuda.set_sync_debug_mode("error")          # a synchronising call raises
    try:
        samples = G.sample_surface(mesh, 1000)
        inter = G.interpolate(samples, mesh, mesh[0])
        grid = G.NearestGrid(cloud)
        near = grid.query(samples.points)
        table = G.metrics_table(near.dist2, near.dist2, (0.1,))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert samples._stats is None and near._stats is None and tuple(table.shape) == (G.COLUMNS,) and tuple(inter.shape) == (1000, 3)
    assert samples.stats["status"] == 0 and near.stats["excluded_queries"] == 0 and samples._stats is not None


@pytest.mark.parametrize("name", list(cases.METRICS))
def test_the_table_equals_the_restatement_and_itself(name):
    from gaussianprediction_amd import geometry_ops as G
    a, b = cases.METRICS[name]
    da, db = dev(a), dev(b)
    got = G.metrics_table(da, db, cases.THRESHOLDS)
    assert got.dtype == torch.float64 and same(got, cases.metrics_result(name))
    assert bytes_equal(G.metrics_table(da, db, cases.THRESHOLDS), got) and same(da, a) and same(db, b)


def test_the_sphere_on_the_device():
    from gaussianprediction_amd import geometry_ops as G
    n = 20000
    mesh = mesh_of("33_sphere")
    samples = G.sample_surface(mesh, n)
    largest = cases.check_sphere_samples(host(samples.points))
    row = G.cloud_distance(samples.points, dev(cases.sphere_points(n)))
    print("largest | |p - c| - r |:", largest, "accuracy", row["accuracy"], "completeness", row["completeness"], "hausdorff", row["hausdorff"])
    assert row["accuracy"] <= cases.SPHERE_BOUND and row["count_ab"] == row["count_ba"] == n


def test_metric_facts_on_the_device():
    from gaussianprediction_amd import geometry_ops as G

    def distance(a, b, thresholds):
        out = G.cloud_distance(dev(a), dev(b), thresholds)
        out["index_ab"] = host(G.nearest(dev(a), dev(b)).index)
        return out

    lat = cases.check_metric_facts(distance)
    print({k: lat[k] for k in ("accuracy", "completeness", "hausdorff", "fscore")})


def test_mesh_distance_of_a_mesh_and_its_simplification():
    from gaussianprediction_amd import geometry_ops as G, mesh_simplify
    from gaussianprediction_amd.tsdf_ops import Mesh
    v, f = mesh_of("33_sphere")
    voxel = 3 * tsdf_cases.EXTRACT["33_sphere"][0].voxel
    light = mesh_simplify.simplify(Mesh(v, f, None), voxel)
    light = light.mesh if hasattr(light, "mesh") else light
    row = G.mesh_distance((v, f), (light[0], light[1]), n=20000)
    print("simplify(voxel_size = %g): %d -> %d faces" % (voxel, f.shape[0], light[1].shape[0]), {k: row[k] for k in ("accuracy", "completeness", "chamfer_l1", "hausdorff", "fscore")})
    assert all(np.isfinite(row[k]) for k in ("accuracy", "completeness", "chamfer_l1", "chamfer_l2", "hausdorff")) and row["n"] == 20000
    itself = G.mesh_distance((v, f), (v, f), n=20000)                             # other samples of the same surface: small, not zero
    assert 0 < itself["accuracy"] < voxel and itself["count_ab"] == 20000
    last = G.mesh_distance((v, f), (v, f), n=1000, seed=2 ** 64 - 1)              # the second seed wraps to 0
    assert last["count_ab"] == last["count_ba"] == 1000 and last["accuracy"] > 0


def test_evaluate_mesh_dirs_and_mesh_motion(tmp_path):
    from gaussianprediction_amd import eval_render, geometry_ops as G
    from gaussianprediction_amd.io_formats import save_mesh_ply
    pred, gt = tmp_path / "run" / "meshes", tmp_path / "truth"
    os.makedirs(pred), os.makedirs(gt)
    for k, (a, b) in enumerate((("33_sphere", "33_sphere"), ("33_torus", "33_torus"), ("33_sphere", "33_torus"))):
        save_mesh_ply(str(pred / f"{k:05d}.ply"), *cases.MESHES[a])
        save_mesh_ply(str(gt / f"{k:05d}.ply"), *cases.MESHES[b])
    save_mesh_ply(str(gt / "00007.ply"), *cases.MESHES["diagonal"])
    out = G.evaluate_mesh_dirs(str(pred), str(gt), n=4000, thresholds=(0.05, 0.2))
    assert out["pairs"] == 3 and [r["name"] for r in out["rows"]] == ["00000.ply", "00001.ply", "00002.ply"] and out["unpaired"] == ["00007.ply"]
    assert out["rows"][0]["accuracy"] < out["rows"][2]["accuracy"] and out["rows"][0]["fscore"][1] == 1.0 and out["rows"][2]["fscore"][1] < 1.0
    assert abs(out["mean"]["accuracy"] - sum(r["accuracy"] for r in out["rows"]) / 3) < 1e-15
    assert json.load(open(tmp_path / "run" / "mesh_metrics.json"))["mean"]["accuracy"] == out["mean"]["accuracy"]
    motion = eval_render.mesh_motion(str(pred), n=4000, thresholds=(0.05,))
    assert [r["frames"] for r in motion["rows"]] == [(0, 1), (1, 2)] and motion["rows"][0]["accuracy"] > 0.05 and motion["rows"][1]["completeness"] > 0.05
    listed = eval_render.mesh_motion([mesh_of("33_sphere"), mesh_of("33_torus")], n=4000, thresholds=(0.05,))
    assert listed["rows"][0]["accuracy"] == motion["rows"][0]["accuracy"] and listed["mean"]["accuracy"] == listed["rows"][0]["accuracy"]


def test_refusals_on_the_device():
    from gaussianprediction_amd import _lib, geometry_ops as G
    for name in cases.REFUSED:
        s = G.sample_surface(mesh_of(name), 50)
        assert s.stats["status"] == G.REFUSED_EMPTY and bool(torch.isnan(s.points).all()) and bool((s.face == -1).all())
        with pytest.raises(_lib.GpHipError, match="mesh_a has no area to sample"):
            G.mesh_distance(mesh_of(name), mesh_of("diagonal"), n=50)
    with pytest.raises(_lib.GpHipError, match="mesh_b has no area"):
        G.mesh_distance(mesh_of("diagonal"), mesh_of("no_area"), n=50)
    none = G.nearest(dev(cases.CLOUDS["uniform"][1]), torch.zeros(0, 3, device=DEV))
    assert bool(torch.isinf(none.dist2).all()) and bool((none.index == -1).all()) and none.stats["candidates"] == 0
    empty = G.nearest(torch.zeros(0, 3, device=DEV), dev(cases.CLOUDS["uniform"][0]))
    assert tuple(empty.dist2.shape) == (0,) and empty.stats["dim_x"] == 22
    row = G.cloud_distance(dev(cases.CLOUDS["none_usable"][0]), dev(cases.CLOUDS["uniform"][0]))
    assert row["count_ab"] == 0 and np.isnan(row["accuracy"]) and np.isnan(row["hausdorff"]) and row["fscore"] == [0.0, 0.0, 0.0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.NearestGrid(dev(cases.CLOUDS["uniform"][0])).query(torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.nearest(torch.zeros(3, 3), dev(cases.CLOUDS["uniform"][0]))
