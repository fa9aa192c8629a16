"""The point-to-surface distance on the device against the numpy restatement tests/surface_ref.py on every case of
tests/surface_cases.py, under every cell rule and both W: all five outputs bit for bit; every call twice with equal bytes; the inputs
unchanged; stats as the only device read of a query; facts with derived bars on the device's own output (never farther than the
vertices, samples on their own surface, no sampling floor, the analytic sphere); interpolate through the result; surface_distance of
a mesh and its simplification beside mesh_distance; evaluate_mesh_dirs and mesh_motion with surface=True; a pair capacity one too
small refused by status with a guard region intact.

Measured on an MI355X: see DESIGN section 31."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import geometry_cases
import surface_cases as cases
import surface_ref as ref
import tsdf_cases

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = np.float32
I = np.int32


def host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else a


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def mesh_of(name):
    v, f = geometry_cases.MESHES[name]
    return dev(v), dev(f)


def own_surface_bar(vertices):
    """A float32 sample ((b - a) * u1 + a) + (c - a) * u2 lies within (2 + 2 + 3 + 4 + 5) * 2^-24 * max|coordinate| of its face per
    component: 16 * sqrt(3) * 2^-24 * max|coordinate| in all."""
    return 16 * np.sqrt(3.0) * 2.0 ** -24 * float(np.abs(vertices).max())


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_device_equals_the_restatement_and_itself(name):
    from gaussianprediction_amd import surface_ops as S
    v, f, q = cases.CASES[name]
    want = cases.result(name)
    mesh, queries = (dev(v), dev(f)), dev(q)
    for rule in cases.RULES:
        for wide in cases.WIDE:
            cell = cases.cell_of(name, rule)
            grid = S.SurfaceGrid(mesh, cell or None, wide_cells=wide)
            got = grid.query(queries)
            assert got._stats is None
            assert [t.dtype for t in got] == [torch.float32, torch.int32, torch.int32, torch.float32, torch.float32]
            equal = cases.equal_result([host(t) for t in got], want)
            assert all(equal), (name, rule, wide, equal)
            again = grid.query(queries)                                              # the grid is built once and asked often
            fresh = S.SurfaceGrid(mesh, cell or None, wide_cells=wide).query(queries)
            assert all(bytes_equal(a, g) for a, g in zip(again, got)) and all(bytes_equal(a, g) for a, g in zip(fresh, got))
            print(name, rule, wide, got.stats)
            assert got.stats["excluded_faces"] == want.excluded_faces and got.stats["excluded_queries"] == want.excluded_queries and got.stats["status"] == 0
            assert got.stats == again.stats == fresh.stats and (got.stats["pairs"], got.stats["wide"]) == (grid.pairs, grid.wide)
            assert got.stats["dim_x"] * got.stats["dim_y"] * got.stats["dim_z"] <= 2 ** 24
    assert all(cases.equal_result([host(t) for t in S.point_mesh_distance(queries, mesh)], want))      # the one-shot form
    assert cases.same(host(mesh[0]), v) and cases.same(host(mesh[1]), f) and cases.same(host(queries), q)      # the inputs are read only


def test_the_device_grid_is_the_emulators(tmp_path):
    """The grid, the boxes, the rings and the candidates are integers both sides compute alike: equal stats."""
    from gaussianprediction_amd import surface_ops as S
    emulator = cases.build_emulator(tmp_path, sanitize=False)          # (plain: sanitizers belong to the host test)
    for name, rule, wide in (("33_torus", "auto", 64), ("33_torus", "1024", 64), ("33_sphere", "7", 1), ("hub", "7", 64), ("far_origin", "1024", 64), ("uneven", "1024", 64), ("mixed", "auto", 64)):
        v, f, q = cases.CASES[name]
        cell = cases.cell_of(name, rule)
        got = S.SurfaceGrid((dev(v), dev(f)), cell or None, wide_cells=wide).query(dev(q))
        want = emulator.query(v, f, q, cell, wide)
        assert [got.stats[k] for k in S.STAT_NAMES] == want[5][:11].tolist(), (name, rule, wide)


def test_stats_are_the_only_device_read_of_a_query():
    from gaussianprediction_amd import geometry_ops as G, surface_ops as S
    mesh, cloud = mesh_of("33_torus"), dev(cases.CASES["33_torus"][2])
    grid = S.SurfaceGrid(mesh)                                         # (the build's one 16-byte read; first calls: the library loads, the allocator grows)
    grid.query(cloud), G.interpolate(grid.query(cloud), mesh, mesh[0])
    torch.cuda.synchronize()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # ("a prototype feature")
        torch.cuda.set_sync_debug_mode("error")          # a synchronising call raises
    try:
        got = grid.query(cloud)
        inter = G.interpolate(got, mesh, mesh[0])
        table = G.metrics_table(got.dist2, got.dist2, (0.1,))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert got._stats is None and tuple(table.shape) == (G.COLUMNS,) and tuple(inter.shape) == (len(cloud), 3)
    assert got.stats["excluded_queries"] == 8 and got._stats is not None and got.stats["max_ring"] >= 2


@pytest.mark.parametrize("name", ["33_sphere", "33_torus"])
def test_the_facts_with_derived_bars(name):
    from gaussianprediction_amd import geometry_ops as G, surface_ops as S
    v, f, q = cases.CASES[name]
    mesh, queries = (dev(v), dev(f)), dev(q)
    grid = S.SurfaceGrid(mesh)
    got = grid.query(queries)
    # the surface is never farther than its own vertices (the slack covers the float32 distance of knn_kernels)
    referenced = dev(v[np.unique(f[ref.usable_faces(v, f)])])
    to_vertices = host(G.NearestGrid(referenced).query(queries).dist2).astype(np.float64)
    d2 = host(got.dist2).astype(np.float64)
    assert (d2 <= to_vertices * (1 + 2.0 ** -20)).all() and np.isfinite(d2).sum() == len(q) - 8
    # samples of a mesh lie on that mesh's surface
    bar = own_surface_bar(v)
    samples = G.sample_surface(mesh, 20000)
    own = np.sqrt(host(grid.query(samples.points).dist2).astype(np.float64))
    print(name, "samples to their own surface: largest", own.max(), "bar", bar, "in units of 2^-24 max|coordinate|:", own.max() / (2.0 ** -24 * np.abs(v).max()))
    assert (own <= bar).all()
    assert (np.sqrt(d2[cases.SAMPLE_ROWS[name]]) <= bar).all()
    # the sampling floor is gone, and the default path still has it
    on = S.surface_distance(mesh, mesh, n=20000)
    off = G.mesh_distance(mesh, mesh, n=20000)
    print(name, "surface_distance(m, m):", {k: on[k] for k in ("accuracy", "completeness", "hausdorff")}, "mesh_distance(m, m):", {k: off[k] for k in ("accuracy", "completeness", "hausdorff")})
    assert all(on[k] <= bar for k in ("accuracy", "completeness", "hausdorff")) and all(off[k] > 1e-3 for k in ("accuracy", "completeness", "hausdorff"))
    assert on["surface"] is True and on["n"] == 20000 and on["count_ab"] == on["count_ba"] == 20000 and "surface" not in off
    assert G.mesh_distance(mesh, mesh, n=20000, surface=True) == on
    if name == "33_sphere":                                                          # the analytic sphere, for the cube queries
        cube = q[cases.CUBE_ROWS].astype(np.float64)
        analytic = np.abs(np.linalg.norm(cube - np.asarray(tsdf_cases.SPHERE.c, np.float64), axis=1) - tsdf_cases.SPHERE.r)
        error = np.abs(np.sqrt(d2[cases.CUBE_ROWS]) - analytic)
        print("the sphere: largest | sqrt(dist2) - | |q - c| - r | |:", error.max(), "bound", geometry_cases.SPHERE_BOUND)
        assert (error <= geometry_cases.SPHERE_BOUND).all()


@pytest.mark.parametrize("name", ["33_torus", "mixed", "hub", "no_faces"])
def test_interpolate_through_the_result(name):
    from gaussianprediction_amd import geometry_ops as G, surface_ops as S
    v, f, q = cases.CASES[name]
    mesh, want = (dev(v), dev(f)), cases.result(name)
    got = S.point_mesh_distance(dev(q), mesh)
    attributes = cases.attributes_of(name)
    assert cases.same(host(G.interpolate(got, mesh, dev(attributes))), ref.interpolate(want, f, attributes))
    if name != "mixed":                                                              # (mixed has non-finite vertices: positions are no attribute there)
        back = host(G.interpolate(got, mesh, mesh[0]))
        ok = host(got.face) >= 0
        assert (np.abs(back[ok].astype(np.float64) - host(got.closest)[ok]) <= 4 * np.spacing(F(np.abs(v).max()))).all() and (back[~ok] == 0).all()


def test_surface_distance_of_a_mesh_and_its_simplification():
    from gaussianprediction_amd import geometry_ops as G, mesh_simplify, surface_ops as S
    from gaussianprediction_amd.tsdf_ops import Mesh
    v, f = mesh_of("33_sphere")
    voxel = 3 * tsdf_cases.EXTRACT["33_sphere"][0].voxel
    light = mesh_simplify.simplify(Mesh(v, f, None), voxel)
    light = light.mesh if hasattr(light, "mesh") else light
    keys = ("accuracy", "completeness", "chamfer_l1", "hausdorff", "fscore")
    on, off = S.surface_distance((v, f), (light[0], light[1]), n=20000), G.mesh_distance((v, f), (light[0], light[1]), n=20000)
    print("simplify(voxel_size = %g): %d -> %d faces" % (voxel, f.shape[0], light[1].shape[0]))
    print("  surface_distance:", {k: on[k] for k in keys})
    print("  mesh_distance:   ", {k: off[k] for k in keys})
    assert all(np.isfinite(on[k]) for k in keys[:4]) and on["surface"] is True
    bar = own_surface_bar(host(v))                                                  # the other mesh's samples lie within it of that mesh's surface: the surface is never farther
    assert 0 < on["accuracy"] <= off["accuracy"] + bar and 0 < on["completeness"] <= off["completeness"] + bar and on["hausdorff"] <= off["hausdorff"] + bar


def test_evaluate_mesh_dirs_and_mesh_motion_through_the_surface(tmp_path):
    from gaussianprediction_amd import eval_render, geometry_ops as G
    from gaussianprediction_amd.io_formats import save_mesh_ply
    pred, gt = tmp_path / "run" / "meshes", tmp_path / "truth"
    os.makedirs(pred), os.makedirs(gt)
    for k, (a, b) in enumerate((("33_sphere", "33_sphere"), ("33_sphere", "33_torus"))):
        save_mesh_ply(str(pred / f"{k:05d}.ply"), *geometry_cases.MESHES[a])
        save_mesh_ply(str(gt / f"{k:05d}.ply"), *geometry_cases.MESHES[b])
    out = G.evaluate_mesh_dirs(str(pred), str(gt), n=4000, thresholds=(0.05, 0.2), surface=True)
    assert out["pairs"] == 2 and all(r["surface"] is True for r in out["rows"]) and out["mean"]["surface"] is True
    assert out["rows"][0]["hausdorff"] <= own_surface_bar(geometry_cases.MESHES["33_sphere"][0]) and out["rows"][0]["fscore"] == [1.0, 1.0] and out["rows"][1]["accuracy"] > 0.05
    written = json.load(open(tmp_path / "run" / "mesh_metrics.json"))
    assert [r["surface"] for r in written["rows"]] == [True, True] and written["mean"]["accuracy"] == out["mean"]["accuracy"]
    plain = G.evaluate_mesh_dirs(str(pred), str(gt), n=4000, thresholds=(0.05, 0.2))
    assert all("surface" not in r for r in plain["rows"]) and plain["rows"][0]["accuracy"] > out["rows"][0]["accuracy"]
    motion = eval_render.mesh_motion([mesh_of("33_sphere"), mesh_of("33_torus")], n=4000, thresholds=(0.05,), surface=True)
    assert motion["rows"][0]["frames"] == (0, 1) and motion["rows"][0]["surface"] is True and motion["rows"][0]["accuracy"] > 0.05 and motion["mean"]["surface"] is True


def test_a_capacity_one_pair_too_small_is_refused_by_status():
    from gaussianprediction_amd import _lib, surface_ops as S
    v, f, q = cases.CASES["33_torus"]
    vertices, faces, queries = dev(v), dev(f), dev(q)
    l, st = S.lib(), _lib.stream_ptr(torch.device(DEV, 0))
    scratch = _lib.scratch(l.gp_surface_scratch_bytes, len(f), 0.0, device=DEV)
    sizes = torch.empty(2, dtype=torch.int64, device=DEV)
    _lib.check(l.gp_surface_grid_count(vertices, faces, len(v), len(f), 0.0, 64, scratch, sizes, st), "gp_surface_grid_count")
    pairs, wide = sizes.tolist()
    assert pairs > 1000
    guard = 4096
    buffer = torch.full((pairs + guard,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)              # the pair array and a guard region after it
    outs = [torch.empty(len(q), dtype=t, device=DEV) for t in (torch.float32, torch.int32, torch.int32)] + [torch.empty(len(q), k, device=DEV) for k in (3, 2)]
    words = torch.empty(S.STAT_WORDS, dtype=torch.int64, device=DEV)

    def fill_and_query(capacity):
        _lib.check(l.gp_surface_grid_fill(len(f), 0.0, 64, scratch, buffer, capacity, st), "gp_surface_grid_fill")
        _lib.check(l.gp_surface_grid_query(queries, len(q), scratch, buffer, len(f), 0.0, *outs, words, st), "gp_surface_grid_query")
        return dict(zip(S.STAT_NAMES, words.tolist()))

    stats = fill_and_query(pairs - 1)
    assert stats["status"] == S.REFUSED_CAPACITY and stats["pairs"] == pairs and stats["candidates"] == 0
    assert bool((buffer == 0x5A5A5A5A).all())                                      # nothing written: not to the array, not past its end
    assert bool(torch.isinf(outs[0]).all()) and bool((outs[1] == -1).all()) and bool(torch.isnan(outs[3]).all())
    stats = fill_and_query(pairs)                                                   # the same scratch, the capacity right: the results
    assert stats["status"] == 0 and bool((buffer[pairs:] == 0x5A5A5A5A).all()) and bool((buffer[:pairs] != 0x5A5A5A5A).all())
    assert cases.same(host(outs[0]), cases.result("33_torus").dist2) and cases.same(host(outs[1]), cases.result("33_torus").face)


def test_refusals_on_the_device():
    from gaussianprediction_amd import _lib, geometry_ops as G, surface_ops as S
    queries = dev(cases.CASES["triangle"][2])
    none = S.point_mesh_distance(queries, mesh_of("no_faces"))
    assert bool(torch.isinf(none.dist2).all()) and bool((none.face == -1).all()) and none.stats["candidates"] == 0 and none.stats["pairs"] == 0
    empty = S.SurfaceGrid(mesh_of("33_torus")).query(torch.zeros(0, 3, device=DEV))
    assert tuple(empty.dist2.shape) == (0,) and tuple(empty.closest.shape) == (0, 3) and empty.stats["dim_x"] == ref.auto_cells(len(geometry_cases.MESHES["33_torus"][1]))
    grid = S.SurfaceGrid(mesh_of("diagonal"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        grid.query(torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match=r"\[N, 3\] float32"):
        grid.query(torch.zeros(3, 3, device=DEV, dtype=torch.float64))
    for name in geometry_cases.REFUSED:
        with pytest.raises(_lib.GpHipError, match="surface_distance: mesh_a has no area to sample"):
            S.surface_distance(mesh_of(name), mesh_of("diagonal"), n=50)
    with pytest.raises(_lib.GpHipError, match="mesh_b has no area"):
        G.mesh_distance(mesh_of("diagonal"), mesh_of("no_area"), n=50, surface=True)
