"""The signed distance on the device against the numpy restatement tests/sdf_ref.py on every case of tests/sdf_cases.py: the integer
outputs bit for bit, the float64 tables within TABLE_K * 2^-53 * sum|term|, sign and sdf exactly on every row the restatement does
not mark unstable; every call twice with equal bytes and the inputs unchanged; the device's sign against the winding number on the
closed cases; contains on the cube's corners and centres; the flipped cube inverted; no synchronising call before stats; the signed
metrics of a mesh against itself and against itself inflated by 2 %; evaluate_mesh_dirs and mesh_motion with and without the signed
row; foreign input and the refusals.

Measured on an MI355X: see DESIGN section 33."""
import json
import os
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import geometry_cases
import sdf_cases as cases
import sdf_ref as ref
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
    """DESIGN section 31's own-surface bar: a float32 sample lies within 16 * sqrt(3) * 2^-24 * max|coordinate| of its face."""
    return 16 * np.sqrt(3.0) * 2.0 ** -24 * float(np.abs(vertices).max())


def tensors(grid, got):
    n = grid.normals
    return [n.face_edges, n.edge_normal, n.vertex_normal, n.stats._pending[0], n.stats._pending[1], got.sdf, got.sign, got.kind, got.element, got._words]


def run(name):
    from gaussianprediction_amd import sdf_ops as D
    v, f, q = cases.CASES[name]
    mesh, queries = (dev(v), dev(f)), dev(q)
    grid = D.SignedGrid(mesh)
    got = grid.query(queries)
    return mesh, queries, grid, got


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_device_against_the_restatement_and_itself(name):
    from gaussianprediction_amd import sdf_ops as D
    v, f, q = cases.CASES[name]
    want = cases.result(name)
    mesh, queries, grid, got = run(name)
    assert got._stats is None
    assert [t.dtype for t in tensors(grid, got)] == [torch.int32, torch.float64, torch.float64, torch.float64, torch.int32, torch.float32, torch.int8, torch.int32, torch.int32, torch.int64]
    assert cases.same(host(grid.normals.topology.edge), want.topology.edge)                  # (section 32's, pinned there)
    assert all(cases.same(host(g), w) for g, w in zip(got.surface, (want.surface.dist2, want.surface.face, want.surface.region, want.surface.closest, want.surface.bary)))
    parts = [host(t) for t in tensors(grid, got)]
    seen = SimpleNamespace(face_edges=parts[0], edge_normal=parts[1], vertex_normal=parts[2], volume=parts[3][0], counts=parts[4], sdf=parts[5], sign=parts[6], kind=parts[7],
                           element=parts[8], stats=parts[9], means=host(D.means(got.sdf, got.sign)))
    cases.compare(name, seen)
    # two runs, equal bytes: the same grid asked again, a fresh one, the one-shot form, the tables from a handed topology
    again = grid.query(queries)
    fresh_grid = D.SignedGrid(mesh, topology=grid.normals.topology)
    fresh = fresh_grid.query(queries)
    assert all(bytes_equal(a, b) for a, b in zip(tensors(grid, again), tensors(grid, got))) and all(bytes_equal(a, b) for a, b in zip(tensors(fresh_grid, fresh), tensors(grid, got)))
    one = D.signed_distance(queries, mesh)
    assert all(bytes_equal(a, b) for a, b in zip(one, got)) and bytes_equal(D.contains(queries, mesh), got.sign < 0)
    assert all(bytes_equal(a, b) for a, b in zip(got.surface, grid.grid.query(queries)))      # surface is the PointSurface, unchanged
    print(name, got.stats, dict(grid.normals.stats))
    assert got.stats == again.stats == fresh.stats and [got.stats[k] for k in D.STAT_NAMES] == parts[9].tolist()
    stats = grid.normals.stats
    assert stats["volume"] == float(want.tables.volume) and stats["outward"] == (want.tables.volume > 0) and stats["watertight"] == want.topology.stats["watertight"]
    assert [stats[k] for k in ("skipped", "zero_area", "missing")] == want.tables.counts[1:].tolist() and stats["euler"] == want.topology.stats["euler"]
    assert cases.same(host(mesh[0]), v) and cases.same(host(mesh[1]), f) and cases.same(host(queries), q)      # the inputs are read only


@pytest.mark.parametrize("name", cases.CLOSED)
def test_the_device_sign_against_the_winding_number(name):
    _, _, grid, got = run(name)
    kept, inside = cases.winding_rows(name)
    finite = np.isfinite(cases.CASES[name][2]).all(axis=1)
    print(name, "rows left out:", int((finite & ~kept).sum()), "of", len(kept), "inside:", int(inside[kept].sum()))
    assert (finite & ~kept).sum() <= cases.UNSTABLE_CAP * len(kept)
    flipped = name == "cube_flipped"
    assert (host(got.sign)[kept] == np.where(inside != flipped, -1, 1)[kept]).all()
    assert grid.normals.stats["watertight"] and grid.normals.stats["outward"] == (not flipped)


def test_contains_on_the_cube_and_the_flipped_cube_inverted():
    from gaussianprediction_amd import sdf_ops as D
    v, f, q = cases.CASES["cube"]
    queries = dev(np.concatenate([cases.CUBE_CORNERS, cases.CUBE_CENTRES]))
    inside = host(D.contains(queries, (dev(v), dev(f))))
    assert inside.dtype == np.bool_ and inside.tolist() == [False] * 8 + [True] * 6
    got = D.signed_distance(queries, (dev(v), dev(f)))
    assert (host(got.kind)[:8] == D.KIND_VERTEX).all() and sorted(host(got.element)[:8].tolist()) == list(range(8))
    assert host(got.sdf)[8] == F(-0.5) and np.allclose(host(got.sdf)[:8], np.sqrt(3 * 0.25 ** 2))
    on = D.signed_distance(dev(cases.CUBE_V), (dev(v), dev(f)))                            # the corners themselves: on the surface, not contained
    assert not host(on.sign).any() and not host(on.sdf).any() and on.stats["undetermined"] == 8
    _, _, grid_a, a = run("cube")
    _, _, grid_b, b = run("cube_flipped")
    assert bytes_equal(b.sign, -a.sign) and bytes_equal(b.sdf, -a.sdf) and bytes_equal(b.kind, a.kind)
    assert (a.stats["inside"], a.stats["outside"]) == (b.stats["outside"], b.stats["inside"])
    assert grid_a.normals.stats["volume"] == 1.0 == -grid_b.normals.stats["volume"] and grid_a.normals.stats["outward"] and not grid_b.normals.stats["outward"]
    assert host(D.contains(queries, (dev(v), dev(cases.CASES["cube_flipped"][1])))).tolist() == [True] * 8 + [False] * 6      # wound inward: every answer inverted


def test_no_synchronising_call_before_stats():
    from gaussianprediction_amd import sdf_ops as D
    v, f, q = cases.CASES["33_torus"]
    mesh, cloud = (dev(v), dev(f)), dev(q)
    grid = D.SignedGrid(mesh)                                          # (the build's reads; first calls: the library loads, the allocator grows)
    grid.query(cloud), D.means(*list(grid.query(cloud))[:2]), D.pseudonormals(mesh, grid.normals.topology)
    torch.cuda.synchronize()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # ("a prototype feature")
        torch.cuda.set_sync_debug_mode("error")          # a synchronising call raises
    try:
        got = grid.query(cloud)
        inside = got.sign < 0
        mean = D.means(got.sdf, got.sign)
        normals = D.pseudonormals(mesh, grid.normals.topology)         # with topology=: nothing is read
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert got._stats is None and got.surface._stats is None and normals.stats._values is None and tuple(mean.shape) == (D.MEAN_WORDS,)
    want = cases.result("33_torus").signed
    assert got.stats["inside"] == int(inside.sum()) == want.stats[ref.INSIDE] and got._stats is not None
    assert normals.stats["watertight"] and normals.stats["outward"] and normals.stats._values is not None


@pytest.mark.parametrize("name", ["33_sphere", "33_torus"])
def test_a_mesh_against_itself(name):
    from gaussianprediction_amd import geometry_ops as G, sdf_ops as D, surface_ops as S
    mesh = mesh_of(name)
    bar = own_surface_bar(geometry_cases.MESHES[name][0])
    on = D.signed_surface_distance(mesh, mesh, n=20000)
    print(name, {k: on[k] for k in ("signed_accuracy", "signed_completeness", "outside_share_a", "outside_share_b", "accuracy", "oriented")}, "bar", bar)
    assert abs(on["signed_accuracy"]) <= bar and abs(on["signed_completeness"]) <= bar and on["oriented"] is True and on["signed"] is True and on["surface"] is True
    assert 0.0 <= on["outside_share_a"] <= 1.0 and 0.0 <= on["outside_share_b"] <= 1.0
    plain = S.surface_distance(mesh, mesh, n=20000)
    assert {k: on[k] for k in plain} == plain                                              # surface_distance's row, byte for byte, plus the new keys
    assert sorted(set(on) - set(plain)) == ["oriented", "outside_share_a", "outside_share_b", "signed", "signed_accuracy", "signed_completeness"]
    assert G.mesh_distance(mesh, mesh, n=20000, surface="signed") == on == D.signed_surface_distance(mesh, mesh, n=20000)


def test_the_sphere_against_itself_inflated():
    from gaussianprediction_amd import sdf_ops as D
    v, f = geometry_cases.MESHES["33_sphere"]
    c = np.asarray(tsdf_cases.SPHERE.c, np.float64)
    large = ((v.astype(np.float64) - c) * 1.02 + c).astype(F)
    small_mesh, large_mesh = (dev(v), dev(f)), (dev(large), dev(f))
    grown = D.signed_surface_distance(large_mesh, small_mesh, n=20000)                     # the prediction is inflated: it lies outside the truth
    shrunk = D.signed_surface_distance(small_mesh, large_mesh, n=20000)
    keys = ("signed_accuracy", "signed_completeness", "outside_share_a", "outside_share_b", "accuracy", "completeness")
    print("inflated by 2 %:", {k: grown[k] for k in keys})
    print("shrunk by 2 %:  ", {k: shrunk[k] for k in keys})
    assert grown["signed_accuracy"] > 0 > grown["signed_completeness"] and grown["outside_share_a"] > 0.99 and grown["outside_share_b"] < 0.01
    assert shrunk["signed_accuracy"] < 0 < shrunk["signed_completeness"] and shrunk["outside_share_a"] < 0.01 and shrunk["outside_share_b"] > 0.99
    assert grown["oriented"] and shrunk["oriented"]
    # the unsigned columns cannot tell the two apart; the signed ones are their mirror images up to the samples
    assert abs(grown["accuracy"] - shrunk["completeness"]) < 1e-3 and abs(grown["signed_accuracy"] - grown["accuracy"]) < 1e-6
    r = tsdf_cases.SPHERE.r
    assert abs(grown["signed_accuracy"] - 0.02 * r) < 2e-3 * r and abs(shrunk["signed_accuracy"] + 0.02 * r) < 2e-3 * r


def test_evaluate_mesh_dirs_and_mesh_motion_with_and_without_the_signed_row(tmp_path):
    from gaussianprediction_amd import eval_render, geometry_ops as G
    from gaussianprediction_amd.io_formats import save_mesh_ply
    pred, gt = tmp_path / "run" / "meshes", tmp_path / "truth"
    os.makedirs(pred), os.makedirs(gt)
    for k, (a, b) in enumerate((("33_sphere", "33_sphere"), ("33_sphere", "33_torus"))):
        save_mesh_ply(str(pred / f"{k:05d}.ply"), *geometry_cases.MESHES[a])
        save_mesh_ply(str(gt / f"{k:05d}.ply"), *geometry_cases.MESHES[b])
    surface = G.evaluate_mesh_dirs(str(pred), str(gt), n=4000, thresholds=(0.05, 0.2), surface=True)
    before = open(tmp_path / "run" / "mesh_metrics.json").read()
    out = G.evaluate_mesh_dirs(str(pred), str(gt), n=4000, thresholds=(0.05, 0.2), surface="signed")
    assert out["pairs"] == 2 and all(r["signed"] is True and r["surface"] is True for r in out["rows"]) and out["mean"]["signed"] is True and out["mean"]["oriented"] is True
    for got, want in zip(out["rows"], surface["rows"]):
        assert {k: got[k] for k in want} == want                                           # the unsigned columns are what they were
    assert abs(out["rows"][0]["signed_accuracy"]) <= own_surface_bar(geometry_cases.MESHES["33_sphere"][0]) and np.isfinite(out["rows"][1]["signed_accuracy"])
    written = json.load(open(tmp_path / "run" / "mesh_metrics.json"))
    assert written["mean"]["signed_accuracy"] == out["mean"]["signed_accuracy"] and [r["signed"] for r in written["rows"]] == [True, True]
    again = G.evaluate_mesh_dirs(str(pred), str(gt), n=4000, thresholds=(0.05, 0.2), surface=True)
    assert again == surface and open(tmp_path / "run" / "mesh_metrics.json").read() == before          # without it: every byte written is what it was
    meshes = [mesh_of("33_sphere"), mesh_of("33_torus")]
    motion = eval_render.mesh_motion(meshes, n=4000, thresholds=(0.05,), surface="signed")
    plain = eval_render.mesh_motion(meshes, n=4000, thresholds=(0.05,), surface=True)
    assert motion["rows"][0]["frames"] == (0, 1) and motion["rows"][0]["signed"] is True and motion["mean"]["signed"] is True
    assert {k: motion["rows"][0][k] for k in plain["rows"][0]} == plain["rows"][0] and "signed" not in plain["rows"][0] and "signed_accuracy" not in plain["mean"]
    assert "surface" not in eval_render.mesh_motion(meshes, n=4000, thresholds=(0.05,))["rows"][0]


def test_foreign_input_and_the_refusals():
    from gaussianprediction_amd import _lib, mesh_smooth as MS, sdf_ops as D
    from gaussianprediction_amd.surface_ops import PointSurface
    v, f, q = cases.CASES["cube"]
    want = cases.result("cube")
    mesh, queries = (dev(v), dev(f)), dev(q)
    grid = D.SignedGrid(mesh)
    got = grid.query(queries)
    face, region = host(got.surface.face).copy(), host(got.surface.region).copy()
    face[0], face[1], face[2], region[3], region[4] = len(f), -2, 2 ** 31 - 1, 4, -1           # outside their arrays: counted undetermined, never read
    foreign = PointSurface(got.surface.dist2, dev(face), dev(region), got.surface.closest, got.surface.bary, got.surface._words)
    seen = D._sign("test", queries, foreign, mesh[0], mesh[1], grid.normals)
    assert not host(seen.sign)[:5].any() and (host(seen.kind)[:5] == -1).all() and (host(seen.element)[:5] == -1).all() and seen.stats["status"] == 1
    assert cases.same(host(seen.sign)[5:], want.signed.sign[5:]) and seen.stats["undetermined"] == got.stats["undetermined"] + 5
    assert cases.same(host(seen.sdf)[:5], np.sqrt(want.surface.dist2[:5].astype(np.float64)).astype(F))
    other = MS.edges(dev(cases.CASES["flat_tet"][1]), 4)                                       # another mesh's topology: sides go missing, a -1 is never an index
    strange = D.pseudonormals(mesh, other)
    assert strange.stats["missing"] > 0 and cases.same(host(strange.face_edges), ref.tables(v, f, host(other.edge)).face_edges)
    assert D.SignedGrid(mesh, topology=other).query(queries).stats["status"] == 0
    none = D.signed_distance(queries, mesh_of("no_faces"))
    assert np.isinf(host(none.sdf)).all() and none.stats["excluded"] == len(q) and not host(none.sign).any() and (host(none.kind) == -1).all()
    with pytest.raises(RuntimeError, match="topology must be an Edges"):
        D.pseudonormals(mesh, topology=(1, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.signed_distance(torch.zeros(3, 3), mesh)
    with pytest.raises(_lib.GpHipError, match="cell must be finite"):
        D.SignedGrid(mesh, cell=-1.0)
    l, st = D.lib(), _lib.stream_ptr(torch.device(DEV, 0))
    scratch = torch.empty(4096, dtype=torch.uint8, device=DEV)
    assert l.gp_sdf_means(got.sdf, got.sign, 2 ** 31, scratch, scratch, st) == 1 and b"2^31 - 1" in l.gp_last_error()
    assert l.gp_sdf_tables(mesh[0], mesh[1], 8, 12, grid.normals.topology.edge, 37, scratch, scratch, scratch, scratch, scratch, scratch, st) == 1 and b"n_edges must be" in l.gp_last_error()
