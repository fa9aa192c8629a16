"""The signed-distance volumes on the device against the numpy restatement tests/volume_ref.py (a brute force, no tree) on every case
of tests/volume_cases.py, bit for bit; every call twice with equal bytes and the inputs unchanged; the tree's stats equal to the
stand-alone CPU build's; MeshTree.query byte-equal to SurfaceGrid.query and SignedTree.query to SignedGrid.query; the lattice equal
to the query on its materialised points and to the restatement; the comparison's counts; the IoU of the cube against itself moved by
half its side; remesh of the cube (watertight, Euler characteristic 2, wound outward, within a cell's diagonal of the cube, its
volume between derived bounds); contains; no synchronising call before stats; the refusals.

Sign and sdf rows are compared as sdf_cases.compare does: exact on every row the restatement does not mark unstable, |sdf| exact
everywhere.  Measured on an MI355X: see DESIGN section 34."""
import warnings

import numpy as np
import pytest
import torch

import sdf_cases
import sdf_ref
import volume_cases as cases
import volume_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = np.float32
I = np.int32
same = cases.same


def host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else a


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def rows_equal(a, b):
    return all(bytes_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return cases.build_emulator(tmp_path_factory.mktemp("volume_emulate"), sanitize=False)          # (plain: sanitizers belong to the host test)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_device_tree_against_the_restatement_the_emulator_and_the_grid(emulator, name):
    from gaussianprediction_amd import surface_ops as S, volume_ops as V
    v, f, q = cases.CASES[name]
    want = cases.result(name)
    mesh, queries = (dev(v), dev(f)), dev(q)
    tree = V.MeshTree(mesh)
    got = tree.query(queries)
    assert got._stats is None and isinstance(got, S.PointSurface)
    assert [t.dtype for t in got] == [torch.float32, torch.int32, torch.int32, torch.float32, torch.float32] and got._words.dtype == torch.int64
    assert all(cases.equal_result([host(t) for t in got], want)), (name, cases.equal_result([host(t) for t in got], want))
    again, fresh = tree.query(queries), V.MeshTree(mesh).query(queries)                        # two runs, equal bytes: the same tree asked again, a fresh one
    assert rows_equal(again, got) and rows_equal(fresh, got) and bytes_equal(again._words, got._words) and bytes_equal(fresh._words, got._words)
    grid = S.SurfaceGrid(mesh).query(queries)
    assert rows_equal(got, grid)                                                               # byte-equal to the grid
    emulated = emulator.run(v, f, q)
    print(name, got.stats, "grid candidates", grid.stats["candidates"])
    assert [got.stats[k] for k in V.STAT_NAMES] == emulated.stats.tolist() == host(got._words).tolist()          # the walk itself is the same on both
    assert got.stats["status"] == 0 and got.stats["excluded_faces"] == want.excluded_faces and got.stats["excluded_queries"] == want.excluded_queries
    assert same(host(mesh[0]), v) and same(host(mesh[1]), f) and same(host(queries), q)          # the inputs are read only


@pytest.mark.parametrize("name", ["sdf/" + k for k in sdf_cases.CASES] + list(cases.DEEP))
def test_the_signed_tree_against_the_signed_grid_and_the_restatement(name):
    from gaussianprediction_amd import sdf_ops as D, volume_ops as V
    v, f, q = cases.CASES[name]
    mesh, queries = (dev(v), dev(f)), dev(q)
    tree = V.SignedTree(mesh)
    got = tree.query(queries)
    grid = D.SignedGrid(mesh, topology=tree.normals.topology).query(queries)
    assert isinstance(got, D.SignedSurface) and rows_equal(got, grid) and rows_equal(got.surface, grid.surface) and bytes_equal(got._words, grid._words)
    assert rows_equal(tree.query(queries), got) and bytes_equal(tree.contains(queries), got.sign < 0)
    want = cases.signed(name).signed
    stable = ~want.unstable
    assert same(host(got.kind), want.kind) and same(host(got.element), want.element)
    assert same(host(got.sign)[stable], want.sign[stable]) and same(host(got.sdf)[stable], want.sdf[stable]) and same(np.abs(host(got.sdf)), np.abs(want.sdf))


@pytest.mark.parametrize("name", list(cases.LATTICES))
def test_the_lattice_against_the_query_on_its_points_and_the_restatement(emulator, name):
    from gaussianprediction_amd import tsdf_ops as T, volume_ops as V
    v, f, origin, voxel, dims = cases.LATTICES[name]
    want = cases.lattice(name)
    mesh = (dev(v), dev(f))
    tree = V.SignedTree(mesh)
    got = tree.lattice(origin, voxel, dims)
    assert got._stats is None and got.sdf.dtype == torch.float32 and tuple(got.sdf.shape) == (dims[2], dims[1], dims[0]) and got.dims == tuple(dims)
    assert got.origin == tuple(float(o) for o in origin) and got.voxel_size == float(voxel)
    cases.compare_sdf(host(got.sdf), want)
    points = dev(want.points)
    rows = tree.query(points)
    assert bytes_equal(got.sdf.reshape(-1), rows.sdf)                                          # the lattice is the query on the materialised points
    assert bytes_equal(got.inside(), got.sdf < 0)
    again = tree.lattice(origin, voxel, dims)
    assert bytes_equal(again.sdf, got.sdf) and bytes_equal(again._words, got._words)
    emulated = emulator.run(v, f, want.points, tables=want.tables, lattice=(origin, voxel, dims))
    words = host(got._words)
    print(name, got.stats)
    assert words[:ref.STAT_WORDS].tolist() == emulated.lattice_stats[:ref.STAT_WORDS].tolist() == [rows.surface.stats[k] for k in V.STAT_NAMES]
    assert words[ref.STAT_WORDS:].tolist() == host(rows._words).tolist() and [got.stats[k] for k in V.LATTICE_NAMES] == words.tolist()
    # the lattice is a TsdfVolume's: to_tsdf keeps origin, voxel and dims, scales and clamps the distance, and weighs the finite points
    volume = got.to_tsdf()
    assert isinstance(volume, T.TsdfVolume) and volume.color is None and volume.origin == got.origin and volume.voxel_size == got.voxel_size and volume.dims == got.dims
    trunc = F(4.0 * float(voxel))
    assert volume.trunc == 4.0 * float(voxel) and same(host(volume.tsdf), np.clip(host(got.sdf) / trunc, F(-1), F(1)).astype(F)) and same(host(volume.weight), np.isfinite(host(got.sdf)).astype(F))


def test_a_mesh_without_a_usable_face_gives_an_infinite_volume():
    from gaussianprediction_amd import volume_ops as V
    v, f, _ = cases.CASES["nf_5"]                              # (every corner NaN: no face is usable; an index out of range is mesh_smooth.edges' to refuse)
    got = V.sdf_volume((dev(np.full_like(v, np.nan)), dev(f)), voxel_size=0.5, origin=(0, 0, 0), dims=(3, 2, 2))
    assert torch.isinf(got.sdf).all() and (got.sdf > 0).all() and got.stats["excluded"] == 12 and got.stats["excluded_faces"] == len(f)
    tsdf = got.to_tsdf()
    assert not host(tsdf.weight).any() and (host(tsdf.tsdf) == 1).all()


@pytest.mark.parametrize("n", list(cases.COMPARES))
def test_the_comparison(n):
    from gaussianprediction_amd import volume_ops as V
    a, b = cases.COMPARES[n]
    got = V.compare(dev(a), dev(b))
    assert got.dtype == torch.int64 and same(host(got), ref.compare(a, b)) and bytes_equal(V.compare(dev(a), dev(b)), got)
    assert host(V.compare(dev(a[:0]), dev(b[:0]))).tolist() == [0] * 6


def test_the_iou_of_the_cube_against_itself_moved_by_half_its_side():
    from gaussianprediction_amd import volume_ops as V
    case = cases.IOU
    a, b = (dev(case.a[0]), dev(case.a[1])), (dev(case.b[0]), dev(case.b[1]))
    va = V.SignedTree(a).lattice(case.origin, case.voxel, case.dims)
    vb = V.SignedTree(b).lattice(case.origin, case.voxel, case.dims)
    counts = host(V.compare(va.sdf, vb.sdf)).tolist()
    print("counts on the case's lattice:", counts)
    assert counts == list(case.counts) + [21 * 16 * 16]
    got = V.volume_iou(a, b, voxel_size=0.1)
    print(got)
    assert got["iou"] == 500 / 1500 and got["undetermined"] == 0 and got["points"] == 21 * 16 * 16 and got["oriented"] is True and got["voxel_size"] == float(F(0.1))
    cell = float(F(0.1)) ** 3
    assert (got["volume_a"], got["volume_b"], got["intersection"], got["union"]) == (1000 * cell, 1000 * cell, 500 * cell, 1500 * cell)
    assert V.volume_iou(a, b, voxel_size=0.1) == got and V.volume_iou(a, a, voxel_size=0.1)["iou"] == 1.0
    flipped = (b[0], b[1][:, [0, 2, 1]].contiguous())
    assert V.volume_iou(a, flipped, voxel_size=0.1)["oriented"] is False


def test_remesh_of_the_cube():
    from gaussianprediction_amd import mesh_smooth as MS, sdf_ops as D, surface_ops as S, tsdf_ops as T, volume_ops as V
    case = cases.REMESH
    cube = (dev(case.mesh[0]), dev(case.mesh[1]))
    voxel = float(case.voxel)
    origin, _, dims = case.explicit
    for name, mesh in (("lattice_for's lattice", V.remesh(cube, voxel_size=voxel)), ("the explicit lattice", V.sdf_volume(cube, voxel_size=voxel, origin=origin, dims=dims).to_tsdf().extract())):
        assert isinstance(mesh, T.Mesh) and mesh.colors is None and mesh.vertices.dtype == torch.float32 and mesh.faces.dtype == torch.int32
        nv, nf = mesh.vertices.shape[0], mesh.faces.shape[0]
        topology = MS.edges(mesh.faces, nv)
        normals = D.pseudonormals(mesh, topology)
        distance = np.sqrt(host(S.SurfaceGrid(cube).query(mesh.vertices).dist2).astype(np.float64))
        volume = normals.stats["volume"]
        print(name, "vertices", nv, "faces", nf, "edges", topology.edge.shape[0], topology.stats, "volume", volume, "farthest vertex", distance.max(), "of", np.sqrt(3.0) * voxel)
        assert topology.stats["watertight"] and nv - topology.edge.shape[0] + nf == 2                   # closed, and a sphere's Euler characteristic
        assert normals.stats["outward"]
        assert distance.max() <= np.sqrt(3.0) * voxel          # a crossing lattice edge is at most a cell's diagonal long, and the exact sign changes only across the surface
        assert (1 - 2 * np.sqrt(3.0) * voxel) ** 3 <= volume <= (1 + 2 * np.sqrt(3.0) * voxel) ** 3
    again = V.remesh(cube, voxel_size=voxel)
    assert bytes_equal(again.vertices, V.remesh(cube, voxel_size=voxel).vertices)


def test_contains_on_the_cube():
    from gaussianprediction_amd import sdf_ops as D, volume_ops as V
    cube = (dev(cases.CUBE_V), dev(cases.CUBE_F))
    queries = dev(np.concatenate([sdf_cases.CUBE_CORNERS, sdf_cases.CUBE_CENTRES]))
    inside = V.SignedTree(cube).contains(queries)
    assert inside.dtype == torch.bool and host(inside).tolist() == [False] * 8 + [True] * 6 and bytes_equal(inside, D.contains(queries, cube))


def test_no_synchronising_call_before_stats():
    from gaussianprediction_amd import volume_ops as V
    v, f, q = cases.CASES["deep_torus"]
    mesh, cloud = (dev(v), dev(f)), dev(q)
    warm = V.SignedTree(mesh)                                          # (first calls: the library loads, the allocator grows; the topology's read)
    warm.query(cloud), warm.lattice((-1.5, -1.5, -0.5), 0.25, (12, 12, 4)), V.compare(warm.lattice((-1.5, -1.5, -0.5), 0.25, (12, 12, 4)).sdf, warm.lattice((-1.5, -1.5, -0.5), 0.25, (12, 12, 4)).sdf)
    V.MeshTree(mesh).query(cloud)
    torch.cuda.synchronize()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # ("a prototype feature")
        torch.cuda.set_sync_debug_mode("error")          # a synchronising call raises
    try:
        tree = V.MeshTree(mesh)                                        # the build reads nothing
        rows = tree.query(cloud)
        signed = V.SignedTree(mesh, topology=warm.normals.topology)    # with topology=: nothing is read
        got = signed.query(cloud)
        inside = signed.contains(cloud)
        volume = signed.lattice((-1.5, -1.5, -0.5), 0.25, (12, 12, 4))
        tsdf = volume.to_tsdf()
        counts = V.compare(volume.sdf, volume.sdf)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert rows._stats is None and got._stats is None and got.surface._stats is None and volume._stats is None and tuple(counts.shape) == (6,) and tsdf.color is None
    assert rows.stats["levels"] == ref.levels(len(f))[0] and rows._stats is not None and volume.stats["inside"] == int(volume.inside().sum()) == int(host(counts)[0])
    assert int(inside.sum()) == got.stats["inside"]


def test_foreign_input_and_the_refusals():
    from gaussianprediction_amd import _lib, mesh_smooth as MS, volume_ops as V
    v, f, origin, voxel, dims = cases.LATTICES["cube_543"]
    want = cases.lattice("cube_543")
    bad = f.copy()
    bad[3, 1], bad[7, 0], bad[9, 2] = 99, -5, 2 ** 31 - 1                                      # outside the vertices: those faces are no candidates and nothing is read through them
    got = V.MeshTree((dev(v), dev(bad))).query(dev(want.points))
    assert all(cases.equal_result([host(t) for t in got], ref.surface_ref.point_mesh(want.points, v, bad))) and got.stats["excluded_faces"] == 3
    other = MS.edges(dev(sdf_cases.CASES["flat_tet"][1]), 4)                                   # another mesh's topology: sides go missing, a -1 is never an index
    strange = V.SignedTree((dev(v), dev(f)), topology=other).lattice(origin, voxel, dims)
    assert strange.stats["sign_status"] == 0 and same(np.abs(host(strange.sdf)), np.abs(want.sdf))
    mesh = (dev(v), dev(f))
    tree = V.SignedTree(mesh)
    for args, word in ((((0, 0, float("nan")), 0.1, (2, 2, 2)), "origin and voxel must be finite"), (((0, 0, 0), -1.0, (2, 2, 2)), "voxel must be > 0"), (((0, 0, 0), 0.1, (2, 0, 2)), "must be >= 1"),
                       (((0, 0, 0), 0.1, (2048, 2048, 512)), "below 2\\^31")):
        with pytest.raises(_lib.GpHipError, match=word):
            tree.lattice(*args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tree.query(torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="same shape"):
        V.compare(torch.zeros(3, device=DEV), torch.zeros(4, device=DEV))
    with pytest.raises(_lib.GpHipError, match="7\\*nx\\*ny\\*nz must be below 2\\^31"):
        V.SdfVolume(torch.zeros(1, device=DEV), (0, 0, 0), 0.1, (1024, 1024, 512), torch.zeros(16, dtype=torch.int64, device=DEV)).to_tsdf()
    l, st = V.lib(), _lib.stream_ptr(torch.device(DEV, 0))
    scratch = torch.empty(4096, dtype=torch.uint8, device=DEV)
    assert l.gp_volume_query(scratch, 2 ** 31, scratch, 12, scratch, scratch, scratch, scratch, scratch, scratch, st) == 1 and b"2^31 - 1" in l.gp_last_error()
    assert l.gp_volume_tree(mesh[0], mesh[1], 8, 2 ** 26, scratch, st) == 1 and b"nf must be below 2^26" in l.gp_last_error()
    assert l.gp_volume_compare(scratch, scratch, -1, scratch, st) == 1 and b"2^31 - 1" in l.gp_last_error()
