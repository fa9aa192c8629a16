"""No GPU: csrc/gp_geometry.h against the binding's table (a binding outside _lib.ABIS); the programs of csrc/geometry_core.h in a
stand-alone build (tests/geometry_emulate.cpp, under the sanitizers where the host compiler can link them) against the numpy
restatement tests/geometry_ref.py on every case of tests/geometry_cases.py -- bit for bit; the grid against the brute force under
every cell rule; facts that do not come from the restatement (samples in their faces, the stratified counts, the sphere, a cloud
against itself, a shifted lattice, swapped arguments); the refusals that need no device."""
import inspect
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import abi_check
import geometry_cases as cases
import geometry_ref as ref
import tsdf_cases
from gaussianprediction_amd import _lib, geometry_ops as G

_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "gp_stream_t": _lib.Ptr}
_POINTEES = {"float", "double", "int32_t", "int64_t", "void"}
F = np.float32
I = np.int32


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the header, the table, the registry ----
def test_prototype_table_equals_the_header_and_stays_out_of_the_registry():
    before = len(_lib.ABIS)
    protos = abi_check.check_table(G.ABI, 9, _SCALARS, _POINTEES)
    assert G.ABI.prototypes is G.PROTOTYPES and G.ABI not in _lib.ABIS and len(_lib.ABIS) == before
    assert os.path.samefile(os.path.join(abi_check.ROOT, "include", G.ABI.header), os.path.join(abi_check.ROOT, "gaussianprediction_amd", "csrc", "gp_geometry.h"))
    for name in ("gp_geometry_sample", "gp_geometry_interpolate", "gp_geometry_grid_build", "gp_geometry_grid_query", "gp_geometry_metrics"):
        assert protos[name][1][-1] == "gp_stream_t"              # the stream is the last parameter
    assert not os.path.exists(os.path.join(abi_check.ROOT, "include", "gp_geometry.h"))
    assert len([h for h in os.listdir(os.path.join(abi_check.ROOT, "include")) if h.endswith(".h")]) == 12      # include/ stays at its twelve


def test_symbols_and_constants():
    text = abi_check.header_text(G.HEADER)
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_GEOMETRY_[A-Z0-9_]+) +(\d+)", text)}
    assert defs["GP_GEOMETRY_ABI_VERSION"] == G.GP_GEOMETRY_ABI_VERSION == G.ABI.version == 1
    for name in ("MAX_FACES", "MAX_CHANNELS", "MAX_AXIS", "MAX_CELLS", "MAX_THRESHOLDS", "WEIGHT_BITS", "STATUS", "BAD_INDEX", "NON_FINITE", "ZERO_WEIGHT", "COUNT_WORDS",
                 "REFUSED_EMPTY", "REFUSED_TOO_MANY", "STAT_WORDS", "COLUMNS", "PRECISION", "RECALL", "FSCORE"):
        assert defs["GP_GEOMETRY_" + name] == getattr(G, name) == getattr(ref, name), name
    assert (G.MAX_FACES, G.MAX_AXIS, G.MAX_CELLS, G.MAX_THRESHOLDS, G.MAX_CHANNELS) == (2 ** 26, 1024, 2 ** 24, 8, 8)
    assert [defs["GP_GEOMETRY_" + n.upper()] for n in G.STAT_NAMES] == list(range(8)) == [getattr(ref, n.upper()) for n in G.STAT_NAMES]
    assert [defs["GP_GEOMETRY_" + n.upper()] for n in G.COLUMN_NAMES] == list(range(13)) and G.COLUMNS == G.FSCORE + G.MAX_THRESHOLDS
    assert G.SAMPLE_STAT_NAMES == ("status", "bad_index", "non_finite", "zero_weight")
    assert G.MAX_FACES * 2 ** (G.WEIGHT_BITS + 1) <= 2 ** 63                 # the total weight fits
    assert "0x9E3779B97F4A7C15" in open(os.path.join(abi_check.ROOT, "include", G.HEADER)).read()          # the constants of h stand in the header
    abi_check.check_applied(G.ABI)


# ---- the programs in a stand-alone build, under the sanitizers ----
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return cases.build_emulator(tmp_path_factory.mktemp("geometry_emulate"), sanitize=True)


@pytest.mark.parametrize("name, n", cases.SAMPLE_RUNS)
def test_the_emulated_sampling_against_the_restatement(emulator, name, n):
    v, f = cases.MESHES[name]
    want = cases.sample_result(name, n)
    got = emulator.samples(v, f, n, 0, cases.attributes_of(name))
    print(name, got[0].tolist(), want.total)
    for k, (g, w) in enumerate(zip(got, (want.counts, want.points, want.face, want.bary, want.interpolated))):
        assert same(g, w), (name, k)
    assert (got[0][ref.STATUS] != 0) == (name in cases.REFUSED)


@pytest.mark.parametrize("name", list(cases.CLOUDS))
def test_the_emulated_grid_against_the_brute_force_under_every_rule(emulator, name):
    p, q = cases.CLOUDS[name]
    dist2, index, bad_points, bad_queries = cases.nearest_result(name)
    seen = {}
    for rule in cases.RULES:
        got = emulator.nearest(p, q, cases.cell_of(name, rule))
        print(name, rule, got[2].tolist(), got[3].tolist())
        assert same(got[0], dist2) and same(got[1], index), (name, rule)
        assert got[2][ref.EXCLUDED_POINTS] == bad_points and got[2][ref.EXCLUDED_QUERIES] == bad_queries
        assert got[3][3] == got[3][:3].prod() <= ref.MAX_CELLS and got[3][:3].max() <= ref.MAX_AXIS
        seen[rule] = got
    back = emulator.nearest(p, q, cases.cell_of(name, "7"), backwards=True)          # another order inside the cells: equal bytes
    assert all(same(g, b) for g, b in zip(seen["7"], back))


def test_the_clouds_reach_what_they_are_for(emulator):
    run = lambda name, rule: emulator.nearest(*cases.CLOUDS[name], cases.cell_of(name, rule))          # noqa: E731
    u = run("uniform", "auto")
    assert u[3].tolist() == [22, 22, 22, 22 ** 3] and u[2][ref.MAX_RING] >= 2 and u[2][ref.SWEPT] == 0 and ref.auto_cells(3000) == 22
    assert u[2][ref.CANDIDATES] < 200 * 3000 // 10                                   # the grid is what makes it cheap
    assert run("uniform", "1024")[3].tolist() == [256, 256, 256, 2 ** 24]           # 1024 halved twice
    s = run("shifted", "1024")
    assert s[3][3] == 2 ** 24 and np.spacing(F(1e6)) > 1.0 / 256                     # a cell is smaller than an ulp
    lat = cases.nearest_result("lattice")
    assert (lat[0] == 0.75).all() and len(np.unique(lat[1])) > 100                   # eight at equal distance; the answer is the smallest index
    p, q = cases.CLOUDS["lattice"]
    ties = (((q[:, None, :] - p[None, :, :]) ** 2).sum(-1) == 0.75)
    assert (ties.sum(axis=1) == 8).all() and (lat[1] == ties.argmax(axis=1)).all()
    assert run("identical", "auto")[3].tolist() == [1, 1, 1, 1] and (cases.nearest_result("identical")[1] == 0).all()
    assert run("collinear", "1024")[3].tolist() == [1024, 1, 1, 1024] and run("coplanar", "1024")[3].tolist() == [1024, 1024, 1, 2 ** 20]
    assert run("boundaries", "7")[3].tolist() == [7, 7, 7, 343]
    far = run("far", "1024")
    assert far[2][ref.SWEPT] == 20 and far[2][ref.CANDIDATES] >= 20 * 3000
    assert run("sphere", "auto")[2][ref.CANDIDATES] < 200 * 3000 // 20
    none = run("none_usable", "auto")
    assert np.isinf(none[0]).all() and (none[1] == -1).all() and none[2][ref.EXCLUDED_POINTS] == 40
    over = run("overflow", "auto")
    assert np.isinf(over[0]).all() and (over[1] == 1).all() and over[3].tolist() == [1, 1, 1, 1] and over[2][ref.EXCLUDED_POINTS] == 1      # +inf with an index
    bad = cases.nearest_result("nonfinite")
    q = cases.CLOUDS["nonfinite"][1]
    assert bad[2] == 37 and bad[3] == 20 and (bad[1][~np.isfinite(q).all(axis=1)] == -1).all() and np.isfinite(cases.CLOUDS["nonfinite"][0][bad[1][bad[1] >= 0]]).all()
    assert [ref.auto_cells(n) for n in (0, 1, 3, 4, 8, 15, 16, 27, 10 ** 6, 2 ** 31 - 2)] == [1, 2, 2, 2, 3, 4, 4, 5, 150, 1024]


@pytest.mark.parametrize("name", list(cases.METRICS))
def test_the_emulated_metrics_against_the_restatement(emulator, name):
    a, b = cases.METRICS[name]
    got, want = emulator.metrics(a, b), cases.metrics_result(name)
    print(name, got[8:13].tolist())
    assert same(got, want)
    # against plain float64 sums: the tree only reorders
    fa, fb = np.isfinite(a), np.isfinite(b)
    if fa.any():
        assert got[0] == fa.sum() and abs(got[ref.ACCURACY] - np.sqrt(a[fa].astype(np.float64)).mean()) < 1e-12 and got[3] == np.sqrt(a[fa].astype(np.float64)).max()
    if fa.any() and fb.any():
        assert got[ref.HAUSDORFF] == max(np.sqrt(a[fa].astype(np.float64)).max(), np.sqrt(b[fb].astype(np.float64)).max())
    else:
        assert np.isnan(got[ref.HAUSDORFF]) and (got[ref.FSCORE:ref.FSCORE + 8] == 0).all()
    assert (got[ref.PRECISION + 3:ref.RECALL] == 0).all()


def test_the_emulator_refuses_as_the_library_does(emulator):
    v, f = cases.MESHES["diagonal"]
    assert "n must be >= 1" in emulator.samples(v, f, 0, code=3)
    p, q = cases.CLOUDS["sizes_63"]
    for cell, word in ((-1.0, "cell must be finite and >= 0"), (float("nan"), "cell must be"), (float("inf"), "cell must be")):
        assert word in emulator.nearest(p, q, cell, code=3)
    a, b = cases.METRICS["one"]
    assert "nt must be 0 .. 8" in emulator.metrics(a, b, nt=9, code=3) and "a threshold is NaN" in emulator.metrics(a, b, (0.1, float("nan")), code=3)


# ---- facts that do not come from the restatement ----
@pytest.mark.parametrize("name, n", [r for r in cases.SAMPLE_RUNS if r[0] not in cases.REFUSED])
def test_samples_lie_in_their_faces_and_follow_the_weights(emulator, name, n):
    v, f = cases.MESHES[name]
    weights = ref.face_weights(v, f)[0]
    counts, points, face, bary, _ = emulator.samples(v, f, n, 0)
    error, deviation = cases.check_samples(v, f, weights, n, points, face, bary)
    print(name, n, error, deviation)
    other = emulator.samples(v, f, n, 12345)                                   # another seed: other bytes, the same bounds
    assert not same(other[1], points) and same(other[0], counts)
    cases.check_samples(v, f, weights, n, other[1], other[2], other[3])


def test_sampling_skips_and_counts_bad_faces_and_refuses_a_mesh_without_area(emulator):
    v, f = cases.MESHES["mixed"]
    counts, points, face, bary, _ = emulator.samples(v, f, 300)
    assert counts.tolist() == [0, 2, 2, 1, 0, 0, 0, 0] and set(np.unique(face).tolist()) == {0, 5} and abs(int((face == 0).sum()) - 150) < 2
    assert np.isfinite(points).all() and (points[:, 2] == 0).all()
    v, f = cases.MESHES["uneven"]
    assert (emulator.samples(v, f, 300)[2] == 0).all() and ref.face_weights(v, f)[0].tolist() == [2 ** 36 * 1000000 // 2 ** 19, 0]      # 10^6 = 1.9 * 2^19
    for name in cases.REFUSED:
        counts, points, face, bary, _ = emulator.samples(*cases.MESHES[name], 50)
        assert counts[ref.STATUS] == ref.REFUSED_EMPTY and np.isnan(points).all() and (face == -1).all() and not bary.any()
    one = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F), np.array([[0, 1, 2]], I))
    assert emulator.samples(*one, 300)[0][ref.STATUS] == 0 and ref.face_weights(*one)[0].tolist() == [2 ** 36]          # T = 2^36 carries any n below 2^31


def test_the_sphere(emulator):
    v, f = cases.MESHES["33_sphere"]
    assert len(f) == 11988 and (ref.face_weights(v, f)[0] > 0).all()
    n = 20000
    counts, points, face, bary, _ = emulator.samples(v, f, n)
    largest = cases.check_sphere_samples(points)
    area = 0.5 * ref.face_areas(v, f)[0].sum()
    want = 4 * np.pi * tsdf_cases.SPHERE.r ** 2
    print("largest | |p - c| - r |:", largest, "bound", cases.SPHERE_BOUND, "area", area, "of", want)
    assert abs(area - want) <= 0.01 * want
    analytic = cases.sphere_points(n)
    ab, ba = emulator.nearest(analytic, points), emulator.nearest(points, analytic)
    row = emulator.metrics(ab[0], ba[0])
    print("accuracy", row[ref.ACCURACY], "completeness", row[ref.COMPLETENESS], "hausdorff", row[ref.HAUSDORFF])
    assert row[ref.ACCURACY] <= cases.SPHERE_BOUND


def test_metric_facts(emulator):
    def distance(a, b, thresholds):
        ab, ba = emulator.nearest(b, a), emulator.nearest(a, b)
        out = cases.row_dict(emulator.metrics(ab[0], ba[0], thresholds), len(thresholds))
        out["index_ab"] = ab[1]
        return out

    lat = cases.check_metric_facts(distance)
    print({k: lat[k] for k in ("accuracy", "completeness", "hausdorff", "fscore")})


# ---- the refusals that need no device ----
def test_refusals_before_any_pointer_is_looked_at():
    l = G.lib()

    def refused(rc, word):
        assert rc == 1 and word in l.gp_last_error(), (word, l.gp_last_error())

    nan, inf = float("nan"), float("inf")
    for args, word in (((-1,), b">= 0"), ((2 ** 26,), b"nf must be below 2^26")):
        assert l.gp_geometry_sample_scratch_bytes(*args) == -1 and word in l.gp_last_error()
    for args, word in (((-1, 0.0), b"np must be"), ((2 ** 31 - 1, 0.0), b"np must be"), ((10, -1.0), b"cell must be"), ((10, nan), b"cell must be"), ((10, inf), b"cell must be")):
        assert l.gp_geometry_grid_scratch_bytes(*args) == -1 and word in l.gp_last_error()
    for args in ((-1, 5), (5, 2 ** 31)):
        assert l.gp_geometry_metrics_scratch_bytes(*args) == -1 and b"2^31 - 1" in l.gp_last_error()
    assert l.gp_geometry_sample_scratch_bytes(0) > 0 and l.gp_geometry_sample_scratch_bytes(10 ** 6) >= 8 * 10 ** 6
    assert l.gp_geometry_grid_scratch_bytes(10 ** 6, 0.0) >= 16 * 10 ** 6 + 8 * 10 ** 6 and l.gp_geometry_grid_scratch_bytes(10, 0.5) >= 8 * 2 ** 24
    assert l.gp_geometry_metrics_scratch_bytes(0, 0) > 0

    def sample(vertices=16, faces=16, nv=4, nf=2, n=10, seed=0, scratch=16, points=16, face=16, bary=16, counts=16):
        return l.gp_geometry_sample(vertices, faces, nv, nf, n, seed, scratch, points, face, bary, counts, None)

    for kw, word in ((dict(nv=-1), b">= 0"), (dict(nv=2 ** 31), b"nv must be below 2^31"), (dict(nf=2 ** 26), b"nf must be below 2^26"), (dict(n=0), b"n must be >= 1"),
                     (dict(n=2 ** 31), b"2^31 - 1"), (dict(scratch=None), b"null"), (dict(scratch=8), b"16-byte aligned"), (dict(points=None), b"null"), (dict(face=None), b"null"),
                     (dict(bary=None), b"null"), (dict(counts=None), b"null"), (dict(vertices=None), b"null"), (dict(faces=None), b"null")):
        refused(sample(**kw), word)
    for args, word in (((16, 0, 16, 4, 2, 16, 16, 10, 16), b"C must be 1 .. 8"), ((16, 9, 16, 4, 2, 16, 16, 10, 16), b"C must be 1 .. 8"), ((None, 3, 16, 4, 2, 16, 16, 10, 16), b"null"),
                       ((16, 3, None, 4, 2, 16, 16, 10, 16), b"null"), ((16, 3, 16, 4, 2, None, 16, 10, 16), b"null"), ((16, 3, 16, 4, 2, 16, None, 10, 16), b"null"),
                       ((16, 3, 16, 4, 2, 16, 16, 10, None), b"null"), ((16, 3, 16, 4, 2 ** 26, 16, 16, 10, 16), b"2^26"), ((16, 3, 16, 4, 2, 16, 16, -1, 16), b"2^31 - 1")):
        refused(l.gp_geometry_interpolate(*args, None), word)
    for args, word in (((16, -1, 0.0, 16), b"np must be"), ((16, 10, -1.0, 16), b"cell must be"), ((16, 10, nan, 16), b"cell must be"), ((16, 10, 0.0, None), b"null"),
                       ((16, 10, 0.0, 24), b"16-byte aligned"), ((None, 10, 0.0, 16), b"null")):
        refused(l.gp_geometry_grid_build(*args, None), word)
    for args, word in (((16, 5, 16, -1, 0.0, 16, 16, 16), b"np must be"), ((16, 2 ** 31, 16, 10, 0.0, 16, 16, 16), b"2^31 - 1"), ((16, 5, 16, 10, inf, 16, 16, 16), b"cell must be"),
                       ((16, 5, None, 10, 0.0, 16, 16, 16), b"null"), ((16, 5, 8, 10, 0.0, 16, 16, 16), b"aligned"), ((None, 5, 16, 10, 0.0, 16, 16, 16), b"null"),
                       ((16, 5, 16, 10, 0.0, None, 16, 16), b"null"), ((16, 5, 16, 10, 0.0, 16, None, 16), b"null"), ((16, 5, 16, 10, 0.0, 16, 16, None), b"null")):
        refused(l.gp_geometry_grid_query(*args, None), word)
    th = (C.c_float * 2)(0.1, nan)
    for args, word in (((16, -1, 16, 5, th, 1, 16, 16), b"2^31 - 1"), ((16, 5, 16, 5, th, 9, 16, 16), b"nt must be 0 .. 8"), ((16, 5, 16, 5, th, -1, 16, 16), b"nt must be"),
                       ((16, 5, 16, 5, th, 1, None, 16), b"null"), ((16, 5, 16, 5, th, 1, 8, 16), b"aligned"), ((16, 5, 16, 5, th, 1, 16, None), b"null"),
                       ((None, 5, 16, 5, th, 1, 16, 16), b"null"), ((16, 5, None, 5, th, 1, 16, 16), b"null"), ((16, 5, 16, 5, None, 1, 16, 16), b"null"),
                       ((16, 5, 16, 5, th, 2, 16, 16), b"a threshold is NaN")):
        refused(l.gp_geometry_metrics(*args, None), word)


def test_the_python_surface_refuses_before_the_device(monkeypatch, tmp_path):
    monkeypatch.setattr(G, "lib", lambda: pytest.fail("a launch was reached"))
    faces, vertices, cloud = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, 3), torch.zeros(5, 3)
    for call in (lambda: G.sample_surface((vertices, faces), 10), lambda: G.nearest(cloud, cloud), lambda: G.NearestGrid(cloud), lambda: G.cloud_distance(cloud, cloud),
                 lambda: G.mesh_distance((vertices, faces), (vertices, faces), n=10), lambda: G.metrics_table(cloud[:, 0], cloud[:, 0])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for call, word in ((lambda: G.sample_surface((vertices, faces.long()), 10), "int32"), (lambda: G.sample_surface((vertices[0], faces), 10), r"\[Nv, 3\]"),
                       (lambda: G.nearest(cloud, cloud.double()), r"\[N, 3\] float32"), (lambda: G.nearest(cloud, cloud[:, :2]), r"\[N, 3\] float32"),
                       (lambda: G.interpolate(None, (vertices, faces), vertices), "SurfaceSamples"), (lambda: G.metrics_table(cloud, cloud), r"\[n\] float32")):
        with pytest.raises(RuntimeError, match=word):
            call()
    for call, word in ((lambda: G.sample_surface((vertices, faces), 0), "n must be 1"), (lambda: G.sample_surface((vertices, faces), 2 ** 31), "n must be 1"),
                       (lambda: G.sample_surface((vertices, faces), 5, seed=-1), "seed"), (lambda: G.NearestGrid(cloud, cell=-1.0), "cell must be finite and >= 0"),
                       (lambda: G.NearestGrid(cloud, cell=float("nan")), "cell must be"), (lambda: G.cloud_distance(cloud, cloud, thresholds=range(9)), "nt must be 0 .. 8"),
                       (lambda: G.cloud_distance(cloud, cloud, thresholds=(float("nan"),)), "a threshold is NaN"), (lambda: G.mesh_distance(None, None, thresholds=range(9)), "nt must be")):
        with pytest.raises(_lib.GpHipError, match=word):
            call()
    assert G.check_cell(None) is None and G.check_cell(0.5) is None and "cell" in G.check_cell(float("inf")) and G.check_thresholds((0.1, 0.2)) is None
    (tmp_path / "a").mkdir(), (tmp_path / "b").mkdir()
    with pytest.raises(RuntimeError, match="no %05d.ply name is in both"):
        G.evaluate_mesh_dirs(str(tmp_path / "a"), str(tmp_path / "b"))


def test_signatures_and_docstrings():
    from gaussianprediction_amd import eval_render as ER
    sig = inspect.signature(G.sample_surface)
    assert list(sig.parameters) == ["mesh", "n", "seed"] and sig.parameters["seed"].default == 0
    assert list(inspect.signature(G.interpolate).parameters) == ["samples", "mesh", "attributes"]
    assert list(inspect.signature(G.nearest).parameters) == ["queries", "points", "cell"] and inspect.signature(G.nearest).parameters["cell"].default is None
    assert list(inspect.signature(G.NearestGrid.__init__).parameters) == ["self", "points", "cell"] and list(inspect.signature(G.NearestGrid.query).parameters) == ["self", "queries"]
    assert list(inspect.signature(G.cloud_distance).parameters)[:3] == ["a", "b", "thresholds"]
    sig = inspect.signature(G.mesh_distance)
    assert list(sig.parameters)[:5] == ["mesh_a", "mesh_b", "n", "seed", "thresholds"] and sig.parameters["seed"].default == 0
    sig = inspect.signature(G.evaluate_mesh_dirs)
    assert list(sig.parameters)[:5] == ["pred_dir", "gt_dir", "n", "thresholds", "seed"] and sig.parameters["seed"].default == 0
    assert list(inspect.signature(ER.mesh_motion).parameters)[:3] == ["meshes", "n", "thresholds"]
    assert open(ER.__file__).read().count("render_meshes(") == 1            # render_meshes itself is left alone
    assert "ONE read" in G.SurfaceSamples.__doc__ and "Nothing is read" in G.sample_surface.__doc__ and "ONE read" in G.cloud_distance.__doc__ and "ONE read" in G.mesh_distance.__doc__
    assert "the only read" in G.Nearest.__doc__ and "Nothing is read" in G.NearestGrid.query.__doc__
    rows = [{"accuracy": 1.0, "fscore": [0.5, 1.0], "thresholds": [1, 2], "name": "a"}, {"accuracy": 3.0, "fscore": [0.0, 0.5], "thresholds": [1, 2], "name": "b"}]
    assert G.mean_row(rows) == {"accuracy": 2.0, "fscore": [0.25, 0.75], "thresholds": [1, 2]} and G.mean_row([]) == {}
