"""No GPU: csrc/gp_surface.h against the binding's table (a binding outside _lib.ABIS); the programs of csrc/surface_core.h in a
stand-alone build (tests/surface_emulate.cpp, under the sanitizers where the host compiler can link them) against the numpy
restatement tests/surface_ref.py on every case of tests/surface_cases.py, under every cell rule and both W -- bit for bit, all five
outputs; facts that do not come from the restatement (the regions of one triangle, the degenerate faces, the ties, a permutation of
the faces, an independent Ericson region walk); the refusals that need no device; the new trailing keywords."""
import inspect
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import abi_check
import surface_cases as cases
import surface_ref as ref
from gaussianprediction_amd import _lib, geometry_ops as G, surface_ops as S

_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "gp_stream_t": _lib.Ptr}
_POINTEES = {"float", "int32_t", "int64_t", "void"}
F = np.float32
I = np.int32
same = cases.same


# ---- the header, the table, the registry ----
def test_prototype_table_equals_the_header_and_stays_out_of_the_registry():
    before = len(_lib.ABIS)
    protos = abi_check.check_table(S.ABI, 5, _SCALARS, _POINTEES)
    assert S.ABI.prototypes is S.PROTOTYPES and S.ABI not in _lib.ABIS and G.ABI not in _lib.ABIS and len(_lib.ABIS) == before
    assert os.path.samefile(os.path.join(abi_check.ROOT, "include", S.ABI.header), os.path.join(abi_check.ROOT, "gaussianprediction_amd", "csrc", "gp_surface.h"))
    for name in ("gp_surface_grid_count", "gp_surface_grid_fill", "gp_surface_grid_query"):
        assert protos[name][1][-1] == "gp_stream_t"              # the stream is the last parameter
    assert not os.path.exists(os.path.join(abi_check.ROOT, "include", "gp_surface.h"))
    assert len([h for h in os.listdir(os.path.join(abi_check.ROOT, "include")) if h.endswith(".h")]) == 12      # include/ stays at its twelve


def test_symbols_and_constants():
    text = abi_check.header_text(S.HEADER)
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_SURFACE_[A-Z0-9_]+) +(\d+)", text)}
    assert defs["GP_SURFACE_ABI_VERSION"] == S.GP_SURFACE_ABI_VERSION == S.ABI.version == 1
    for name in ("WIDE_CELLS", "MAX_WIDE_CELLS", "STAT_WORDS", "REFUSED_CAPACITY"):
        assert defs["GP_SURFACE_" + name] == getattr(S, name) == getattr(ref, name), name
    assert [defs["GP_SURFACE_" + n.upper()] for n in S.STAT_NAMES] == list(range(11)) == [getattr(ref, n.upper()) for n in S.STAT_NAMES]
    assert S.MAX_WIDE_CELLS * (G.MAX_FACES - 1) < 2 ** 32 and S.WIDE_CELLS <= S.MAX_WIDE_CELLS          # the pairs fit 32 bits
    geometry = {k: int(v) for k, v in re.findall(r"#define (GP_GEOMETRY_[A-Z0-9_]+) +(\d+)", abi_check.header_text(G.HEADER))}
    assert geometry["GP_GEOMETRY_ABI_VERSION"] == 1 and G.ABI.version == 1                               # gp_geometry.h is as it was
    raw = open(os.path.join(abi_check.ROOT, "include", S.HEADER)).read()
    for words in ("Why (b) is exact", "2^-48 * M_k", "the margin does not change", "dot(x, y) = (x_0*y_0 + x_1*y_1) + x_2*y_2"):
        assert words in raw, words                                # the definition's order and the proof stand in the header
    abi_check.check_applied(S.ABI)
    assert [ref.auto_cells(n) for n in (0, 1, 35, 36, 99, 100, 10 ** 4, 11988, 70692, 1780644, 2 ** 26 - 1)] == [1, 1, 1, 2, 2, 3, 25, 27, 66, 334, 1024]


# ---- the programs in a stand-alone build, under the sanitizers ----
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return cases.build_emulator(tmp_path_factory.mktemp("surface_emulate"), sanitize=True)


def test_the_emulator_is_its_own_program():
    text = open(os.path.join(abi_check.ROOT, "tests", "surface_emulate.cpp")).read()
    assert '#include "../gaussianprediction_amd/csrc/surface_core.h"' in text and "int main(int argc" in text
    driver = inspect.getsource(cases.build_emulator)
    assert 'emulate_build.build("surface_emulate"' in driver and "subprocess.run([exe" in driver          # a child process: nothing is loaded into Python
    assert "sanitize=True" in inspect.getsource(emulator)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_emulated_grid_against_the_restatement_under_every_rule_and_w(emulator, name):
    v, f, q = cases.CASES[name]
    want = cases.result(name)
    seen = {}
    for rule in cases.RULES:
        for wide in cases.WIDE:
            got = emulator.query(v, f, q, cases.cell_of(name, rule), wide)
            print(name, rule, wide, got[5].tolist(), got[6].tolist())
            assert all(cases.equal_result(got[:5], want)), (name, rule, wide, cases.equal_result(got[:5], want))
            stats, dims = got[5], got[6]
            assert stats[ref.EXCLUDED_FACES] == want.excluded_faces and stats[ref.EXCLUDED_QUERIES] == want.excluded_queries and stats[ref.STATUS] == 0
            assert dims[3] == dims[:3].prod() <= G.MAX_CELLS and dims[:3].max() <= G.MAX_AXIS and stats[ref.DIM_X:ref.DIM_Z + 1].tolist() == dims[:3].tolist()
            assert stats[ref.PAIRS] <= wide * (len(f) - stats[ref.EXCLUDED_FACES] - stats[ref.WIDE])
            if rule == "1":
                assert dims.tolist() == [1, 1, 1, 1] and stats[ref.WIDE] == 0 and stats[ref.PAIRS] == len(f) - want.excluded_faces      # the brute force
            seen[rule, wide] = got
    back = emulator.query(v, f, q, cases.cell_of(name, "7"), ref.WIDE_CELLS, backwards=True)          # another order inside the cells: equal bytes
    assert all(same(g, b) for g, b in zip(seen["7", ref.WIDE_CELLS], back))
    back = emulator.query(v, f, q, cases.cell_of(name, "7"), 1, backwards=True)                       # and inside the wide list
    assert all(same(g, b) for g, b in zip(seen["7", 1], back))


def test_the_cases_reach_what_they_are_for(emulator):
    run = lambda name, rule, wide=ref.WIDE_CELLS: emulator.query(*cases.CASES[name], cases.cell_of(name, rule), wide)          # noqa: E731
    t = cases.result("triangle")
    assert t.region[:7].tolist() == [0, 1, 2, 3, 1, 1, 2] and t.dist2[:7].tolist() == [1.0, 1.25, 2.0625, 1.0625, 2.25, 1.265625, 1.25]      # the seven regions
    assert t.bary[4].tolist() == [0.0, 0.0] and t.bary[5].tolist() == [1.0, 0.0] and t.bary[6].tolist() == [0.0, 1.0]      # the corners, seen from outside
    assert (t.dist2[7:14] == 0).all() and t.region[7:14].tolist() == [0, 0, 0, 0, 0, 0, 0] and same(t.closest[7:14], cases.CASES["triangle"][2][7:14])      # on the triangle itself
    assert set(np.unique(t.region).tolist()) == {0, 1, 2, 3}
    p = cases.result("point_face")
    assert p.dist2[0] == 1.0 and p.dist2[1] == 0.0 and (p.region == 1).all() and (p.closest == F([1, 2, 3])).all() and (p.bary == 0).all()
    s = cases.result("segment_face")
    assert s.dist2[:4].tolist() == [1.0, 1.0, 1.0, 1.0] and (s.region != 0).all() and s.closest[0].tolist() == [2.0, 0.0, 0.0]
    m = cases.result("mixed")
    assert m.excluded_faces == 4 and set(np.unique(m.face).tolist()) <= {0, 4} and m.face[1] == 4 and m.dist2[1] == 0.25 and m.face[0] == 0      # face 5 repeats face 0 and never wins
    none = run("no_faces", "auto")
    assert np.isinf(none[0]).all() and (none[1] == -1).all() and (none[2] == 0).all() and np.isnan(none[3]).all() and not none[4].any() and none[5][ref.CANDIDATES] == 0
    i = cases.result("identical")
    assert (i.face == 0).all() and len(i.ties) == len(i.face) and all(t.tolist() == [0, 1, 2] for t in i.ties.values())
    e = cases.result("shared_edge")
    assert e.face[:4].tolist() == [0, 0, 0, 0] and all(e.ties[k].tolist() == [0, 1] for k in range(4)) and e.dist2[:4].tolist() == [0.0, 0.0, 1.0, 4.0]
    mid = cases.result("mid_plane")
    assert mid.face[:2].tolist() == [0, 0] and mid.ties[0].tolist() == [0, 1] and mid.dist2[:2].tolist() == [1.0, 1.0] and mid.region[:2].tolist() == [0, 0]
    u = run("uneven", "auto")
    assert u[5][ref.WIDE] == 0 and u[6].tolist() == [1, 1, 1, 1]                                  # two faces: one cell
    u = run("uneven", "1024")
    assert u[5][ref.WIDE] == 1 and u[5][ref.PAIRS] >= 1 and set(np.unique(u[1]).tolist()) == {0, 1}      # the large face is wide, the small one sits in its cells
    h = run("hub", "1024")
    assert h[5][ref.WIDE] > 1900                                                                  # long thin faces: nearly every box holds more than 64 cells
    h = run("hub", "7")
    assert h[6].tolist()[:2] == [7, 7] and h[5][ref.WIDE] == 0 and h[5][ref.PAIRS] > 4 * 2000 and h[5][ref.CANDIDATES] >= 2000 * 3      # the hub's cells hold every face
    far = run("far_origin", "1024")
    assert np.spacing(F(1e6)) > cases.cell_of("far_origin", "1024")                               # a cell is smaller than an ulp
    for name in ("33_sphere", "33_torus"):
        assert run(name, "1024")[5][ref.SWEPT] >= 8                                               # the queries far away end with the pass over all records
        got = run(name, "auto")
        assert got[5][ref.EXCLUDED_QUERIES] == 8 and got[5][ref.MAX_RING] >= 2 and got[6][:3].max() == ref.auto_cells(len(cases.CASES[name][1])) == 27
        assert got[5][ref.CANDIDATES] < len(got[0]) * len(cases.CASES[name][1]) // 2               # under half a brute force, the cube's far queries included
        bad = ~np.isfinite(cases.CASES[name][2]).all(axis=1)
        assert bad.sum() == 8 and np.isinf(got[0][bad]).all() and (got[1][bad] == -1).all()
        assert run(name, "auto", 1)[5][ref.WIDE] > 0.5 * len(cases.CASES[name][1])                 # W = 1: the wide path sees most faces
        assert run(name, "1024", 1)[5][ref.WIDE] > 0.9 * len(cases.CASES[name][1]) and run(name, "2")[5][ref.WIDE] == 0      # ... nearly all of them; and none


@pytest.mark.parametrize("name", list(cases.CASES))
def test_a_permutation_of_the_faces(emulator, name):
    """dist2 never depends on the order of the faces; where one face alone wins, closest, region and bary are equal to the byte and the
    face maps through the permutation; where several tie, the smaller NEW number wins."""
    v, f, q = cases.CASES[name]
    want = cases.result(name)
    perm = np.random.default_rng(7).permutation(len(f))
    new_number = np.empty(len(f), np.int64)
    new_number[perm] = np.arange(len(f))
    got = emulator.query(v, f[perm], q, cases.cell_of(name, "auto"))
    assert same(got[0], want.dist2)
    tied = np.zeros(len(q), bool)
    tied[list(want.ties)] = True
    alone = ~tied & (want.face >= 0)
    assert (got[1][alone] == new_number[want.face[alone]]).all() and same(got[2][alone], want.region[alone]) and same(got[3][alone], want.closest[alone])
    assert same(got[4][alone], want.bary[alone])
    for k, faces in want.ties.items():
        assert got[1][k] == new_number[faces].min(), (name, k)
    assert (got[1][want.face < 0] == -1).all()
    print(name, "rows won alone:", int(alone.sum()), "tied:", int(tied.sum()))


def ericson(p, a, b, c):
    """Ericson's closest point on a triangle (Real-Time Collision Detection 5.1.5), the region walk, row by row in float64."""
    out = np.empty_like(p)
    for i in range(len(p)):
        P, A, B, Cc = p[i], a[i], b[i], c[i]
        ab, ac, ap = B - A, Cc - A, P - A
        d1, d2 = ab @ ap, ac @ ap
        if d1 <= 0 and d2 <= 0:
            out[i] = A
            continue
        bp = P - B
        d3, d4 = ab @ bp, ac @ bp
        if d3 >= 0 and d4 <= d3:
            out[i] = B
            continue
        vc = d1 * d4 - d3 * d2
        if vc <= 0 and d1 >= 0 and d3 <= 0:
            out[i] = A + ab * (d1 / (d1 - d3))
            continue
        cp = P - Cc
        d5, d6 = ab @ cp, ac @ cp
        if d6 >= 0 and d5 <= d6:
            out[i] = Cc
            continue
        vb = d5 * d2 - d1 * d6
        if vb <= 0 and d2 >= 0 and d6 <= 0:
            out[i] = A + ac * (d2 / (d2 - d6))
            continue
        va = d3 * d6 - d5 * d4
        if va <= 0 and (d4 - d3) >= 0 and (d5 - d6) >= 0:
            out[i] = B + (Cc - B) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))
            continue
        denom = 1.0 / (va + vb + vc)
        out[i] = A + ab * (vb * denom) + ac * (vc * denom)
    return out


def test_the_definition_against_ericsons_region_walk():
    rng = np.random.default_rng(11)
    n = 20000
    p, a, b, c = (rng.normal(size=(n, 3)).astype(F).astype(np.float64) for _ in range(4))
    d, region, closest, u1, u2 = ref.face_candidates(p, a, b, c)
    other = ericson(p, a, b, c)
    d_other = ((p - other) ** 2).sum(axis=1)
    error = np.abs(d - d_other) / d_other
    print("largest relative difference of the squared distance:", error.max(), "regions", np.bincount(region, minlength=4).tolist())
    assert error.max() <= 1e-12 and (np.bincount(region, minlength=4) > 1000).all()
    again = a + (b - a) * u1[:, None] + (c - a) * u2[:, None]                       # the barycentrics name the closest point
    assert np.abs(again - closest).max() <= 1e-14 * 16 and (u1 >= 0).all() and (u2 >= 0).all() and (u1 + u2 <= 1 + 1e-15).all()


def test_the_emulator_refuses_as_the_library_does(emulator):
    v, f, q = cases.CASES["sizes_63"]
    for cell, word in ((-1.0, "cell must be finite and >= 0"), (float("nan"), "cell must be"), (float("inf"), "cell must be")):
        assert word in emulator.query(v, f, q, cell, code=3)
    for wide in (0, 65, -1):
        assert "wide_cells must be 1 .. 64" in emulator.query(v, f, q, 0.0, wide, code=3)
    assert "nf must be below 2^26" in emulator.query(v, f, q, sizes=(len(v), 2 ** 26, len(q)), code=3)
    for name, rule in (("sizes_63", "7"), ("hub", "auto"), ("33_torus", "auto")):          # one pair too few: refused by status, nothing written (the pair array is exact)
        v, f, q = cases.CASES[name]
        got = emulator.query(v, f, q, cases.cell_of(name, rule), short_by=1)
        assert got[5][ref.STATUS] == ref.REFUSED_CAPACITY and got[5][ref.PAIRS] > 0 and got[5][ref.CANDIDATES] == 0
        assert np.isinf(got[0]).all() and (got[1] == -1).all() and np.isnan(got[3]).all()


# ---- the refusals that need no device ----
def test_refusals_before_any_pointer_is_looked_at():
    l = S.lib()

    def refused(rc, word):
        assert rc == 1 and word in l.gp_last_error(), (word, l.gp_last_error())

    nan, inf = float("nan"), float("inf")
    for args, word in (((-1, 0.0), b">= 0"), ((2 ** 26, 0.0), b"nf must be below 2^26"), ((10, -1.0), b"cell must be"), ((10, nan), b"cell must be"), ((10, inf), b"cell must be")):
        assert l.gp_surface_scratch_bytes(*args) == -1 and word in l.gp_last_error()
    assert l.gp_surface_scratch_bytes(0, 0.0) > 0 and l.gp_surface_scratch_bytes(10 ** 6, 0.0) >= 52 * 10 ** 6 + 8 * 250 ** 3 and l.gp_surface_scratch_bytes(10, 0.5) >= 8 * 2 ** 24
    assert l.gp_surface_scratch_bytes(100, 0.0) < 2 ** 16

    def count(vertices=16, faces=16, nv=4, nf=2, cell=0.0, wide=64, scratch=16, sizes=16):
        return l.gp_surface_grid_count(vertices, faces, nv, nf, cell, wide, scratch, sizes, None)

    for kw, word in ((dict(nv=-1), b">= 0"), (dict(nv=2 ** 31), b"nv must be below 2^31"), (dict(nf=2 ** 26), b"nf must be below 2^26"), (dict(cell=-1.0), b"cell must be"),
                     (dict(cell=nan), b"cell must be"), (dict(wide=0), b"wide_cells must be 1 .. 64"), (dict(wide=65), b"wide_cells must be"), (dict(scratch=None), b"null"),
                     (dict(scratch=8), b"16-byte aligned"), (dict(sizes=None), b"null"), (dict(vertices=None), b"null"), (dict(faces=None), b"null")):
        refused(count(**kw), word)

    def fill(nf=2, cell=0.0, wide=64, scratch=16, pairs=16, capacity=10):
        return l.gp_surface_grid_fill(nf, cell, wide, scratch, pairs, capacity, None)

    for kw, word in ((dict(nf=-1), b">= 0"), (dict(nf=2 ** 26), b"2^26"), (dict(cell=inf), b"cell must be"), (dict(wide=0), b"wide_cells"), (dict(capacity=-1), b"pair_capacity must be"),
                     (dict(capacity=2 ** 32), b"pair_capacity must be"), (dict(scratch=None), b"null"), (dict(scratch=24), b"16-byte aligned"), (dict(pairs=None), b"null")):
        refused(fill(**kw), word)

    def query(queries=16, nq=5, scratch=16, pairs=16, nf=2, cell=0.0, dist2=16, face=16, region=16, closest=16, bary=16, stats=16):
        return l.gp_surface_grid_query(queries, nq, scratch, pairs, nf, cell, dist2, face, region, closest, bary, stats, None)

    for kw, word in ((dict(nf=2 ** 26), b"2^26"), (dict(nq=-1), b"2^31 - 1"), (dict(nq=2 ** 31), b"2^31 - 1"), (dict(cell=-0.5), b"cell must be"), (dict(scratch=None), b"null"),
                     (dict(scratch=8), b"aligned"), (dict(queries=None), b"null"), (dict(dist2=None), b"null"), (dict(face=None), b"null"), (dict(region=None), b"null"),
                     (dict(closest=None), b"null"), (dict(bary=None), b"null"), (dict(stats=None), b"null")):
        refused(query(**kw), word)


def test_the_python_surface_refuses_before_the_device(monkeypatch):
    monkeypatch.setattr(S, "lib", lambda: pytest.fail("a launch was reached"))
    monkeypatch.setattr(G, "lib", lambda: pytest.fail("a launch was reached"))
    faces, vertices, cloud = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, 3), torch.zeros(5, 3)
    mesh = (vertices, faces)
    for call in (lambda: S.SurfaceGrid(mesh), lambda: S.point_mesh_distance(cloud, mesh), lambda: S.surface_distance(mesh, mesh, n=10), lambda: G.mesh_distance(mesh, mesh, n=10, surface=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for call, word in ((lambda: S.SurfaceGrid((vertices, faces.long())), "int32"), (lambda: S.SurfaceGrid((vertices[0], faces)), r"\[Nv, 3\]"),
                       (lambda: G.interpolate(None, mesh, vertices), "SurfaceSamples"), (lambda: G.interpolate(object(), mesh, vertices), "PointSurface")):
        with pytest.raises(RuntimeError, match=word):
            call()
    for call, word in ((lambda: S.SurfaceGrid(mesh, cell=-1.0), "cell must be finite and >= 0"), (lambda: S.SurfaceGrid(mesh, cell=float("nan")), "cell must be"),
                       (lambda: S.SurfaceGrid(mesh, wide_cells=0), "wide_cells must be 1 .. 64"), (lambda: S.SurfaceGrid(mesh, wide_cells=65), "wide_cells must be"),
                       (lambda: S.point_mesh_distance(cloud, mesh, cell=float("inf")), "cell must be"), (lambda: S.surface_distance(None, None, thresholds=range(9)), "nt must be 0 .. 8"),
                       (lambda: S.surface_distance(None, None, thresholds=(float("nan"),)), "a threshold is NaN"),
                       (lambda: G.mesh_distance(None, None, thresholds=range(9), surface=True), "nt must be")):
        with pytest.raises(_lib.GpHipError, match=word):
            call()


def test_signatures_keywords_and_docstrings():
    from gaussianprediction_amd import eval_render as ER
    assert list(inspect.signature(S.SurfaceGrid.__init__).parameters) == ["self", "mesh", "cell", "wide_cells"] and inspect.signature(S.SurfaceGrid.__init__).parameters["cell"].default is None
    assert inspect.signature(S.SurfaceGrid.__init__).parameters["wide_cells"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(S.SurfaceGrid.query).parameters) == ["self", "queries"] and list(inspect.signature(S.point_mesh_distance).parameters) == ["queries", "mesh", "cell"]
    sig = inspect.signature(S.surface_distance)
    assert list(sig.parameters) == ["mesh_a", "mesh_b", "n", "seed", "thresholds", "cell"] and [p.default for p in sig.parameters.values()][2:] == [100000, 0, G.THRESHOLDS, None]
    # the trailing keyword, and everything before it as it was
    sig = inspect.signature(G.mesh_distance)
    assert list(sig.parameters) == ["mesh_a", "mesh_b", "n", "seed", "thresholds", "cell", "surface"] and sig.parameters["surface"].default is False
    assert [p.default for p in sig.parameters.values()][2:6] == [100000, 0, G.THRESHOLDS, None]
    sig = inspect.signature(G.evaluate_mesh_dirs)
    assert list(sig.parameters) == ["pred_dir", "gt_dir", "n", "thresholds", "seed", "device", "surface"] and sig.parameters["surface"].default is False
    assert [p.default for p in sig.parameters.values()][2:6] == [100000, G.THRESHOLDS, 0, "cuda"]
    sig = inspect.signature(ER.mesh_motion)
    assert list(sig.parameters) == ["meshes", "n", "thresholds", "seed", "device", "surface"] and sig.parameters["surface"].default is False
    assert [p.default for p in sig.parameters.values()][1:5] == [100000, None, 0, "cuda"]
    assert open(ER.__file__).read().count("render_meshes(") == 1
    assert "ONE 16-byte read" in S.SurfaceGrid.__doc__ and "Nothing is read" in S.SurfaceGrid.query.__doc__ and "the only read" in S.PointSurface.__doc__
    assert "ONE read" in S.surface_distance.__doc__ and "16-byte sizing reads" in S.surface_distance.__doc__ and "ONE 16-byte" in S.point_mesh_distance.__doc__
    assert "ONE read" in G.mesh_distance.__doc__ and "surface=True" in G.mesh_distance.__doc__ and "surface=True" in ER.mesh_motion.__doc__
    rows = [{"accuracy": 1.0, "surface": True, "n": 5}, {"accuracy": 3.0, "surface": True, "n": 5}]
    assert G.mean_row(rows) == {"accuracy": 2.0, "surface": True, "n": 5}
    assert S.STAT_NAMES == ("excluded_faces", "excluded_queries", "candidates", "max_ring", "dim_x", "dim_y", "dim_z", "swept", "pairs", "wide", "status")
