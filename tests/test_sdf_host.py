"""No GPU: csrc/gp_sdf.h against the binding's table (a binding outside _lib.ABIS); the programs of csrc/sdf_core.h in a stand-alone
build (tests/sdf_emulate.cpp, under the sanitizers where the host compiler can link them) against the numpy restatement
tests/sdf_ref.py on every case of tests/sdf_cases.py; facts that do not come from the restatement (the winding number, the cube's
corners and centres, the flipped cube, the cancelling edge, foreign input); the refusals that need no device; the untouched defaults
of the functions that learnt the signed row."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import abi_check
import sdf_cases as cases
import sdf_ref as ref
from gaussianprediction_amd import _lib, geometry_ops as G, mesh_smooth as MS, sdf_ops as D, surface_ops as S

_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "gp_stream_t": _lib.Ptr}
_POINTEES = {"float", "double", "int8_t", "int32_t", "int64_t", "void"}
F = np.float32
I = np.int32
same = cases.same


# ---- the header, the table, the registry ----
def test_prototype_table_equals_the_header_and_stays_out_of_the_registry():
    before = len(_lib.ABIS)
    protos = abi_check.check_table(D.ABI, 6, _SCALARS, _POINTEES)
    assert D.ABI.prototypes is D.PROTOTYPES and D.ABI not in _lib.ABIS and S.ABI not in _lib.ABIS and MS.ABI not in _lib.ABIS and len(_lib.ABIS) == before
    assert os.path.samefile(os.path.join(abi_check.ROOT, "include", D.ABI.header), os.path.join(abi_check.ROOT, "gaussianprediction_amd", "csrc", "gp_sdf.h"))
    for name in ("gp_sdf_tables", "gp_sdf_sign", "gp_sdf_means"):
        assert protos[name][1][-1] == "gp_stream_t"              # the stream is the last parameter
    assert not os.path.exists(os.path.join(abi_check.ROOT, "include", "gp_sdf.h"))
    assert len([h for h in os.listdir(os.path.join(abi_check.ROOT, "include")) if h.endswith(".h")]) == 12      # include/ stays at its twelve


def test_symbols_and_constants():
    text = abi_check.header_text(D.HEADER)
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_SDF_[A-Z0-9_]+) +(\d+)", text)}
    assert defs["GP_SDF_ABI_VERSION"] == D.GP_SDF_ABI_VERSION == D.ABI.version == 1
    for name in ("COUNT_WORDS", "STAT_WORDS", "MEAN_WORDS"):
        assert defs["GP_SDF_" + name] == getattr(D, name) == getattr(ref, name), name
    assert [defs["GP_SDF_" + n.upper()] for n in D.STAT_NAMES] == list(range(8)) and D.STAT_NAMES == ref.STAT_NAMES
    assert [defs["GP_SDF_COUNT_" + n.upper()] for n in D.COUNT_NAMES] == list(range(4)) and D.COUNT_NAMES == ref.COUNT_NAMES
    assert [defs["GP_SDF_KIND_" + n] for n in ("FACE", "EDGE", "VERTEX")] == [D.KIND_FACE, D.KIND_EDGE, D.KIND_VERTEX] == [0, 1, 2]
    raw = open(os.path.join(abi_check.ROOT, "include", D.HEADER)).read()
    for words in ("angle = atan2(sqrt(dot(x, x)), dot(e1, e2))", "(face number, side number), starting from +0.0","for d = 128, 64, ..., 1", "Foreign input", "tau = 1"):
        assert words in raw, words                                # the definitions and their order stand in the header
    abi_check.check_applied(D.ABI)
    source = open(os.path.join(abi_check.ROOT, "gaussianprediction_amd", "csrc", "sdf_kernels.hip")).read()
    assert '#include "sdf_core.h"' in source and "atomicAdd(" in source and "double* word" not in source
    core = open(os.path.join(abi_check.ROOT, "gaussianprediction_amd", "csrc", "sdf_core.h")).read()
    assert '#include "surface_core.h"' in core and "sf_interior(" in core and "sf_edge(" in core          # the candidate again: surface_core.h's own functions
    import __graft_entry__ as entry
    assert "sdf_kernels.hip" in entry.HIP_SOURCES and "-ffp-contract=off" in entry.HIP_FLAGS


# ---- the programs in a stand-alone build, under the sanitizers ----
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return cases.build_emulator(tmp_path_factory.mktemp("sdf_emulate"), sanitize=True)


def emulate(emulator, name):
    v, f, q = cases.CASES[name]
    want = cases.result(name)
    return emulator.run(v, f, want.topology.edge, q, want.surface.dist2, want.surface.face, want.surface.region)


def test_the_emulator_is_its_own_program():
    text = open(os.path.join(abi_check.ROOT, "tests", "sdf_emulate.cpp")).read()
    assert '#include "../gaussianprediction_amd/csrc/sdf_core.h"' in text and "int main(int argc" in text
    driver = inspect.getsource(cases.build_emulator)
    assert 'emulate_build.build("sdf_emulate"' in driver and "subprocess.run([exe" in driver          # a child process: nothing is loaded into Python
    assert "sanitize=True" in inspect.getsource(emulator)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_emulated_programs_against_the_restatement(emulator, name):
    got = emulate(emulator, name)
    cases.compare(name, got)


def test_the_cases_reach_what_they_are_for(emulator):
    r = cases.result
    for name in cases.CASES:
        s = r(name).signed
        print(name, dict(zip(ref.STAT_NAMES, s.stats.tolist())), "volume", float(r(name).tables.volume), "counts", r(name).tables.counts.tolist())
    # the cube: corners outside and nearest to a vertex, centres inside; the flipped cube inverts every sign and the volume
    cube, flipped = r("cube"), r("cube_flipped")
    assert (cube.signed.sign[:8] == 1).all() and (cube.signed.kind[:8] == 2).all() and sorted(cube.signed.element[:8].tolist()) == list(range(8))
    assert (cube.signed.sign[8:14] == -1).all() and (cube.signed.sdf[8:14] < 0).all() and cube.signed.sdf[8] == F(-0.5)
    assert same(flipped.signed.sign, (-cube.signed.sign).astype(np.int8)) and same(flipped.signed.sdf, -cube.signed.sdf) and cube.tables.volume == 1.0 == -flipped.tables.volume
    assert same(flipped.signed.kind, cube.signed.kind) and set(np.unique(cube.signed.kind).tolist()) == {0, 1, 2}
    # the cube's tables, from no library: every edge normal is the sum of the unit normals of its two (or, on a face's diagonal, equal) faces
    e = cube.tables.edge_normal
    assert set(np.round((e * e).sum(axis=1), 12).tolist()) == {2.0, 4.0} and np.abs(cube.tables.vertex_normal).min() > 0.5
    # the flat tetrahedron: both numberings give the same signs (the face numbers differ); all three kinds are met
    a, b = r("flat_tet").signed, r("flat_tet_backwards").signed
    assert same(a.sign, b.sign) and same(a.sdf, b.sdf) and same(a.kind, b.kind) and {0, 1, 2} <= set(np.unique(a.kind).tolist())
    assert not same(r("flat_tet").surface.face, r("flat_tet_backwards").surface.face)
    # open sheets: the sign is the side of the sheet
    t = r("triangle").signed
    assert t.sign[0] == 1 and t.sign[3] == -1 and (t.sign[6:13] == 0).all() and (t.sdf[6:13] == 0).all()          # above, below, on the triangle itself
    # a non-manifold edge holds three faces; a duplicated face counts twice
    three = r("three_on_edge")
    assert three.topology.face_count.max() == 3 and three.signed.stats[ref.EDGE] > 0
    dup = r("duplicate_face")
    k = int(np.nonzero((dup.topology.edge == [0, 1]).all(axis=1))[0][0])
    assert dup.topology.face_count[k] == 2 and same(dup.tables.edge_normal[k], np.array([0.0, 0.0, 2.0]))
    # two faces wound against each other: every edge and vertex normal is exactly zero; the queries nearest to them are undetermined and counted
    ag = r("against")
    assert not ag.tables.edge_normal.any() and not ag.tables.vertex_normal.any() and ag.tables.volume == 0.0
    assert (ag.signed.sign[:3] == 0).all() and (ag.signed.kind[:3] > 0).all() and ag.signed.sign[3] == 1 and ag.signed.sign[4] == -1
    assert ag.signed.stats[ref.UNDETERMINED] >= 3 and ag.signed.stats[ref.STATUS] == 0
    # degenerate faces contribute nothing, and their sides with equal ends have no edge
    dg = r("degenerate")
    assert dg.tables.counts.tolist() == [0, 1, 1, 0] and dg.tables.face_edges[0, 0] == -1 and (dg.tables.face_edges[0, 1:] >= 0).all()
    # the hub: one run of 2000 corners
    hub = r("hub")
    assert (cases.CASES["hub"][1] == 0).sum() == 2000 and hub.tables.vertex_size[0].max() > 3 and hub.signed.stats[ref.VERTEX] > 0
    # NaN and inf queries are excluded
    bad = r("nan_query").signed
    gone = ~np.isfinite(cases.CASES["nan_query"][2]).all(axis=1)
    assert gone.sum() == bad.stats[ref.EXCLUDED] > 0 and np.isinf(bad.sdf[gone]).all() and (bad.sign[gone] == 0).all() and (bad.kind[gone] == -1).all() and (bad.element[gone] == -1).all()
    for name in ("33_sphere", "33_torus"):
        assert len(r(name).signed.sign) == 300 and r(name).signed.stats[ref.INSIDE] > 20 and r(name).signed.stats[ref.OUTSIDE] > 20


@pytest.mark.parametrize("name", cases.CLOSED)
def test_the_emulated_sign_against_the_winding_number(emulator, name):
    got = emulate(emulator, name)
    kept, inside = cases.winding_rows(name)
    finite = np.isfinite(cases.CASES[name][2]).all(axis=1)
    print(name, "rows left out:", int((finite & ~kept).sum()), "of", len(kept), "inside:", int(inside[kept].sum()))
    assert (finite & ~kept).sum() <= cases.UNSTABLE_CAP * len(kept)
    expect = np.where(inside, -1, 1) * (1 if name != "cube_flipped" else -1)
    assert (got.sign[kept] == expect[kept]).all()


def test_foreign_input_is_counted_and_never_read(emulator):
    v, f, q = cases.CASES["cube"]
    want = cases.result("cube")
    face, region = want.surface.face.copy(), want.surface.region.copy()
    face[0], face[1], face[2], region[3], region[4] = len(f), -2, 2 ** 31 - 1, 4, -1
    got = emulator.run(v, f, want.topology.edge, q, want.surface.dist2, face, region)          # (exact arrays under the sanitizers: a read through them is an error)
    assert (got.sign[:5] == 0).all() and (got.kind[:5] == -1).all() and (got.element[:5] == -1).all() and got.stats[ref.STATUS] == 1
    assert same(got.sdf[:5], np.sqrt(want.surface.dist2[:5].astype(np.float64)).astype(F)) and same(got.sign[5:], want.signed.sign[5:])
    assert got.stats[ref.UNDETERMINED] == want.signed.stats[ref.UNDETERMINED] + 5
    bad_faces = f.copy()
    bad_faces[3, 1] = 99                                                                       # a face index outside the vertices: skipped, status raised
    got = emulator.run(v, bad_faces, want.topology.edge, q, want.surface.dist2, np.full(len(q), 3, I), want.surface.region)
    assert got.counts[ref.COUNT_NAMES.index("status")] == 1 and (got.face_edges[3] == -1).all() and (got.kind == -1).all() and got.stats[ref.STATUS] == 1
    other = cases.result("flat_tet").topology.edge                                             # another mesh's edges: sides go missing, nothing is read beyond them
    got = emulator.run(v, f, other, q, want.surface.dist2, want.surface.face, want.surface.region)
    assert got.counts[ref.COUNT_NAMES.index("missing")] > 0 and same(got.face_edges, ref.tables(v, f, other).face_edges)
    empty = emulator.run(np.zeros((0, 3), F), np.zeros((0, 3), I), np.zeros((0, 2), I), q[:4], np.full(4, np.inf, F), np.full(4, -1, I), np.zeros(4, I))
    assert np.isinf(empty.sdf).all() and empty.stats[ref.EXCLUDED] == 4 and empty.volume == 0.0
    for sizes, word in (((-1, 1, 0, 1), ">= 0"), ((4, 2 ** 26, 0, 1), "nf must be below 2^26"), ((4, 2, 7, 1), "n_edges must be 0 .. 3*nf"), ((4, 2, 0, -1), "2^31 - 1")):
        assert word in emulator.run(v, f, want.topology.edge, q, want.surface.dist2, want.surface.face, want.surface.region, code=3, sizes=sizes)


def test_the_winding_number_is_independent_and_right():
    v, f, _ = cases.CASES["cube"]
    w = ref.winding_number(np.array([[0.5, 0.5, 0.5], [0.1, 0.2, 0.3], [2, 2, 2], [-1, 0.5, 0.5]], F), v, f)
    assert np.abs(w - [1, 1, 0, 0]).max() < 1e-12
    assert np.abs(ref.winding_number(np.array([[0.5, 0.5, 0.5]], F), v, f[:, ::-1]) + 1).max() < 1e-12
    source = inspect.getsource(ref.winding_number)
    assert "arctan2" in source and "tables" not in source and "sign(" not in source


# ---- the refusals that need no device ----
def test_refusals_before_any_pointer_is_looked_at():
    l = D.lib()

    def refused(rc, word):
        assert rc == 1 and word in l.gp_last_error(), (word, l.gp_last_error())

    for args, word in (((-1, 0, 0), b">= 0"), ((2 ** 31, 0, 0), b"nv must be below 2^31"), ((4, 2 ** 26, 0), b"nf must be below 2^26"), ((4, 2, 7), b"n_edges must be 0 .. 3*nf"),
                       ((4, 2, -1), b"n_edges must be")):
        assert l.gp_sdf_tables_scratch_bytes(*args) == -1 and word in l.gp_last_error()
    assert l.gp_sdf_tables_scratch_bytes(0, 0, 0) > 0 and l.gp_sdf_tables_scratch_bytes(10 ** 6, 2 * 10 ** 6, 3 * 10 ** 6) >= (48 + 5 * 12) * 2 * 10 ** 6

    def tables(vertices=16, faces=16, nv=4, nf=2, edge=16, ne=5, scratch=16, face_edges=16, edge_normal=16, vertex_normal=16, volume=16, counts=16):
        return l.gp_sdf_tables(vertices, faces, nv, nf, edge, ne, scratch, face_edges, edge_normal, vertex_normal, volume, counts, None)

    for kw, word in ((dict(nv=-1), b">= 0"), (dict(nv=2 ** 31), b"nv must be below 2^31"), (dict(nf=2 ** 26), b"nf must be below 2^26"), (dict(ne=7), b"n_edges must be"),
                     (dict(ne=-1), b"n_edges must be"), (dict(scratch=None), b"null"), (dict(scratch=12), b"8-byte aligned"), (dict(vertices=None), b"null"),
                     (dict(faces=None), b"null"), (dict(edge=None), b"null"), (dict(face_edges=None), b"null"), (dict(edge_normal=None), b"null"),
                     (dict(vertex_normal=None), b"null"), (dict(volume=None), b"null"), (dict(counts=None), b"null")):
        refused(tables(**kw), word)

    def sign(queries=16, nq=5, dist2=16, face=16, region=16, closest=None, bary=None, vertices=16, faces=16, nv=4, nf=2, face_edges=16, edge_normal=16, ne=5, vertex_normal=16,
             sdf=16, sg=16, kind=16, element=16, stats=16):
        return l.gp_sdf_sign(queries, nq, dist2, face, region, closest, bary, vertices, faces, nv, nf, face_edges, edge_normal, ne, vertex_normal, sdf, sg, kind, element, stats, None)

    for kw, word in ((dict(nq=-1), b"2^31 - 1"), (dict(nq=2 ** 31), b"2^31 - 1"), (dict(nv=2 ** 31), b"nv must be below"), (dict(nf=2 ** 26), b"2^26"), (dict(ne=7), b"n_edges must be"),
                     (dict(queries=None), b"null"), (dict(dist2=None), b"null"), (dict(face=None), b"null"), (dict(region=None), b"null"), (dict(vertices=None), b"null"),
                     (dict(faces=None), b"null"), (dict(face_edges=None), b"null"), (dict(edge_normal=None), b"null"), (dict(vertex_normal=None), b"null"), (dict(sdf=None), b"null"),
                     (dict(sg=None), b"null"), (dict(kind=None), b"null"), (dict(element=None), b"null"), (dict(stats=None), b"null")):
        refused(sign(**kw), word)

    for n, word in ((-1, b"2^31 - 1"), (2 ** 31, b"2^31 - 1")):
        assert l.gp_sdf_means_scratch_bytes(n) == -1 and word in l.gp_last_error()
    assert l.gp_sdf_means_scratch_bytes(0) > 0 and l.gp_sdf_means_scratch_bytes(10 ** 6) >= 32 * 3907

    def means(sdf=16, sg=16, n=5, scratch=16, out=16):
        return l.gp_sdf_means(sdf, sg, n, scratch, out, None)

    for kw, word in ((dict(n=-1), b"2^31 - 1"), (dict(scratch=None), b"null"), (dict(scratch=4), b"8-byte aligned"), (dict(sdf=None), b"null"), (dict(sg=None), b"null"),
                     (dict(out=None), b"null")):
        refused(means(**kw), word)


def test_the_python_surface_refuses_before_the_device(monkeypatch):
    for module in (D, S, G, MS):
        monkeypatch.setattr(module, "lib", lambda: pytest.fail("a launch was reached"))
    faces, vertices, cloud = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, 3), torch.zeros(5, 3)
    mesh = (vertices, faces)
    for call in (lambda: D.pseudonormals(mesh), lambda: D.SignedGrid(mesh), lambda: D.signed_distance(cloud, mesh), lambda: D.contains(cloud, mesh),
                 lambda: D.signed_surface_distance(mesh, mesh, n=10), lambda: G.mesh_distance(mesh, mesh, n=10, surface="signed"),
                 lambda: D.means(torch.zeros(3), torch.zeros(3, dtype=torch.int8))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for call, word in ((lambda: D.pseudonormals((vertices, faces.long())), "int32"), (lambda: D.pseudonormals((vertices[0], faces)), r"\[Nv, 3\]"),
                       (lambda: D.means(torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.int8)), "float32"),
                       (lambda: G.mesh_distance(mesh, mesh, surface="unsigned"), "surface must be False, True or \"signed\"")):
        with pytest.raises(RuntimeError, match=word):
            call()
    for call, word in ((lambda: D.SignedGrid(mesh, cell=-1.0), "cell must be finite and >= 0"), (lambda: D.signed_distance(cloud, mesh, cell=float("nan")), "cell must be"),
                       (lambda: D.signed_surface_distance(None, None, thresholds=range(9)), "nt must be 0 .. 8"),
                       (lambda: G.mesh_distance(None, None, thresholds=(float("nan"),), surface="signed"), "a threshold is NaN")):
        with pytest.raises(_lib.GpHipError, match=word):
            call()


def test_signatures_docstrings_and_the_untouched_defaults():
    from gaussianprediction_amd import eval_render as ER
    assert list(inspect.signature(D.pseudonormals).parameters) == ["mesh", "topology"] and list(inspect.signature(D.SignedGrid.__init__).parameters) == ["self", "mesh", "cell", "topology"]
    assert list(inspect.signature(D.SignedGrid.query).parameters) == ["self", "queries"]
    assert list(inspect.signature(D.signed_distance).parameters)[:2] == list(inspect.signature(D.contains).parameters)[:2] == ["queries", "mesh"]
    sig = inspect.signature(D.signed_surface_distance)
    assert list(sig.parameters) == ["mesh_a", "mesh_b", "n", "seed", "thresholds", "cell"] and [p.default for p in sig.parameters.values()][2:] == [100000, 0, G.THRESHOLDS, None]
    assert sig == inspect.signature(S.surface_distance)
    assert D.Pseudonormals._fields == ("face_edges", "edge_normal", "vertex_normal", "topology", "stats")
    assert D.SignedSurface.__slots__ == ("sdf", "sign", "kind", "element", "surface")
    # the three functions that learnt the signed row: their signatures and their defaults are what they were (surface="signed" asks for it)
    for fn, names in ((G.mesh_distance, ["mesh_a", "mesh_b", "n", "seed", "thresholds", "cell", "surface"]), (G.evaluate_mesh_dirs, ["pred_dir", "gt_dir", "n", "thresholds", "seed", "device", "surface"]),
                      (ER.mesh_motion, ["meshes", "n", "thresholds", "seed", "device", "surface"])):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == names and sig.parameters["surface"].default is False and "surface=\"signed\"" in fn.__doc__, fn.__name__
    body = inspect.getsource(G.mesh_distance)
    assert body.index("isinstance(surface, str)") < body.index("if surface:") and inspect.getsource(G).count("from .sdf_ops import") == 1 == body.count("from .sdf_ops import")      # imported only where it is asked for
    assert "watertight" in D.contains.__doc__ and "outward" in D.contains.__doc__ and "slow" in D.contains.__doc__ and "no read" in D.contains.__doc__
    assert "Nothing is read" in D.SignedGrid.query.__doc__ and "the only read" in D.SignedSurface.__doc__ and "ONE read" in D.signed_surface_distance.__doc__
    assert "nothing is read" in D.pseudonormals.__doc__ and "positive means a lies outside b" in D.signed_surface_distance.__doc__
    rows = [{"accuracy": 1.0, "surface": True, "n": 5}, {"accuracy": 3.0, "surface": True, "n": 5}]
    assert G.mean_row(rows) == {"accuracy": 2.0, "surface": True, "n": 5}                                 # as it was
    rows = [{"signed_accuracy": 1.0, "signed": True, "oriented": True}, {"signed_accuracy": -2.0, "signed": True, "oriented": False}]
    assert G.mean_row(rows) == {"signed_accuracy": -0.5, "signed": True, "oriented": False}


def test_the_vectorised_restatement_against_a_loop_per_list():
    """sdf_ref.tables adds the j-th entry of every run at once; here every list is walked on its own, entry by entry."""
    for name in ("flat_tet", "cube", "three_on_edge", "duplicate_face", "degenerate", "against"):
        v, f, _ = cases.CASES[name]
        t = cases.result(name)
        contributes, bad, p, u, made = ref.face_normals(v, f)
        edge_normal, vertex_normal = np.zeros_like(t.tables.edge_normal), np.zeros_like(t.tables.vertex_normal)
        for face in range(len(f)):
            if not made[face]:
                continue
            for k in range(3):
                e1, e2 = p[face, (k + 1) % 3] - p[face, k], p[face, (k + 2) % 3] - p[face, k]
                x = ref.cross(e1, e2)
                angle = np.arctan2(np.sqrt(ref.dot(x, x)), ref.dot(e1, e2))
                vertex_normal[f[face, k]] = vertex_normal[f[face, k]] + angle * u[face]
                if t.tables.face_edges[face, k] >= 0:
                    edge_normal[t.tables.face_edges[face, k]] = edge_normal[t.tables.face_edges[face, k]] + u[face]
        assert same(edge_normal, t.tables.edge_normal) and same(vertex_normal, t.tables.vertex_normal), name
        for face in range(len(f)):
            for k in range(3):
                s, e = sorted((int(f[face, k]), int(f[face, (k + 1) % 3])))
                hit = np.nonzero((t.topology.edge == [s, e]).all(axis=1))[0]
                assert t.tables.face_edges[face, k] == (hit[0] if len(hit) and s != e else -1)
