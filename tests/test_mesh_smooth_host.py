"""No GPU: csrc/gp_mesh_smooth.h against the binding's table (a binding outside _lib.ABIS); the programs of
csrc/mesh_smooth_core.h in a stand-alone build (tests/mesh_smooth_emulate.cpp, under the sanitizers where the host compiler can link
them) against the numpy restatement tests/mesh_smooth_ref.py on every case and option set of tests/mesh_smooth_cases.py -- bit for
bit; face indices out of range under the sanitizers; exact results that need no restatement; the cases against what they are for;
the properties of any topology; the relations the GPU test asserts on the fused sphere, here on an extracted sphere of
tests/tsdf_ref.py; the refusals that need no device."""
import ctypes as C
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import abi_check
import emulate_build
import mesh_smooth_cases as cases
import mesh_smooth_ref as ref
import tsdf_ref
from gaussianprediction_amd import _lib, mesh_smooth as MT
from gaussianprediction_amd.tsdf_ops import Mesh

_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "gp_stream_t": _lib.Ptr}
_POINTEES = {"float", "int32_t", "uint8_t", "void"}
F = np.float32
I = np.int32


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the header, the table, the registry ----
def test_prototype_table_equals_the_header_and_stays_out_of_the_registry():
    before = len(_lib.ABIS)
    protos = abi_check.check_table(MT.ABI, 7, _SCALARS, _POINTEES)
    assert MT.ABI.prototypes is MT.PROTOTYPES and MT.ABI not in _lib.ABIS and len(_lib.ABIS) == before
    assert os.path.samefile(os.path.join(abi_check.ROOT, "include", MT.ABI.header), os.path.join(abi_check.ROOT, "gaussianprediction_amd", "csrc", "gp_mesh_smooth.h"))
    for name in ("gp_mesh_smooth_edges_plan", "gp_mesh_smooth_edges_apply", "gp_mesh_smooth_steps", "gp_mesh_smooth_umbrella"):
        assert protos[name][1][-1] == "gp_stream_t"              # the stream is the last parameter
    assert not os.path.exists(os.path.join(abi_check.ROOT, "include", "gp_mesh_smooth.h"))
    assert len([h for h in os.listdir(os.path.join(abi_check.ROOT, "include")) if h.endswith(".h")]) == 12      # include/ stays at its twelve


def test_symbols_and_constants():
    text = abi_check.header_text(MT.HEADER)
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_MESH_SMOOTH_[A-Z0-9_]+) +(\d+)", text)}
    assert defs["GP_MESH_SMOOTH_ABI_VERSION"] == MT.GP_MESH_SMOOTH_ABI_VERSION == MT.ABI.version == 1
    assert (defs["GP_MESH_SMOOTH_LAPLACIAN"], defs["GP_MESH_SMOOTH_TAUBIN"], defs["GP_MESH_SMOOTH_FREE"], defs["GP_MESH_SMOOTH_FIXED"]) == (MT.LAPLACIAN, MT.TAUBIN, MT.FREE, MT.FIXED)
    assert defs["GP_MESH_SMOOTH_MAX_ITERATIONS"] == MT.MAX_ITERATIONS == ref.MAX_ITERATIONS == 10000
    assert (defs["GP_MESH_SMOOTH_FLAG_BOUNDARY"], defs["GP_MESH_SMOOTH_FLAG_NONMANIFOLD"], defs["GP_MESH_SMOOTH_FLAG_ISOLATED"]) == (MT.FLAG_BOUNDARY, MT.FLAG_NONMANIFOLD, MT.FLAG_ISOLATED) == (1, 2, 4)
    names = ("STATUS", "EDGES", "BOUNDARY", "NONMANIFOLD", "INCONSISTENT", "DEGENERATE", "VERTICES", "FACES", "COUNT_WORDS")
    assert [defs["GP_MESH_SMOOTH_" + n] for n in names] == [MT.STATUS, MT.EDGES, MT.BOUNDARY, MT.NONMANIFOLD, MT.INCONSISTENT, MT.DEGENERATE, MT.VERTICES, MT.FACES, MT.COUNT_WORDS]
    assert [n.lower() for n in names[:8]] == list(MT.COUNT_NAMES) == list(ref.COUNT_NAMES) and MT.COUNT_WORDS == 8
    abi_check.check_applied(MT.ABI)
    assert MT.Edges._fields == ("edge", "face_count", "wind", "offsets", "neighbors", "vertex_flags", "stats")
    assert MT.Smoothed._fields == ("mesh", "attributes", "topology", "stats") and MT.METHODS == {"laplacian": 0, "taubin": 1} and MT.BOUNDARIES == {"free": 0, "fixed": 1}


# ---- the programs in a stand-alone build, under the sanitizers ----
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    d = tmp_path_factory.mktemp("mesh_smooth_emulate")
    exe = emulate_build.build("mesh_smooth_emulate", d, sanitize=True)

    def run(head, arrays, code=0):
        job, out = str(d / "job.bin"), str(d / "out.bin")
        with open(job, "wb") as fp:
            fp.write(head)
            for a in arrays:
                fp.write(np.ascontiguousarray(a).tobytes())
        done = subprocess.run([exe, job, out], timeout=300, stderr=subprocess.PIPE)
        assert done.returncode == code, done.stderr.decode()
        return done.stderr.decode() if code else open(out, "rb").read()

    return run


def job_head(nv, nf, k, options):
    return struct.pack("<iiiiiidd", nv, nf, k, MT.METHODS.get(options["method"], 7), MT.BOUNDARIES.get(options["boundary"], 7), options["iterations"], options["lambda_"], options["mu"])


def emulated(emulator, nv, faces, table, options):
    """(counts, [edge, face_count, wind, offsets, neighbors, vertex_flags], pinned, smoothed, umbrella) of the stand-alone build."""
    nf, k = len(faces), table.shape[1]
    raw = emulator(job_head(nv, nf, k, options), [faces, table])
    counts = np.frombuffer(raw, I, 8)
    ne = int(counts[MT.EDGES])
    assert len(raw) == 4 * (8 + 2 * ne + ne + ne + nv + 1 + 2 * ne + 1 + 2 * nv * k) + nv
    at, out = 32, []
    for dtype, shape in ((I, (ne, 2)), (I, (ne,)), (I, (ne,)), (I, (nv + 1,)), (I, (2 * ne,)), (np.uint8, (nv,)), (I, (1,)), (F, (nv, k)), (F, (nv, k))):
        n = int(np.prod(shape))
        out.append(np.frombuffer(raw, dtype, n, at).reshape(shape))
        at += n * np.dtype(dtype).itemsize
    return counts, out[:6], int(out[6][0]), out[7], out[8]


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_emulated_programs_against_the_restatement(emulator, name):
    m, t = cases.CASES[name], cases.topology(name)
    for run in cases.runs_of(name):
        options = cases.RUNS[name][run]
        counts, topo, pinned, smoothed, umbrella = emulated(emulator, len(m.vertices), m.faces, cases.table(m), options)
        print(name, run, counts.tolist(), pinned)
        assert t.status == 0 and same(counts, t.counts) and all(same(g, w) for g, w in zip(topo, ref.parts(t))), (name, run)
        assert pinned == ref.pinned_count(t, options["boundary"])
        assert all(same(g, w) for g, w in zip(cases.split(smoothed), cases.smoothed(name, run))), (name, run)
        assert all(same(g, w) for g, w in zip(cases.split(umbrella), cases.umbrella(name))), (name, run)


def test_the_vectorised_restatement_equals_the_loop():
    for name in cases.CASES:
        m, t = cases.CASES[name], cases.topology(name)
        packed = ref.edges_vectorised(m.faces, len(m.vertices))
        assert packed.stats == t.stats and same(packed.counts, t.counts) and all(same(g, w) for g, w in zip(ref.parts(packed), ref.parts(t))), name
        for run in cases.runs_of(name):
            if (name, run) not in cases.VECTORISED:
                assert same(ref.smooth(cases.table(m), t, one_step=ref.step_vectorised, **cases.RUNS[name][run]), np.concatenate(cases.smoothed(name, run), axis=1)), (name, run)
    assert cases.VECTORISED == {(cases.LARGE, 1)} and cases.RUNS[cases.LARGE][0]["iterations"] == 1          # the large case has its run under the loop too


@pytest.mark.parametrize("case, face, corner, value", cases.BAD)
def test_the_emulator_skips_and_reports_a_face_index_out_of_range(emulator, case, face, corner, value):
    """Under the sanitizers every array has its exact size: an index dereferenced without its check ends the child."""
    m = cases.CASES[case]
    faces = cases.bad_faces(case, face, corner, value)
    want = ref.edges(faces, len(m.vertices))
    counts, topo, _, _, _ = emulated(emulator, len(m.vertices), faces, np.zeros((len(m.vertices), 0), F), cases.S(0))
    assert counts[MT.STATUS] == 1 == want.status and counts[MT.FACES] == len(faces) - 1 and same(counts, want.counts) and all(same(g, w) for g, w in zip(topo, ref.parts(want)))


def test_the_emulator_refuses_as_the_library_does(emulator):
    m = cases.CASES["one_triangle"]
    for kw, word in ((dict(lambda_=np.nan), "lambda_ and mu must be finite"), (dict(mu=np.inf), "lambda_ and mu must be finite"), (dict(iterations=-1), "iterations must be"),
                     (dict(iterations=10001), "iterations must be"), (dict(method="cotangent"), "method must be"), (dict(boundary="sliding"), "boundary must be")):
        options = dict(cases.S(1), **kw)
        said = emulator(job_head(3, 1, 3, options), [m.faces, m.vertices], code=3)
        assert word in said and MT.check_options(**options) in said and ref.check_options(**options) in said
    assert MT.check_options(**cases.S(10000)) is None and MT.check_options(**cases.S(0, lambda_=-1e300, mu=1e300)) is None and MT.check_options(**cases.S(True)) is not None


# ---- exact results, known without any restatement ----
def test_the_octahedron_halves_the_single_triangle_stays_and_no_iteration_is_the_identity(emulator):
    v, f = cases.OCTAHEDRON
    t = ref.edges(f, 6)
    assert t.stats == dict(edges=12, boundary=0, nonmanifold=0, inconsistent=0, degenerate=0, vertices=6, faces=8, euler=2, watertight=True)
    assert (np.diff(t.offsets) == 4).all() and all(v[t.neighbors[t.offsets[i]:t.offsets[i + 1]]].sum(axis=0).tolist() == [0, 0, 0] for i in range(6))
    for n in (1, 2, 5, 30):                  # four neighbours that sum to zero: n steps with lambda_ = 0.5 give exactly p 2^-n
        options = cases.S(n, "laplacian", "fixed")
        want = v * F(2.0 ** -n)
        assert same(ref.smooth(v, t, **options), want) and same(emulated(emulator, 6, f, v, options)[3], want)
    tri = cases.CASES["one_triangle"]
    for method in ("laplacian", "taubin"):
        got = emulated(emulator, 3, tri.faces, tri.vertices, cases.S(5, method, "fixed"))
        assert same(got[3], tri.vertices) and got[2] == 3 and same(ref.smooth(tri.vertices, cases.topology("one_triangle"), 5, method), tri.vertices)
        assert not same(emulated(emulator, 3, tri.faces, tri.vertices, cases.S(5, method, "free"))[3], tri.vertices)
    for name in ("not_finite", "hub", "cube_soup"):
        m = cases.CASES[name]
        for method in ("laplacian", "taubin"):
            assert same(emulated(emulator, len(m.vertices), m.faces, cases.table(m), cases.S(0, method, "free"))[3], cases.table(m))          # NaN and -0.0 in equal bits


# ---- the cases reach what they are for ----
def test_the_small_cases_reach_what_they_are_for():
    T = cases.topology
    assert T("empty").counts.tolist() == [0] * 8 and T("empty").offsets.tolist() == [0] and not T("empty").stats["watertight"]
    assert T("no_faces").vertex_flags.tolist() == [4] * 5 and T("no_faces").offsets.tolist() == [0] * 6
    one = T("one_triangle")
    assert one.edge.tolist() == [[0, 1], [0, 2], [1, 2]] and one.face_count.tolist() == [1, 1, 1] and one.wind.tolist() == [1, -1, 1] and one.vertex_flags.tolist() == [1, 1, 1]
    assert one.stats["boundary"] == 3 and one.stats["euler"] == 1 and one.neighbors.tolist() == [1, 2, 0, 2, 0, 1]
    for name, wind, inconsistent in (("two_consistent", 0, 0), ("two_inconsistent", 2, 1), ("two_inconsistent_down", -2, 1)):
        t = T(name)
        shared = t.edge.tolist().index([1, 2])
        assert t.face_count[shared] == 2 and t.wind[shared] == wind and t.stats["inconsistent"] == inconsistent and t.stats["boundary"] == 4 and t.stats["edges"] == 5
    for name, euler, ne in (("tetrahedron", 2, 6), ("octahedron", 2, 12), ("cube_welded", 2, 18), ("torus_64", 0, 192), ("torus_1025", 0, 3075), (cases.LARGE, 0, 3 * 20022)):
        t = T(name)
        assert t.stats["watertight"] and t.stats["euler"] == euler and t.stats["edges"] == ne and (t.face_count == 2).all() and (t.wind == 0).all() and not t.vertex_flags.any()
        assert tsdf_ref.mesh_facts(cases.CASES[name].vertices, cases.CASES[name].faces)["edge_uses"] == {2}
    three = T("three_on_an_edge")
    assert three.face_count[three.edge.tolist().index([1, 2])] == 3 and three.stats["nonmanifold"] == 1 and three.vertex_flags.tolist() == [1, 3, 3, 1, 1]
    dup = T("duplicated_face")
    assert dup.face_count.tolist() == [2, 2, 3, 1, 1] and dup.wind.tolist() == [2, -2, 1, 1, -1] and dup.stats["inconsistent"] == 2 and dup.stats["nonmanifold"] == 1
    soup = T("cube_soup")
    assert soup.stats["boundary"] == soup.stats["edges"] == 36 and (soup.vertex_flags == 1).all() and soup.stats["euler"] == 36 - 36 + 12
    rep = T("repeated_index")
    assert rep.stats["degenerate"] == 4 and rep.stats["faces"] == 3 and int(rep.face_count.sum()) == 3 * 3 - 4 and rep.edge.tolist() == [[0, 1], [0, 2], [1, 2], [1, 3]]
    assert rep.face_count.tolist() == [1, 1, 1, 2] and rep.wind.tolist() == [1, -1, 1, 0]          # the face (1, 1, 3) runs 1 -> 3 and 3 -> 1
    iso = T("isolated")
    assert np.nonzero(iso.vertex_flags == 4)[0].tolist() == [0, 1, 5, 6, 9, 11, 12] and iso.stats["vertices"] == 6 and iso.stats["watertight"] and iso.stats["euler"] == 2
    hub = T("hub")
    assert int(np.diff(hub.offsets)[0]) == 2000 and hub.stats["boundary"] == 2000 and hub.vertex_flags[0] == 0 and (hub.vertex_flags[1:] == 1).all()
    assert [len(cases.CASES[f"torus_{n}"].vertices) for n in (63, 64, 65, 1023, 1024, 1025)] == [63, 64, 65, 1023, 1024, 1025] and len(cases.CASES[cases.LARGE].vertices) == 20022
    assert sorted({o["iterations"] for o in cases.ALL}) == [0, 1, 5] and {(o["method"], o["boundary"]) for o in cases.ALL} == {(m, b) for m in MT.METHODS for b in MT.BOUNDARIES}
    assert [r.shape[1] for r in cases.CASES["hub"].rows] == [1, 4, 7]


def test_the_order_of_the_hub_sum_shows_and_values_that_are_not_finite_pass_through():
    m, t = cases.CASES["hub"], cases.topology("hub")
    v = m.vertices.astype(np.float64)
    forwards, backwards = np.zeros(3), np.zeros(3)
    for u in t.neighbors[:2000]:
        forwards = forwards + v[u]
    for u in t.neighbors[:2000][::-1]:
        backwards = backwards + v[u]
    assert not same(forwards, backwards) and same((forwards / 2000.0 - v[0]).astype(F), cases.umbrella("hub")[0][0])
    nf = cases.smoothed("not_finite", cases.ALL.index(cases.S(1, "laplacian", "free")))
    assert np.isnan(nf[0][:, 0]).all() and np.isfinite(nf[0][:, 1:]).all()          # every vertex has the NaN or a neighbour with it
    fixed = cases.smoothed("hub", 1)[0]
    assert same(fixed[1:], m.vertices[1:]) and not same(fixed[0], m.vertices[0])          # the rim is boundary; the hub moves


# ---- the properties of any result, here of the restatement's ----
@pytest.mark.parametrize("name", list(cases.CASES))
def test_properties_of_the_restatement(name):
    m, t = cases.CASES[name], cases.topology(name)
    cases.check_properties(len(m.vertices), len(m.faces), *ref.parts(t), t.stats)
    for run in cases.runs_of(name):
        options, got = cases.RUNS[name][run], cases.smoothed(name, run)
        still = np.diff(t.offsets) == 0
        if options["boundary"] == "fixed":
            still |= (t.vertex_flags & 3) != 0
        if options["iterations"] == 0:
            still[:] = True
        for g, w in zip(got, cases.split(cases.table(m))):
            assert same(g[still], w[still])


# ---- the relations the GPU test asserts on the fused sphere, on an extracted volume of tsdf_ref ----
def test_an_extracted_volume_is_watertight_and_taubin_smooths_without_the_shrinkage_of_laplacian():
    m = cases.mesh_cases.CASES["two_spheres"]
    t = ref.edges(m.faces, len(m.vertices))
    print(t.stats)
    assert t.stats["boundary"] == 0 and t.stats["watertight"] and t.stats["euler"] == 4 and t.stats["degenerate"] == 0          # DESIGN section 26's word, checked
    taubin = ref.smooth(m.vertices, t, 10, "taubin", one_step=ref.step_vectorised)
    laplacian = ref.smooth(m.vertices, t, 10, "laplacian", one_step=ref.step_vectorised)
    rough = [ref.roughness(v, t) for v in (m.vertices, taubin, laplacian)]
    volume = [ref.enclosed_volume(v, m.faces) for v in (m.vertices, taubin, laplacian)]
    print("roughness", rough, "volume", volume)
    assert rough[1] < rough[0] and 0 < volume[2] < volume[1]


# ---- the refusals that need no device ----
def test_refusals_before_any_pointer_is_looked_at():
    l = MT.lib()

    def refused(rc, word):
        assert rc == 1 and word in l.gp_last_error(), (word, l.gp_last_error())

    from gaussianprediction_amd import mesh_ops
    sizes = (((2 ** 31, 4), b"nv must be below 2^31"), ((4, 715827883), b"3*nf must be below 2^31"), ((-1, 4), b">= 0"), ((4, -1), b">= 0"), ((4, 357913942), b"6*nf must be below 2^31"))
    for (nv, nf), word in sizes:
        assert l.gp_mesh_smooth_scratch_bytes(nv, nf) == -1 and word in l.gp_last_error() and MT.check_sizes(nv, nf).encode() in l.gp_last_error()
        refused(l.gp_mesh_smooth_edges_plan(8, nv, nf, 8, 8, None), word)
        refused(l.gp_mesh_smooth_edges_apply(nv, nf, 0, 8, 8, 8, 8, 8, 8, 8, None), word)
    assert mesh_ops.check_sizes(4, 357913942) is None and MT.check_sizes(4, 357913941) is None
    assert l.gp_mesh_smooth_scratch_bytes(0, 0) > 0 and l.gp_mesh_smooth_scratch_bytes(2 ** 31 - 1, 357913941) > 38 * (2 ** 31 - 6)
    for args, word in (((None, 4, 2, 8, 8), b"null"), ((8, 4, 2, None, 8), b"null"), ((8, 4, 2, 8, None), b"null"), ((8, 4, 2, 12, 8), b"aligned")):
        refused(l.gp_mesh_smooth_edges_plan(*args, None), word)
    for args, word in (((4, 2, 7, 8, 8, 8, 8, 8, 8, 8), b"n_edges"), ((4, 2, -1, 8, 8, 8, 8, 8, 8, 8), b"n_edges"), ((4, 2, 5, None, 8, 8, 8, 8, 8, 8), b"null"),
                       ((4, 2, 5, 12, 8, 8, 8, 8, 8, 8), b"aligned"), ((4, 2, 5, 8, None, 8, 8, 8, 8, 8), b"null"), ((4, 2, 5, 8, 8, None, 8, 8, 8, 8), b"null"),
                       ((4, 2, 5, 8, 8, 8, None, 8, 8, 8), b"null"), ((4, 2, 5, 8, 8, 8, 8, None, 8, 8), b"null"), ((4, 2, 5, 8, 8, 8, 8, 8, None, 8), b"null"),
                       ((4, 2, 5, 8, 8, 8, 8, 8, 8, None), b"null")):
        refused(l.gp_mesh_smooth_edges_apply(*args, None), word)

    def steps(src=8, nv=4, k=3, offsets=8, neighbors=8, n=10, pinned=8, method=MT.TAUBIN, boundary=MT.FIXED, iterations=1, lambda_=0.5, mu=-0.53, scratch=8, dst=8):
        return l.gp_mesh_smooth_steps(src, nv, k, offsets, neighbors, n, pinned, method, boundary, iterations, lambda_, mu, scratch, dst, None, None)

    for kw, word in ((dict(k=0), b"k must be"), (dict(k=1025), b"k must be"), (dict(nv=2 ** 22, k=1024), b"nv*k"), (dict(nv=-1), b"nv must be"), (dict(n=-1), b"n_neighbors"),
                     (dict(n=2 ** 31), b"n_neighbors"), (dict(method=2), b"method must be"), (dict(boundary=2), b"boundary must be"), (dict(iterations=-1), b"iterations must be"),
                     (dict(iterations=10001), b"iterations must be"), (dict(lambda_=float("nan")), b"finite"), (dict(mu=float("-inf")), b"finite"), (dict(scratch=None), b"null"),
                     (dict(scratch=12), b"aligned"), (dict(src=None), b"null"), (dict(dst=None), b"null"), (dict(offsets=None), b"null"), (dict(neighbors=None), b"null"),
                     (dict(pinned=None), b"null")):
        refused(steps(**kw), word)
        if b"must be" in word or b"finite" in word:
            assert any(w.encode() in l.gp_last_error() for w in ("k must be 1 .. 1024", "nv*k must be below 2^31", "nv must be", "n_neighbors must be", MT.check_options("x", "fixed", 1, 0.5, 0.5),
                                                                 MT.check_options("taubin", "x", 1, 0.5, 0.5), MT.check_options("taubin", "fixed", -1, 0.5, 0.5),
                                                                 MT.check_options("taubin", "fixed", 1, float("nan"), 0.5)))
    for args, word in (((8, 4, 0, 8, 8, 10, 8), b"k must be"), ((8, 2 ** 22, 1024, 8, 8, 10, 8), b"nv*k"), ((None, 4, 3, 8, 8, 10, 8), b"null"), ((8, 4, 3, None, 8, 10, 8), b"null"),
                       ((8, 4, 3, 8, None, 10, 8), b"null"), ((8, 4, 3, 8, 8, 10, None), b"null"), ((8, 4, 3, 8, 8, -1, 8), b"n_neighbors")):
        refused(l.gp_mesh_smooth_umbrella(*args, None), word)
    assert l.gp_mesh_smooth_rows_bytes(4, 0) == -1 and b"k must be" in l.gp_last_error() and l.gp_mesh_smooth_rows_bytes(2 ** 22, 1024) == -1 and l.gp_mesh_smooth_rows_bytes(1000, 3) >= 24000


def test_the_python_surface_refuses_before_the_device(monkeypatch):
    monkeypatch.setattr(MT, "lib", lambda: pytest.fail("a launch was reached"))
    faces, vertices = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, 3)
    mesh = Mesh(vertices, faces, None)
    topo = MT.Edges(None, None, None, torch.zeros(5, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(4, dtype=torch.uint8), {})
    for call in (lambda: MT.edges(faces, 4), lambda: MT.smooth(mesh), lambda: MT.smooth(mesh, topology=topo), lambda: MT.umbrella(vertices, topo)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for call, word in ((lambda: MT.edges(faces.long(), 4), "int32"), (lambda: MT.edges(faces[:, :2], 4), r"\[Nf, 3\]"), (lambda: MT.smooth(Mesh(vertices[0], faces, None)), r"\[Nv, 3\]"),
                       (lambda: MT.umbrella(vertices[0], topo), r"\[Nv, k\]")):
        with pytest.raises(RuntimeError, match=word):
            call()
    for call, word in ((lambda: MT.smooth(mesh, lambda_=float("nan")), "must be finite"), (lambda: MT.smooth(mesh, mu=float("inf")), "must be finite"),
                       (lambda: MT.smooth(mesh, iterations=-1), "iterations must be 0 .. 10000"), (lambda: MT.smooth(mesh, iterations=10001), "iterations must be"),
                       (lambda: MT.smooth(mesh, iterations=2.5), "iterations must be"), (lambda: MT.smooth(mesh, method="cotangent"), "method must be"),
                       (lambda: MT.smooth(mesh, boundary="sliding"), "boundary must be")):
        with pytest.raises(_lib.GpHipError, match=word):
            call()


def test_signatures_and_docstrings():
    from gaussianprediction_amd import eval_render as ER
    assert list(inspect.signature(MT.edges).parameters) == ["faces", "n_vertices"] and list(inspect.signature(MT.umbrella).parameters) == ["rows", "topology"]
    sig = inspect.signature(MT.smooth)
    assert list(sig.parameters) == ["mesh", "iterations", "method", "lambda_", "mu", "boundary", "colors", "attributes", "topology"]
    assert [p.default for p in sig.parameters.values()][1:] == [10, "taubin", 0.5, -0.53, "fixed", False, (), None]
    sig = inspect.signature(ER.render_meshes)
    assert [sig.parameters[k].default for k in ("smooth", "smooth_method", "smooth_boundary", "topology_report")] == [0, "taubin", "fixed", False]
    assert open(ER.__file__).read().count("render_meshes(") == 1 and "mesh_topology.json" in ER.render_meshes.__doc__
    doc = " ".join(MT.smooth.__doc__.split())
    assert "Parity with Open3D to the bit is unpinned" in doc and "nothing is read" in doc and "One read" in MT.edges.__doc__ and "Nothing is read" in MT.umbrella.__doc__
