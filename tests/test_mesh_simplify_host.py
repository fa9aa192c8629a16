"""No GPU: csrc/gp_mesh_simplify.h against the binding's table (a binding outside _lib.ABIS); the programs of
csrc/mesh_simplify_core.h in a stand-alone build (tests/mesh_simplify_emulate.cpp, under the sanitizers where the host compiler can
link them) against the numpy restatement tests/mesh_simplify_ref.py on every case and option set of tests/mesh_simplify_cases.py --
bit for bit; face indices out of range under the sanitizers; the cases against what they are for and against facts that do not come
from the restatement; the properties of any result; the refusals that need no device."""
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
import mesh_simplify_cases as cases
import mesh_simplify_ref as ref
import tsdf_ref
from gaussianprediction_amd import _lib, mesh_simplify as MZ
from gaussianprediction_amd.tsdf_ops import Mesh

_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "gp_stream_t": _lib.Ptr}
_POINTEES = {"float", "double", "int32_t", "void"}
F = np.float32
I = np.int32


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the header, the table, the registry ----
def test_prototype_table_equals_the_header_and_stays_out_of_the_registry():
    before = len(_lib.ABIS)
    protos = abi_check.check_table(MZ.ABI, 6, _SCALARS, _POINTEES)
    assert MZ.ABI.prototypes is MZ.PROTOTYPES and MZ.ABI not in _lib.ABIS and len(_lib.ABIS) == before
    assert os.path.samefile(os.path.join(abi_check.ROOT, "include", MZ.ABI.header), os.path.join(abi_check.ROOT, "gaussianprediction_amd", "csrc", "gp_mesh_simplify.h"))
    for name in ("gp_mesh_simplify_bounds", "gp_mesh_simplify_plan", "gp_mesh_simplify_apply", "gp_mesh_simplify_rows"):
        assert protos[name][1][-1] == "gp_stream_t"              # the stream is the last parameter
    assert not os.path.exists(os.path.join(abi_check.ROOT, "include", "gp_mesh_simplify.h"))
    assert len([h for h in os.listdir(os.path.join(abi_check.ROOT, "include")) if h.endswith(".h")]) == 12      # include/ stays at its twelve


def test_symbols_and_constants():
    text = abi_check.header_text(MZ.HEADER)
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_MESH_SIMPLIFY_[A-Z0-9_]+) +(\d+)", text)}
    assert defs["GP_MESH_SIMPLIFY_ABI_VERSION"] == MZ.GP_MESH_SIMPLIFY_ABI_VERSION == MZ.ABI.version == 1
    assert (defs["GP_MESH_SIMPLIFY_WELD"], defs["GP_MESH_SIMPLIFY_GRID"], defs["GP_MESH_SIMPLIFY_FIRST"], defs["GP_MESH_SIMPLIFY_AVERAGE"]) == (MZ.WELD, MZ.GRID, MZ.FIRST, MZ.AVERAGE)
    assert defs["GP_MESH_SIMPLIFY_MAX_DIM"] == MZ.MAX_DIM == ref.MAX_DIM == 2 ** 21
    names = ("STATUS", "VERTICES", "FACES", "CLUSTERS", "COLLAPSED", "ZERO_AREA", "DUPLICATES", "COUNT_WORDS")
    assert [defs["GP_MESH_SIMPLIFY_" + n] for n in names] == [MZ.STATUS, MZ.VERTICES, MZ.FACES, MZ.CLUSTERS, MZ.COLLAPSED, MZ.ZERO_AREA, MZ.DUPLICATES, MZ.COUNT_WORDS]
    assert names.index("COUNT_WORDS") == 7 and MZ.COUNT_WORDS == 8 and defs["GP_MESH_SIMPLIFY_RECORD_WORDS"] == MZ.RECORD_WORDS == 8
    abi_check.check_applied(MZ.ABI)
    assert MZ.Simplified._fields == ("mesh", "vertex_map", "face_index", "vertex_counts", "attributes", "stats") and MZ.CONTRACTIONS == {"first": 0, "average": 1}


# ---- the programs in a stand-alone build, under the sanitizers ----
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    d = tmp_path_factory.mktemp("mesh_simplify_emulate")
    exe = emulate_build.build("mesh_simplify_emulate", d, sanitize=True)

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


def job_head(nv, nf, options, k):
    voxel, bounds = options["voxel_size"], options.get("bounds")
    box = np.zeros(6) if bounds is None else np.concatenate([np.asarray(b, np.float64) for b in bounds])
    return (struct.pack("<iii", 1, nv, nf) + struct.pack("<iiiiii", MZ.WELD if voxel is None else MZ.GRID, MZ.CONTRACTIONS[options.get("contraction", "average")],
                                                         int(options.get("drop_zero_area", False)), int(options.get("drop_duplicates", True)),
                                                         int(options.get("keep_unreferenced", False)), k)
            + struct.pack("<d", 0.0 if voxel is None else voxel) + box.tobytes())


def emulated_bounds(emulator, vertices):
    raw = emulator(struct.pack("<iii", 0, len(vertices), 0), [vertices])
    assert len(raw) == 64
    return np.frombuffer(raw, np.float64)


def emulated(emulator, vertices, faces, rows, options):
    """(counts, [vertices, faces, vertex_map, face_index, vertex_counts, *rows]) of the stand-alone build.  Without bounds in the
    options the emulated bounds entry comes first, as on the device."""
    nv, nf = len(vertices), len(faces)
    if options["voxel_size"] is not None and options.get("bounds") is None and nv:
        record = emulated_bounds(emulator, vertices)
        assert record[6] == 0
        options = dict(options, bounds=(record[:3], record[3:6]))
    table = np.concatenate(rows, axis=1) if rows else np.zeros((nv, 0), F)
    k = table.shape[1]
    raw = emulator(job_head(nv, nf, options, k), [vertices, faces, table])
    counts = np.frombuffer(raw, I, 8)
    nv2, nf2 = int(counts[MZ.VERTICES]), int(counts[MZ.FACES])
    assert len(raw) == 4 * (8 + 3 * nv2 + 3 * nf2 + nv + nf2 + nv2 + k * nv2)
    at = 32
    out = []
    for dtype, shape in ((F, (nv2, 3)), (I, (nf2, 3)), (I, (nv,)), (I, (nf2,)), (I, (nv2,)), (F, (nv2, k))):
        n = int(np.prod(shape))
        out.append(np.frombuffer(raw, dtype, n, at).reshape(shape))
        at += 4 * n
    widths = np.cumsum([r.shape[1] for r in rows])[:-1] if rows else []
    return counts, out[:5] + (np.split(out[5], widths, axis=1) if rows else [])


def check_counts(counts, want):
    s = want.stats
    assert counts.tolist() == [want.status, len(want.vertices), len(want.faces), s["clusters"], s["collapsed"], s["zero_area"], s["duplicates"], 0]


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_emulated_programs_against_the_restatement(emulator, name):
    m = cases.CASES[name]
    for run in cases.runs_of(name):
        want = cases.result(name, run)
        counts, got = emulated(emulator, m.vertices, m.faces, cases.rows_of(m), cases.RUNS[name][run])
        print(name, run, counts.tolist())
        check_counts(counts, want)
        assert want.status == 0 and len(got) == 7 and all(same(g, w) for g, w in zip(got, cases.parts(want))), (name, run)


def test_the_emulated_bounds_against_the_restatement(emulator):
    for name in ("one_triangle", "cube_soup", "fan", "two_spheres", "zero_area"):
        v = cases.CASES[name].vertices
        assert same(emulated_bounds(emulator, v), ref.exact_bounds(v)), name
    zero = emulated_bounds(emulator, np.array([[-0.0, 0.0, -0.0], [np.inf, np.nan, -np.inf]], F))
    assert same(zero, np.array([0, 0, 0, 0, 0, 0, 1, 0], np.float64)) and not np.signbit(zero).any()          # a zero is +0.0; what is not finite only raises the flag
    assert ref.exact_bounds(cases.CASES["zero_area"].vertices)[6] == 1


@pytest.mark.parametrize("case, face, corner, value", cases.BAD)
def test_the_emulator_skips_and_reports_a_face_index_out_of_range(emulator, case, face, corner, value):
    """Under the sanitizers every array has its exact size: an index dereferenced without its check ends the child."""
    m = cases.mesh_cases.CASES[case]
    faces = cases.bad_faces(case, face, corner, value)
    for options in (cases.W(), cases.G(0.5, drop_zero_area=True)):
        want = ref.simplify(m.vertices, faces, cases.rows_of(m), **options)
        counts, got = emulated(emulator, m.vertices, faces, cases.rows_of(m), options)
        check_counts(counts, want)
        assert counts[MZ.STATUS] == 1 and face not in got[3] and all(same(g, w) for g, w in zip(got, cases.parts(want)))


def test_the_emulator_reports_a_vertex_outside_the_bounds_and_refuses_as_the_library_does(emulator):
    m = cases.CASES["one_triangle"]
    inside, outside = cases.G(0.5, bounds=((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))), cases.G(0.5, bounds=((0.0, 0.0, 0.0), (0.25, 1.0, 1.0)))
    assert emulated(emulator, m.vertices, m.faces, [], inside)[0][MZ.STATUS] == 0 and ref.simplify(m.vertices, m.faces, **outside).status == 1
    assert emulated(emulator, m.vertices, m.faces, [], outside)[0][MZ.STATUS] == 1
    for bad in ([np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [3e38, 0, 0]):          # never a conversion of such a value: the sanitizers would end the child
        v = m.vertices.copy()
        v[1] = bad
        assert emulated(emulator, v, m.faces, [], inside)[0][MZ.STATUS] == 1 and ref.simplify(v, m.faces, **inside).status == 1
    box = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    for voxel, bounds, word in ((0.0, box, "finite and > 0"), (-1.0, box, "finite and > 0"), (np.nan, box, "finite and > 0"), (np.inf, box, "finite and > 0"),
                                (2.0 ** -21, box, "voxel_size is too small"), (0.5, ((0.0, 0.0, 0.0), (1.0, np.inf, 1.0)), "bounds must be finite"),
                                (0.5, ((0.0, 2.0, 0.0), (1.0, 1.0, 1.0)), "bounds must be finite")):
        said = emulator(job_head(3, 1, cases.G(voxel, bounds=bounds), 0), [m.vertices, m.faces], code=3)
        assert word in said and MZ.check_voxel(voxel, bounds) in said and ref.plan_grid(voxel, np.concatenate(bounds)) in said
    assert MZ.check_voxel(2.0 ** -20, box) is None and MZ.check_voxel(0.5) is None and not isinstance(ref.plan_grid(2.0 ** -20, np.concatenate(box)), str)


# ---- the cases reach what they are for; the restatement against independent facts ----
def test_the_small_cases_reach_what_they_are_for():
    R = cases.result
    assert [len(R("empty", k).vertices) for k in cases.runs_of("empty")] == [0] * 4 and R("empty", 2).stats["clusters"] == 0
    assert len(R("no_faces", 0).vertices) == 0 and (R("no_faces", 0).vertex_map == -1).all() and len(R("no_faces", 1).vertices) == 5
    assert R("no_faces", 2).vertex_counts.tolist() == [1, 1, 2, 1] and same(R("no_faces", 2).vertices, np.array([[0, 1, 2], [3, 4, 5], [7.5, 8.5, 9.5], [12, 13, 14]], F))
    one = cases.CASES["one_triangle"]
    assert same(R("one_triangle", 0).vertices, one.vertices) and same(R("one_triangle", 0).faces, one.faces) and len(R("one_triangle", 4).faces) == 0
    assert R("one_triangle", 4).vertex_counts.tolist() == [3] and R("one_triangle", 4).stats["collapsed"] == 1
    # the cube: 36 vertices of 12 faces weld to the 8 corners of a closed surface of volume s^3
    cube, soup = R("cube_soup", 0), cases.CASES["cube_soup"]
    assert np.signbit(soup.vertices[0, 0]) and (soup.vertices[1:] == 0).any() and not np.signbit(soup.vertices[1:]).any()
    assert cube.vertices.shape == (8, 3) and cube.faces.shape == (12, 3) and cube.vertex_counts.sum() == 36 and set(cube.vertex_counts.tolist()) <= {3, 4, 5, 6}
    facts = tsdf_ref.mesh_facts(cube.vertices, cube.faces)
    assert facts["edge_uses"] == {2} and facts["euler"] == 2 and facts["volume"] == cases.CUBE_SIDE ** 3 and facts["unreferenced"] == 0
    assert np.signbit(cube.vertices[0, 0])                      # "first": the bits of the smallest member, its -0.0 included
    # collapse: two corners in a cell, three in a cell; the face that shares the cells of another is its copy
    c = R("collapse", 1)
    assert c.stats == dict(clusters=6, collapsed=2, zero_area=0, duplicates=1, unreferenced=3) and c.face_index.tolist() == [2] and c.vertex_map.tolist() == [-1] * 6 + [0, 1, 2] * 2
    assert R("collapse", 2).face_index.tolist() == [2, 3] and R("collapse", 0).face_index.tolist() == [0, 1, 2, 3]
    # duplicates: the rotations and the copy go, the first, the flip and the other face stay
    d = R("duplicates", 0)
    assert d.face_index.tolist() == [0, 4, 5] and d.stats["duplicates"] == 3 and same(d.faces, cases.CASES["duplicates"].faces[[0, 4, 5]])
    assert R("duplicates", 1).face_index.tolist() == list(range(6))
    # zero area: the collinear face goes, the face with a NaN vector stays
    z = R("zero_area", 0)
    assert z.face_index.tolist() == [1, 2] and z.stats["zero_area"] == 1 and z.vertex_map.tolist() == [0, 1, -1, 2, 3, 4] and R("zero_area", 1).face_index.tolist() == [0, 1, 2]
    assert np.isnan(ref.mesh_ref.face_vectors(cases.CASES["zero_area"].vertices, cases.CASES["zero_area"].faces)[1]).any()
    # cell boundaries: the exact value and the float32 above it share a cell, the one below lies in the cell before
    b, B = cases.CASES["cell_boundary"], cases.BOUNDARY
    status, key = ref.keys(b.vertices, B.voxel, np.concatenate(B.bounds))
    assert status == 0 and (F(B.at) + 0.125) / 0.25 == 2.0 and [key[3 * a:3 * a + 3, a].tolist() for a in range(3)] == [[1, 2, 2]] * 3
    assert b.vertices[0, 0] < b.vertices[1, 0] < b.vertices[2, 0] and b.vertices[2, 0] - b.vertices[0, 0] < 1e-7
    assert R("cell_boundary", 0).stats["clusters"] == 8 and R("cell_boundary", 0).vertex_counts.tolist() == [1, 2, 1, 2, 1, 2, 1, 1]
    # a cluster all of whose faces collapse
    lost, kept = R("lost_cluster", 0), R("lost_cluster", 1)
    assert lost.vertex_map.tolist() == [-1, -1, -1, 0, 1, 2, -1] and lost.stats["unreferenced"] == 2 and kept.vertex_map.tolist() == [0, 0, 0, 1, 2, 3, 4]
    assert kept.vertex_counts.tolist() == [3, 1, 1, 1, 1] and same(lost.faces, kept.faces - 1) and len(kept.vertices) == 5


def test_the_long_list_and_the_tiles():
    R = cases.result
    # the fan under one coarse cell: one member list of 5002.  The float64 sum of its float32 coordinates is exact whatever the order;
    # on the fan whose radii span forty powers of two it rounds, and summed backwards the float64 sum has other bits
    one = R("fan", 0)
    assert one.vertex_counts.tolist() == [5002] and len(one.faces) == 0 and one.stats["collapsed"] == 5000 and len(R("fan", 1).vertices) == 0 and (R("fan", 1).vertex_map == -1).all()
    for name, differs in (("fan", False), ("fan_wide", True)):
        v, mean = cases.CASES[name].vertices.astype(np.float64), R(name, 0)
        forwards, backwards = np.zeros(3), np.zeros(3)
        for row in v:
            forwards = forwards + row
        for row in v[::-1]:
            backwards = backwards + row
        assert mean.vertex_counts.tolist() == [5002] and same((forwards / 5002.0).astype(F).reshape(1, 3), mean.vertices)
        assert same(forwards, backwards) != differs, name          # (the float64 sums; a float32 mean seldom shows their last bits)
    # strip and many_small: more than 1024 clusters and kept faces, so heads and faces cross the tiles; on the strip the numbering by
    # smallest member is not the numbering by key
    strip = R("strip", 0)
    assert strip.stats["clusters"] == 2050 > 1024 and len(strip.faces) == 2048 > 1024 and len(cases.CASES["strip"].vertices) == 4098
    _, by_key = np.unique(strip.key, axis=0, return_inverse=True)
    assert not np.array_equal(by_key.reshape(-1), strip.cluster) and len(np.unique(strip.cluster)) == 2050
    first = np.full(2050, 4098)
    np.minimum.at(first, strip.cluster, np.arange(4098))
    assert (np.diff(first) > 0).all()                            # ascending smallest member
    many = R("many_small", 0)
    assert many.stats["clusters"] > 1024 and len(many.faces) > 1024 and many.stats["unreferenced"] > 0 and len(cases.CASES["many_small"].vertices) == 9006
    assert same(R("strip", 1).vertices, cases.CASES["strip"].vertices) and same(R("many_small", 1).faces, cases.CASES["many_small"].faces)


def test_the_two_sphere_volume():
    m = cases.CASES["two_spheres"]
    assert m.vertices.shape == (3932, 3) and m.faces.shape == (7856, 3)
    for run, (voxel, (nv2, nf2, collapsed, duplicates)) in enumerate(cases.TWO_SPHERES.items()):
        r = cases.result("two_spheres", run)
        assert cases.RUNS["two_spheres"][run] == dict(voxel_size=voxel)
        assert (len(r.vertices), len(r.faces), r.stats["collapsed"], r.stats["duplicates"], r.stats["unreferenced"], r.stats["zero_area"]) == (nv2, nf2, collapsed, duplicates, 0, 0)
    facts = tsdf_ref.mesh_facts(cases.result("two_spheres", 2).vertices, cases.result("two_spheres", 2).faces)
    assert facts["edge_uses"] == {2} and facts["euler"] == 4
    # no two bit-equal vertices, no unreferenced vertex: weld is the identity, in bytes (a fact that needs no restatement)
    assert len(np.unique(m.vertices, axis=0)) == 3932 and len(np.unique(m.faces)) == 3932
    w = cases.result("two_spheres", 3)
    assert same(w.vertices, m.vertices) and same(w.faces, m.faces) and same(w.rows[0], m.colors) and same(w.rows[1], m.attribute)
    assert w.vertex_map.tolist() == list(range(3932)) and w.face_index.tolist() == list(range(7856)) and (w.vertex_counts == 1).all()


def test_the_volume_with_samples_on_its_iso_welds_to_a_mesh_of_the_same_volume():
    m, w = cases.CASES["equal_iso"], cases.result("equal_iso", 0)
    assert cases.RUNS["equal_iso"][0] == cases.W(drop_zero_area=True)
    assert len(w.vertices) < len(m.vertices) and len(np.unique(m.vertices.view(np.uint32), axis=0)) < len(m.vertices)
    canon = w.vertices + F(0)                                    # (-0.0 as +0.0)
    assert len(np.unique(canon.view(np.uint32), axis=0)) == len(w.vertices)          # no two bit-equal vertices
    f = w.faces
    assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])).all() and len(f) < 10 ** 5
    before, after = tsdf_ref.mesh_facts(m.vertices, m.faces)["volume"], tsdf_ref.mesh_facts(w.vertices, f)["volume"]
    print("volume", before, after)
    assert abs(after - before) <= 1e-9 * abs(before) and before != 0


# ---- the properties of any result, here of the restatement's ----
@pytest.mark.parametrize("name", list(cases.CASES))
def test_properties_of_the_restatement(name):
    m = cases.CASES[name]
    for run in cases.runs_of(name):
        options, r = cases.RUNS[name][run], cases.result(name, run)
        cases.check_properties(m, options, r.vertices, r.faces, r.vertex_map, r.vertex_counts)
        if options["voxel_size"] is None or (options.get("contraction") == "first" and options.get("bounds") is not None):          # applied twice equals once
            again = ref.simplify(r.vertices, r.faces, r.rows, **options)
            assert all(same(a, b) for a, b in zip((again.vertices, again.faces, *again.rows), (r.vertices, r.faces, *r.rows))), (name, run)
            assert again.stats["collapsed"] == again.stats["duplicates"] == 0 and (again.vertex_counts == 1).all()


# ---- the refusals that need no device ----
def test_refusals_before_any_pointer_is_looked_at():
    l = MZ.lib()
    box = (C.c_double * 6)(0, 0, 0, 1, 1, 1)

    def refused(rc, word):
        assert rc == 1 and word in l.gp_last_error(), (word, l.gp_last_error())

    def plan(nv=4, nf=2, mode=MZ.GRID, voxel=0.5, bounds=box, contraction=MZ.AVERAGE, vertices=8, faces=8, scratch=8, counts=8):
        return l.gp_mesh_simplify_plan(vertices, faces, nv, nf, mode, voxel, bounds, contraction, 0, 1, 0, scratch, counts, None)

    from gaussianprediction_amd import mesh_ops
    sizes = (((2 ** 31, 4), b"nv must be below 2^31"), ((4, 715827883), b"3*nf must be below 2^31"), ((-1, 4), b">= 0"), ((4, -1), b">= 0"), ((4, 2 ** 40), b"3*nf"))
    for (nv, nf), word in sizes:
        assert l.gp_mesh_simplify_scratch_bytes(nv, nf) == -1 and word in l.gp_last_error()
        assert mesh_ops.check_sizes(nv, nf).encode() in l.gp_last_error()          # gp_mesh.h's words
        refused(plan(nv, nf), word)
        refused(l.gp_mesh_simplify_apply(8, nv, nf, 8, 8, 8, 8, 8, 8, None), word)
        refused(l.gp_mesh_simplify_rows(8, nv, nf, 3, 0, 8, 8, None), word)
    refused(l.gp_mesh_simplify_bounds(8, 2 ** 31, 8, 8, None), b"nv must be below 2^31")
    refused(l.gp_mesh_simplify_bounds(8, 0, 8, 8, None), b"nv must be >= 1")
    for args, word in (((None, 4, 8, 8), b"null"), ((8, 4, None, 8), b"null"), ((8, 4, 8, None), b"null"), ((8, 4, 12, 8), b"aligned"), ((8, 4, 8, 12), b"aligned")):
        refused(l.gp_mesh_simplify_bounds(*args, None), word)
    assert l.gp_mesh_simplify_scratch_bytes(0, 0) > 0 and l.gp_mesh_simplify_scratch_bytes(2 ** 31 - 1, 715827882) > 48 * (2 ** 31 - 1)
    for kw, word in ((dict(voxel=0.0), b"finite and > 0"), (dict(voxel=-1.0), b"finite and > 0"), (dict(voxel=float("nan")), b"finite and > 0"),
                     (dict(voxel=float("inf")), b"finite and > 0"), (dict(voxel=2.0 ** -21), b"voxel_size is too small"), (dict(bounds=None), b"null"),
                     (dict(bounds=(C.c_double * 6)(0, 0, 0, 1, float("nan"), 1)), b"bounds must be finite"), (dict(bounds=(C.c_double * 6)(0, 2, 0, 1, 1, 1)), b"bounds must be finite"),
                     (dict(mode=2), b"mode must be"), (dict(contraction=2), b"contraction must be"), (dict(vertices=None), b"null"), (dict(faces=None), b"null"),
                     (dict(scratch=None), b"null"), (dict(counts=None), b"null"), (dict(scratch=12), b"aligned")):
        refused(plan(**kw), word)
    refused(plan(mode=MZ.WELD, voxel=-1.0, bounds=None, contraction=7, counts=None), b"gp_mesh_simplify_plan: null argument")          # weld looks at none of the three
    for args, word in (((None, 4, 2, 8, 8, 8, 8, 8, 8), b"null"), ((8, 4, 2, None, 8, 8, 8, 8, 8), b"null"), ((8, 4, 2, 8, None, 8, 8, 8, 8), b"null"),
                       ((8, 4, 2, 8, 8, None, 8, 8, 8), b"null"), ((8, 4, 2, 8, 8, 8, None, 8, 8), b"null"), ((8, 4, 2, 8, 8, 8, 8, None, 8), b"null"),
                       ((8, 4, 2, 8, 8, 8, 8, 8, None), b"null"), ((8, 4, 2, 4, 8, 8, 8, 8, 8), b"aligned")):
        refused(l.gp_mesh_simplify_apply(*args, None), word)
    for args, word in (((8, 4, 2, 0, 0, 8, 8), b"k must be"), ((8, 4, 2, 1025, 0, 8, 8), b"k must be"), ((8, 2 ** 22, 2, 1024, 0, 8, 8), b"nv*k"), ((8, 4, 2, 3, 2, 8, 8), b"contraction must be"),
                       ((None, 4, 2, 3, 0, 8, 8), b"null"), ((8, 4, 2, 3, 0, None, 8), b"null"), ((8, 4, 2, 3, 0, 8, None), b"null")):
        refused(l.gp_mesh_simplify_rows(*args, None), word)


def test_the_python_surface_refuses_before_the_device(monkeypatch):
    monkeypatch.setattr(MZ, "lib", lambda: pytest.fail("a launch was reached"))
    faces, vertices = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, 3)
    mesh = Mesh(vertices, faces, None)
    for call in (lambda: MZ.weld(mesh), lambda: MZ.simplify(mesh, 0.5), lambda: MZ.simplify(mesh, 0.5, "first", ((0, 0, 0), (1, 1, 1)))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for call, word in ((lambda: MZ.weld(Mesh(vertices, faces.long(), None)), "int32"), (lambda: MZ.weld(Mesh(vertices, faces[:, :2], None)), r"\[Nf, 3\]"),
                       (lambda: MZ.simplify(Mesh(vertices[0], faces, None), 0.5), r"\[Nv, 3\]")):
        with pytest.raises(RuntimeError, match=word):
            call()
    for call, word in ((lambda: MZ.simplify(mesh, 0.0), "finite and > 0"), (lambda: MZ.simplify(mesh, float("nan")), "finite and > 0"), (lambda: MZ.simplify(mesh, -2), "finite and > 0"),
                       (lambda: MZ.simplify(mesh, 2.0 ** -21, bounds=((0, 0, 0), (1, 1, 1))), "voxel_size is too small"),
                       (lambda: MZ.simplify(mesh, 0.5, bounds=((0, 0, 0), (1, float("inf"), 1))), "bounds must be finite"),
                       (lambda: MZ.simplify(mesh, 0.5, bounds=((0, 3, 0), (1, 1, 1))), "min <= max"), (lambda: MZ.simplify(mesh, 0.5, contraction="median"), "contraction must be")):
        with pytest.raises(_lib.GpHipError, match=word):
            call()
    assert MZ.check_voxel(0.5) is None and MZ.check_voxel(0.5, ((0, 0, 0), (1, 1, 1))) is None and MZ.check_voxel(0) == "voxel_size must be finite and > 0"
    assert MZ.check_voxel(1e-7, ((0, 0, 0), (1, 1, 1))) == "voxel_size is too small" and MZ.check_voxel(2.0 ** -20, ((0, 0, 0), (1, 1, 1))) is None


def test_signatures_and_docstrings():
    from gaussianprediction_amd import eval_render as ER
    sig = inspect.signature(MZ.weld)
    assert list(sig.parameters) == ["mesh", "drop_zero_area", "drop_duplicates", "keep_unreferenced", "attributes"]
    assert [p.default for p in sig.parameters.values()][1:] == [False, True, False, ()]
    sig = inspect.signature(MZ.simplify)
    assert list(sig.parameters) == ["mesh", "voxel_size", "contraction", "bounds", "drop_zero_area", "drop_duplicates", "keep_unreferenced", "attributes"]
    assert [p.default for p in sig.parameters.values()][2:] == ["average", None, False, True, False, ()]
    assert list(inspect.signature(MZ.check_voxel).parameters) == ["voxel_size", "bounds"]
    sig = inspect.signature(ER.render_meshes)
    names = list(sig.parameters)
    assert names[:9] == ["model_path", "name", "iteration", "views", "gaussians", "pipeline", "background", "times", "resolution"]
    assert names[-3:] == ["min_triangles", "keep_largest", "normals"] and names[names.index("color") + 1:-3] == ["weld", "simplify_voxel", "simplify_contraction"]
    assert [sig.parameters[k].default for k in ("weld", "simplify_voxel", "simplify_contraction")] == [False, None, "average"]
    assert open(ER.__file__).read().count("render_meshes(") == 1
    assert "One read" in MZ.weld.__doc__ and "Two reads" in MZ.simplify.__doc__ and "one read with `bounds` given" in " ".join(MZ.simplify.__doc__.split())
