"""No GPU: csrc/gp_mesh.h against the binding's table (a binding outside _lib.ABIS); the programs of csrc/mesh_core.h in a stand-alone
build (tests/mesh_emulate.cpp, under the sanitizers where the host compiler can link them) against the numpy restatement
tests/mesh_ref.py on every case of tests/mesh_cases.py -- bit for bit for labels, the table, the filter's indices, faces and rows
and the normals; the rounds of the path case under its cap; face indices out of range under the sanitizers; the restatement against
the facts of the two-sphere volume; the mesh PLY files with normals; the refusals that need no device."""
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
import mesh_cases as cases
import mesh_ref as ref
import tsdf_ref
from gaussianprediction_amd import _lib, io_formats, mesh_ops as MO
from gaussianprediction_amd.tsdf_ops import Mesh

_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "gp_stream_t": _lib.Ptr}
_POINTEES = {"float", "int32_t", "void"}
F = np.float32
I = np.int32


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the header, the table, the registry ----
def test_prototype_table_equals_the_header_and_stays_out_of_the_registry():
    before = len(_lib.ABIS)
    protos = abi_check.check_table(MO.ABI, 7, _SCALARS, _POINTEES)
    assert MO.ABI.prototypes is MO.PROTOTYPES and MO.ABI not in _lib.ABIS and len(_lib.ABIS) == before
    assert os.path.samefile(os.path.join(abi_check.ROOT, "include", MO.ABI.header), os.path.join(abi_check.ROOT, "gaussianprediction_amd", "csrc", "gp_mesh.h"))
    for name in ("gp_mesh_components", "gp_mesh_filter_plan", "gp_mesh_filter_apply", "gp_mesh_gather_rows", "gp_mesh_vertex_normals"):
        assert protos[name][1][-1] == "gp_stream_t"              # the stream is the last parameter
    assert not os.path.exists(os.path.join(abi_check.ROOT, "include", "gp_mesh.h"))
    assert len([h for h in os.listdir(os.path.join(abi_check.ROOT, "include")) if h.endswith(".h")]) == 12      # include/ stays at its twelve


def test_symbols_and_constants():
    text = abi_check.header_text(MO.HEADER)
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_MESH_[A-Z0-9_]+) +(\d+)", text)}
    assert defs["GP_MESH_ABI_VERSION"] == MO.GP_MESH_ABI_VERSION == MO.ABI.version == 1
    assert (defs["GP_MESH_TILE"], defs["GP_MESH_HOPS"], defs["GP_MESH_MAX_ROUNDS"]) == (MO.TILE, MO.HOPS, MO.MAX_ROUNDS) == (1024, 4, 64)
    assert [defs["GP_MESH_" + n] for n in ("STATUS", "CONVERGED", "COUNT", "ROUNDS", "STATE_WORDS")] == [MO.STATUS, MO.CONVERGED, MO.COUNT, MO.ROUNDS, MO.STATE_WORDS]
    assert 1 <= MO.ROUNDS_PER_READ <= MO.MAX_ROUNDS
    abi_check.check_applied(MO.ABI)
    assert MO.Components._fields[:5] == ("vertex_label", "face_label", "labels", "vertex_counts", "face_counts")
    assert MO.Filtered._fields[:3] == ("mesh", "vertex_index", "face_index") and Mesh._fields == ("vertices", "faces", "colors")


# ---- the programs in a stand-alone build, under the sanitizers ----
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    d = tmp_path_factory.mktemp("mesh_emulate")
    exe = emulate_build.build("mesh_emulate", d, sanitize=True)

    def run(head, arrays):
        job, out = str(d / "job.bin"), str(d / "out.bin")
        with open(job, "wb") as fp:
            fp.write(head)
            for a in arrays:
                fp.write(np.ascontiguousarray(a).tobytes())
        subprocess.check_call([exe, job, out], timeout=300)
        return open(out, "rb").read()

    return run


def emulated_components(emulator, faces, nv):
    nf = len(faces)
    raw = emulator(struct.pack("<iii", 0, nv, nf), [faces])
    state = np.frombuffer(raw, I, 4)
    count = int(state[MO.COUNT])
    assert len(raw) == 4 * (4 + nv + nf + 3 * count)
    parts = np.split(np.frombuffer(raw, I, nv + nf + 3 * count, 16), np.cumsum([nv, nf, count, count]))
    return state, parts


def emulated_filter(emulator, m, comps, min_triangles, keep_largest):
    _, vertex_label, _, labels, _, face_counts = comps
    nv, nf, rows = len(m.vertices), len(m.faces), np.concatenate([m.vertices, m.colors, m.attribute], axis=1)
    k = rows.shape[1]
    raw = emulator(struct.pack("<iiiiiii", 1, nv, nf, len(labels), -1 if min_triangles is None else min_triangles, -1 if keep_largest is None else keep_largest, k),
                   [m.faces, vertex_label, labels, face_counts, rows])
    status, nv2, nf2 = np.frombuffer(raw, I, 3).tolist()
    assert len(raw) == 4 * (3 + nv2 + nf2 + 3 * nf2 + k * nv2)
    ints = np.frombuffer(raw, I, nv2 + 4 * nf2, 12)
    rows2 = np.frombuffer(raw, F, k * nv2, 12 + 4 * (nv2 + 4 * nf2)).reshape(nv2, k)
    return status, rows2[:, :3], ints[nv2 + nf2:].reshape(nf2, 3), ints[:nv2], ints[nv2:nv2 + nf2], [rows2[:, 3:6], rows2[:, 6:]]


def emulated_normals(emulator, vertices, faces):
    raw = emulator(struct.pack("<iii", 2, len(vertices), len(faces)), [vertices, faces])
    assert len(raw) == 4 + 12 * len(vertices)
    return int(np.frombuffer(raw, I, 1)[0]), np.frombuffer(raw, F, 3 * len(vertices), 4).reshape(-1, 3)


def check_filtered(got, want):
    assert got[0] == want[0]
    for g, w in zip(got[1:5], want[1:5]):
        assert same(g, w)
    assert len(got[5]) == len(want[5]) and all(same(g, w) for g, w in zip(got[5], want[5]))


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_emulated_components_against_the_restatement(emulator, name):
    m = cases.CASES[name]
    state, parts = emulated_components(emulator, m.faces, len(m.vertices))
    want = cases.components(name)
    print(name, "rounds", int(state[MO.ROUNDS]), "components", int(state[MO.COUNT]))
    assert state[MO.STATUS] == want[0] == 0 and state[MO.CONVERGED] == 1 and state[MO.COUNT] == len(want[3])
    assert all(same(g, w) for g, w in zip(parts, want[1:]))
    if name == "strip":                                          # synchronous rounds: a scheme bound by the diameter needs about 2048
        assert int(state[MO.ROUNDS]) <= cases.STRIP_CAP == 60


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_emulated_filter_and_normals_against_the_restatement(emulator, name):
    m = cases.CASES[name]
    for min_triangles, keep_largest in cases.filters_of(name):
        check_filtered(emulated_filter(emulator, m, cases.components(name), min_triangles, keep_largest), cases.filtered(name, min_triangles, keep_largest))
    status, normals = emulated_normals(emulator, m.vertices, m.faces)
    assert status == 0 and same(normals, cases.normals(name)) and np.isfinite(normals).all()


@pytest.mark.parametrize("case, face, corner, value", cases.BAD)
def test_the_emulator_skips_and_reports_a_face_index_out_of_range(emulator, case, face, corner, value):
    """Under the sanitizers every array has its exact size: an index dereferenced without its check ends the child."""
    m = cases.CASES[case]
    nv, faces = len(m.vertices), cases.bad_faces(case, face, corner, value)
    assert not ref.good_faces(faces, nv)[face] and ref.good_faces(faces, nv).sum() == len(faces) - 1
    state, parts = emulated_components(emulator, faces, nv)
    want = ref.components(faces, nv)
    assert state[MO.STATUS] == want[0] == 1 and all(same(g, w) for g, w in zip(parts, want[1:])) and parts[1][face] == -1
    bad = type(m)(**{**vars(m), "faces": faces})
    got = emulated_filter(emulator, bad, want, None, None)
    check_filtered(got, ref.filter_components(m.vertices, faces, [m.colors, m.attribute]))
    assert got[0] == 1 and face not in got[4]
    status, normals = emulated_normals(emulator, m.vertices, faces)
    assert status == 1 and same(normals, ref.vertex_normals(m.vertices, faces))
    # labels handed in from elsewhere are checked too
    stray = (want[0], np.full(nv, nv, I)) + want[2:]
    assert emulated_filter(emulator, bad, stray, None, None)[0] == 1


# ---- the cases reach what they are for; the restatement against independent facts ----
def test_the_cases_reach_what_they_are_for():
    X, N = cases.components, cases.normals
    assert [len(X(n)[3]) for n in ("empty", "no_faces", "one_triangle", "two_disjoint", "shared_vertex", "repeated_index")] == [0, 5, 1, 2, 2, 1]
    assert X("no_faces")[5].tolist() == [0] * 5 and X("shared_vertex")[3].tolist() == [0, 5] and X("shared_vertex")[5].tolist() == [2, 0]
    assert X("two_disjoint")[2].tolist() == [3, 0] and X("repeated_index")[3].tolist() == [0] and X("repeated_index")[4].tolist() == [4]
    assert same(N("collinear"), np.zeros((4, 3), F)) and same(N("overflow"), np.zeros((4, 3), F))
    strip = cases.CASES["strip"]
    assert strip.faces.shape == (4096, 3) and len(strip.vertices) == 4098 and X("strip")[3].tolist() == [0] and X("strip")[5].tolist() == [4096]
    assert (N("strip")[:, 2] < -0.5).all()                      # consistently wound
    fan = cases.CASES["fan"]
    assert fan.faces.shape == (5000, 3) and (fan.faces[:, 0] == 0).all() and np.isclose(np.linalg.norm(N("fan"), axis=1), 1, atol=1e-6).all()
    # the fan's centre: 5000 float32 additions in THIS order; another order gives other bits
    fv = ref.face_vectors(fan.vertices, fan.faces)
    backwards = np.zeros(3, F)
    for row in fv[::-1]:
        backwards = backwards + row
    forwards = np.zeros(3, F)
    for row in fv:
        forwards = forwards + row
    assert not same(backwards, forwards) and same(forwards / np.sqrt((forwards[0] * forwards[0] + forwards[1] * forwards[1]) + forwards[2] * forwards[2]), N("fan")[0])
    many = cases.CASES["many_small"]
    assert len(X("many_small")[3]) == 3001 > 1024 and len(many.vertices) == 9006 and X("many_small")[5].tolist() == [1] * 3000 + [8]
    octa = cases.filtered("many_small", None, 1)
    assert octa[3].tolist() == list(range(9000, 9006)) and same(octa[2], cases.OCTAHEDRON[1]) and octa[4].tolist() == list(range(3000, 3008))
    tie = cases.filtered("many_small", None, 2)                 # the tie among 3000 single triangles goes to label 0
    assert tie[3].tolist() == [0, 1, 2] + list(range(9000, 9006)) and tie[4].tolist() == [0] + list(range(3000, 3008))
    check_filtered(cases.filtered("many_small", 2, None), octa)
    assert len(cases.filtered("many_small", 1, 5)[4]) == 12 and len(cases.filtered("many_small", None, 0)[3]) == 0
    assert len(cases.filtered("fan", 5001, None)[3]) == 0 and len(cases.filtered("shared_vertex", None, None)[3]) == 5


def test_the_two_sphere_volume():
    m = cases.CASES["two_spheres"]
    assert m.vertices.shape == (3932, 3) and m.faces.shape == (7856, 3)
    _, vertex_label, face_label, labels, vertex_counts, face_counts = cases.components("two_spheres")
    assert labels.tolist() == [0, 1382] and vertex_counts.tolist() == [3630, 302] and face_counts.tolist() == [7256, 600]
    facts = tsdf_ref.mesh_facts(m.vertices, m.faces)
    assert facts["edge_uses"] == {2} and facts["euler"] == 4
    status, vertices, faces, vertex_index, face_index, rows = cases.filtered("two_spheres", None, 1)
    assert status == 0 and vertices.shape == (3630, 3) and faces.shape == (7256, 3)
    facts = tsdf_ref.mesh_facts(vertices, faces)
    assert facts["edge_uses"] == {2} and facts["euler"] == 2 and facts["unreferenced"] == 0 and facts["volume"] > 0
    assert same(vertices, m.vertices[vertex_index]) and same(rows[0], m.colors[vertex_index]) and (np.diff(vertex_index) > 0).all() and (np.diff(face_index) > 0).all()
    normals = ref.vertex_normals(vertices, faces)
    assert ((normals.astype(np.float64) * (vertices.astype(np.float64) - np.array(cases.TWO_SPHERES.c0))).sum(axis=1) > 0).all()
    check_filtered(cases.filtered("two_spheres", 601, None), cases.filtered("two_spheres", None, 1))
    assert len(cases.filtered("two_spheres", 600, 2)[4]) == 7856
    both = cases.normals("two_spheres")
    centre = np.where((vertex_label == 0)[:, None], np.array(cases.TWO_SPHERES.c0), np.array(cases.TWO_SPHERES.c1))
    assert ((both.astype(np.float64) * (m.vertices.astype(np.float64) - centre)).sum(axis=1) > 0).all()


# ---- mesh PLY files with normals ----
def test_mesh_ply_with_normals(tmp_path):
    m = cases.CASES["shared_vertex"]
    normals = cases.normals("shared_vertex")
    path, plain = str(tmp_path / "deep" / "mesh.ply"), str(tmp_path / "plain.ply")
    nv, nf = len(m.vertices), len(m.faces)
    io_formats.save_mesh_ply_normals(path, m.vertices, m.faces, normals, m.colors)
    raw = open(path, "rb").read()
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\n"
              "property float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n"
              % (nv, nf)).encode()
    assert raw.startswith(header) and len(raw) == len(header) + 27 * nv + 13 * nf
    assert raw[len(header):len(header) + 24] == m.vertices[0].tobytes() + normals[0].tobytes()
    v, f, c, n = io_formats.read_mesh_ply(path, normals=True)
    assert same(v, m.vertices) and same(f, m.faces) and same(c, io_formats.color_to_uint8(m.colors)) and same(n, normals)
    assert len(io_formats.read_mesh_ply(path)) == 3 and same(io_formats.read_mesh_ply(path)[0], m.vertices)
    io_formats.save_mesh_ply_normals(path, torch.from_numpy(m.vertices), torch.from_numpy(m.faces), torch.from_numpy(normals))      # tensors pass alike, no colours
    v, f, c, n = io_formats.read_mesh_ply(path, normals=True)
    assert c is None and same(n, normals) and same(v, m.vertices)
    # without normals: the bytes of the writer as it was
    io_formats.save_mesh_ply(plain, m.vertices, m.faces, m.colors)
    io_formats.save_mesh_ply_normals(path, m.vertices, m.faces, None, m.colors)
    old_header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n"
                  "property uchar green\nproperty uchar blue\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n" % (nv, nf)).encode()
    rows = np.empty(nf, dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    rows["n"], rows["v"] = 3, m.faces
    table = b"".join(m.vertices[k].tobytes() + io_formats.color_to_uint8(m.colors)[k].tobytes() for k in range(nv))
    assert open(plain, "rb").read() == open(path, "rb").read() == old_header + table + rows.tobytes()
    v, f, c, n = io_formats.read_mesh_ply(plain, normals=True)
    assert n is None and same(v, m.vertices) and len(io_formats.read_mesh_ply(plain)) == 3
    with pytest.raises(ValueError, match="normals"):
        io_formats.save_mesh_ply_normals(path, m.vertices, m.faces, normals[:-1])


# ---- the refusals that need no device ----
def test_refusals_before_any_pointer_is_looked_at():
    l = MO.lib()

    def refused(rc, word):
        assert rc == 1 and word in l.gp_last_error(), (word, l.gp_last_error())

    sizes = (((2 ** 31, 4), b"nv must be below 2^31"), ((4, 715827883), b"3*nf must be below 2^31"), ((-1, 4), b">= 0"), ((4, -1), b">= 0"), ((4, 2 ** 40), b"3*nf"))
    for (nv, nf), word in sizes:
        assert l.gp_mesh_scratch_bytes(nv, nf) == -1 and word in l.gp_last_error()
        assert MO.check_sizes(nv, nf).encode() in l.gp_last_error()
        refused(l.gp_mesh_components(8, nv, nf, 4, 1, 8, 8, 8, 8, 8, None), word)
        refused(l.gp_mesh_filter_plan(8, nv, nf, 8, 8, 8, 1, -1, -1, 8, 8, None), word)
        refused(l.gp_mesh_filter_apply(8, nv, nf, 8, 8, 8, 8, None), word)
        refused(l.gp_mesh_vertex_normals(8, 8, nv, nf, 8, 8, 8, None), word)
    assert MO.check_sizes(2 ** 31 - 1, 715827882) is None and MO.check_sizes(0, 0) is None
    assert l.gp_mesh_scratch_bytes(0, 0) > 0 and l.gp_mesh_scratch_bytes(2 ** 31 - 1, 715827882) > 48 * 715827882
    for args, word in (((8, 4, 2, 0, 1, 8, 8, 8, 8, 8), b"rounds must be"), ((8, 4, 2, 65, 1, 8, 8, 8, 8, 8), b"rounds must be"), ((8, 4, 2, 4, 1, 8, 8, 8, None, 8), b"null"),
                       ((8, 4, 2, 4, 1, 8, 8, 8, 10, 8), b"aligned"), ((None, 4, 2, 4, 1, 8, 8, 8, 8, 8), b"null"), ((8, 4, 2, 4, 1, None, 8, 8, 8, 8), b"null"),
                       ((8, 4, 2, 4, 1, 8, None, 8, 8, 8), b"null"), ((8, 4, 2, 4, 1, 8, 8, None, 8, 8), b"null"), ((8, 4, 2, 4, 1, 8, 8, 8, 8, None), b"null")):
        refused(l.gp_mesh_components(*args, None), word)
    for args, word in (((8, 4, 2, 8, 8, 8, 5, -1, -1, 8, 8), b"components must be"), ((8, 4, 2, 8, 8, 8, -1, -1, -1, 8, 8), b"components must be"),
                       ((8, 4, 2, 8, 8, 8, 1, -1, -1, 8, None), b"null"), ((8, 4, 2, None, 8, 8, 1, -1, -1, 8, 8), b"null"), ((8, 4, 2, 8, None, 8, 1, -1, -1, 8, 8), b"null"),
                       ((8, 4, 2, 8, 8, 8, 1, -1, -1, None, 8), b"null"), ((8, 4, 2, 8, 8, 8, 1, -1, -1, 6, 8), b"aligned")):
        refused(l.gp_mesh_filter_plan(*args, None), word)
    for args, word in (((8, 4, 2, None, 8, 8, 8), b"null"), ((8, 4, 2, 8, None, 8, 8), b"null"), ((8, 4, 2, 8, 8, None, 8), b"null"), ((8, 4, 2, 8, 8, 8, None), b"null")):
        refused(l.gp_mesh_filter_apply(*args, None), word)
    for args, word in (((8, 4, 0, 8, 8), b"k must be"), ((8, 4, 1025, 8, 8), b"k must be"), ((8, 2 ** 22, 1024, 8, 8), b"nv*k"), ((None, 4, 3, 8, 8), b"null"), ((8, 4, 3, None, 8), b"null"),
                       ((8, 4, 3, 8, None), b"null")):
        refused(l.gp_mesh_gather_rows(*args, None), word)
    for args, word in (((None, 8, 4, 2, 8, 8, 8), b"null"), ((8, None, 4, 2, 8, 8, 8), b"null"), ((8, 8, 4, 2, None, 8, 8), b"null"), ((8, 8, 4, 2, 8, None, 8), b"null")):
        refused(l.gp_mesh_vertex_normals(*args, None), word)


def test_the_python_surface_refuses_before_the_device(monkeypatch):
    monkeypatch.setattr(MO, "lib", lambda: pytest.fail("a launch was reached"))
    faces, vertices = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, 3)
    for call in (lambda: MO.connected_components(faces, 4), lambda: MO.filter_components(Mesh(vertices, faces, None)), lambda: MO.vertex_normals(vertices, faces),
                 lambda: MO.clean(Mesh(vertices, faces, None), keep_largest=1, normals=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for call, word in ((lambda: MO.connected_components(faces.long(), 4), "int32"), (lambda: MO.connected_components(faces[:, :2], 4), r"\[Nf, 3\]"),
                       (lambda: MO.vertex_normals(vertices[0], faces), r"\[Nv, 3\]")):
        with pytest.raises(RuntimeError, match=word):
            call()
    assert MO.check_sizes(-1, 0) == "nv and nf must be >= 0"


def test_signatures_and_docstrings():
    from gaussianprediction_amd import eval_render as ER
    assert list(inspect.signature(MO.connected_components).parameters)[:2] == ["faces", "n_vertices"]
    assert list(inspect.signature(MO.filter_components).parameters) == ["mesh", "min_triangles", "keep_largest", "components", "attributes"]
    assert list(inspect.signature(MO.vertex_normals).parameters)[:2] == ["vertices", "faces"]
    assert list(inspect.signature(MO.clean).parameters) == ["mesh", "min_triangles", "keep_largest", "normals"]
    assert [p.default for p in inspect.signature(MO.clean).parameters.values()][1:] == [None, None, False]
    sig = inspect.signature(ER.render_meshes)
    assert list(sig.parameters)[-3:] == ["min_triangles", "keep_largest", "normals"]
    assert [sig.parameters[k].default for k in ("min_triangles", "keep_largest", "normals")] == [None, None, False]
    assert inspect.signature(io_formats.read_mesh_ply).parameters["normals"].default is False
    assert list(inspect.signature(io_formats.save_mesh_ply_normals).parameters) == ["path", "vertices", "faces", "normals", "colors"]
    doc = " ".join(MO.connected_components.__doc__.split())
    assert "one read per 12 rounds" in doc and MO.ROUNDS_PER_READ == 12 and "Nothing is read" in MO.vertex_normals.__doc__ and "One read" in MO.filter_components.__doc__
