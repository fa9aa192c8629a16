"""No GPU: csrc/gp_volume.h against the binding's table (a binding outside _lib.ABIS); the programs of csrc/volume_core.h in a
stand-alone build (tests/volume_emulate.cpp, under the sanitizers where the host compiler can link them) against the numpy restatement
tests/volume_ref.py -- a brute force with no tree -- bit for bit on every case of tests/volume_cases.py, for leaves of 1, 2, 4 and 8
records and for the faces in reversed order; the lattice, the comparison, foreign input, the refusals that need no device,
lattice_for's rule, and the requirement that the tree tests fewer boxes and records than the grid tests records where the queries lie
deep inside or far outside."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import abi_check
import sdf_ref
import surface_cases
import volume_cases as cases
import volume_ref as ref
from gaussianprediction_amd import _lib, geometry_ops as G, mesh_smooth as MS, sdf_ops as D, surface_ops as S, tsdf_ops as T, volume_ops as V

_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "gp_stream_t": _lib.Ptr}
_POINTEES = {"float", "double", "int32_t", "int64_t", "void"}
F = np.float32
I = np.int32
same = cases.same


# ---- the header, the table, the registry ----
def test_prototype_table_equals_the_header_and_stays_out_of_the_registry():
    before = len(_lib.ABIS)
    protos = abi_check.check_table(V.ABI, 6, _SCALARS, _POINTEES)
    assert V.ABI.prototypes is V.PROTOTYPES and V.ABI not in _lib.ABIS and D.ABI not in _lib.ABIS and S.ABI not in _lib.ABIS and MS.ABI not in _lib.ABIS and len(_lib.ABIS) == before
    assert os.path.samefile(os.path.join(abi_check.ROOT, "include", V.ABI.header), os.path.join(abi_check.ROOT, "gaussianprediction_amd", "csrc", "gp_volume.h"))
    for name in ("gp_volume_tree", "gp_volume_query", "gp_volume_lattice", "gp_volume_compare"):
        assert protos[name][1][-1] == "gp_stream_t"              # the stream is the last parameter
    assert not os.path.exists(os.path.join(abi_check.ROOT, "include", "gp_volume.h"))
    assert len([h for h in os.listdir(os.path.join(abi_check.ROOT, "include")) if h.endswith(".h")]) == 12      # include/ stays at its twelve


def test_symbols_and_constants():
    text = abi_check.header_text(V.HEADER)
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_VOLUME_[A-Z0-9_]+) +(\d+)", text)}
    assert defs["GP_VOLUME_ABI_VERSION"] == V.GP_VOLUME_ABI_VERSION == V.ABI.version == 1
    assert defs["GP_VOLUME_LEAF"] == V.LEAF == ref.LEAF and defs["GP_VOLUME_STACK"] == V.STACK >= defs["GP_VOLUME_MAX_LEVELS"] + 1
    for name in ("STAT_WORDS", "LATTICE_WORDS", "COUNT_WORDS"):
        assert defs["GP_VOLUME_" + name] == getattr(V, name) == getattr(ref, name), name
    assert [defs["GP_VOLUME_" + n.upper()] for n in V.STAT_NAMES] == list(range(8)) and V.STAT_NAMES == ref.STAT_NAMES
    assert [defs["GP_VOLUME_" + n.upper()] for n in V.COUNT_NAMES] == list(range(6)) and V.COUNT_NAMES == ref.COUNT_NAMES
    assert V.LATTICE_WORDS == V.STAT_WORDS + D.STAT_WORDS and V.LATTICE_NAMES[:8] == V.STAT_NAMES and V.LATTICE_NAMES[8:15] == D.STAT_NAMES[:7]
    raw = open(os.path.join(abi_check.ROOT, "include", V.HEADER)).read()
    for words in ("lb * (1 - 2^-40) > best", "2^-47 * M", "lb >= 2^-100", "Why the rule is exact", "equal bounds go to the lower index", "fmaf((float)i, voxel, ox)",
                  "gp_surface.h section 1, unchanged"):
        assert words in raw, words                                # the rule and its proof stand in the header
    abi_check.check_applied(V.ABI)
    source = open(os.path.join(abi_check.ROOT, "gaussianprediction_amd", "csrc", "volume_kernels.hip")).read()
    assert '#include "volume_core.h"' in source and "atomicAdd(" in source and "gp_radix_sort_pairs(" in source
    assert not re.search(r"atomic\w*\(\s*\(?(float|double)", source) and "hipMemcpy(" not in source and "Synchronize" not in source      # no float atomics, no read
    core = open(os.path.join(abi_check.ROOT, "gaussianprediction_amd", "csrc", "volume_core.h")).read()
    assert '#include "sdf_core.h"' in core and "sf_test(" in core and "sd_sign(" in core and "sf_record" in source + core      # the arithmetic is reused, not restated
    for restated in ("sf_dot(", "sf_cross(", "sf_edge(", "sf_interior(", "sqrt(", "atan2("):
        assert restated not in core, restated
    import __graft_entry__ as entry
    assert "volume_kernels.hip" in entry.HIP_SOURCES and "-ffp-contract=off" in entry.HIP_FLAGS


# ---- the programs in a stand-alone build, under the sanitizers ----
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return cases.build_emulator(tmp_path_factory.mktemp("volume_emulate"), sanitize=True)


def test_the_emulator_is_its_own_program():
    text = open(os.path.join(abi_check.ROOT, "tests", "volume_emulate.cpp")).read()
    assert '#include "../gaussianprediction_amd/csrc/volume_core.h"' in text and "int main(int argc" in text
    driver = inspect.getsource(cases.build_emulator)
    assert 'emulate_build.build("volume_emulate"' in driver and "subprocess.run([exe" in driver          # a child process: nothing is loaded into Python
    assert "sanitize=True" in inspect.getsource(emulator)


def check_stats(name, stats, nf, leaf, want):
    levels, leaves = ref.levels(nf, leaf)
    assert stats[ref.LEVELS] == levels and stats[ref.LEAVES] == leaves and stats[ref.STATUS] == 0, (name, stats)
    assert stats[ref.EXCLUDED_FACES] == want.excluded_faces and stats[ref.EXCLUDED_QUERIES] == want.excluded_queries, (name, stats)
    assert stats[ref.MAX_STACK] <= levels + 1 <= V.STACK and stats[ref.CANDIDATES] <= (len(want.face) - want.excluded_queries) * nf        # every record once at the most
    assert stats[ref.NODES] <= (len(want.face) - want.excluded_queries) * (2 * leaves + levels)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_emulated_tree_against_the_restatement(emulator, name):
    v, f, q = cases.CASES[name]
    want = cases.result(name)
    seen = {}
    for leaf in cases.LEAVES:
        got = emulator.run(v, f, q, leaf=leaf)
        assert all(cases.equal_result(got.row, want)), (name, leaf, cases.equal_result(got.row, want))
        check_stats(name, got.stats, len(f), leaf, want)
        seen[leaf] = (int(got.stats[ref.NODES]), int(got.stats[ref.CANDIDATES]))
    print(name, "nodes, candidates by leaf:", seen)
    # the faces in reversed order: equal dist2 everywhere, the mapped face where one face wins alone, the smaller NEW number where several tie
    nf = len(f)
    got = emulator.run(v, f[::-1].copy(), q)
    assert same(got.dist2, want.dist2), name
    alone = np.array([i not in want.ties for i in range(len(q))], bool) & (want.face >= 0)
    mapped = np.where(want.face >= 0, nf - 1 - want.face, -1).astype(I)
    assert same(got.face[alone], mapped[alone]) and same(got.region[alone], want.region[alone]) and same(got.closest[alone], want.closest[alone]) and same(got.bary[alone], want.bary[alone])
    for i, tied in want.ties.items():
        assert got.face[i] == nf - 1 - int(np.max(tied)), (name, i, tied)
    assert same(got.face[want.face < 0], want.face[want.face < 0])


def test_the_cases_reach_what_they_are_for(emulator):
    for name in ("same_faces", "surface/identical"):
        want = cases.result(name)
        assert len(want.ties) > 0 and all(want.face[i] == min(t) for i, t in want.ties.items())          # ties go to the smallest face
    assert (cases.result("same_faces").face == 0).all()
    assert (cases.result("unusable").face == -1).all() and cases.result("unusable").excluded_faces == 10
    assert (cases.result("nf_0").face == -1).all()
    for name in cases.DEEP:
        v, f, q = cases.CASES[name]
        want = cases.result(name)
        assert want.excluded_queries == 4 and np.isfinite(want.dist2[:-6]).all() and np.isfinite(want.dist2[-2:]).all() and len(q) == 1 + 64 + 7 + 24 + 6
    far = cases.CASES["far"]
    assert np.abs(far[0][np.isfinite(far[0]).all(axis=1)]).max() > 9e5
    assert [ref.levels(nf) for nf in (0, 1, 3, 4, 5, 63, 65, 257)] == [(1, 1), (1, 1), (2, 2), (2, 2), (3, 3), (6, 32), (7, 33), (9, 129)]
    assert ref.levels(2 ** 26 - 1, 1)[0] == 27 == V.STACK - 5
    sparse = emulator.run(*cases.CASES["sparse"])
    assert sparse.stats[ref.CANDIDATES] < 0.5 * 100 * len(cases.CASES["sparse"][2])                       # most boxes are skipped


@pytest.mark.parametrize("name", list(cases.LATTICES))
def test_the_emulated_lattice_against_the_restatement_and_the_query(emulator, name):
    v, f, origin, voxel, dims = cases.LATTICES[name]
    want = cases.lattice(name)
    for leaf in (1, ref.LEAF):
        got = emulator.run(v, f, want.points, leaf=leaf, tables=want.tables, lattice=(origin, voxel, dims))
        assert got.sdf.shape == (dims[2], dims[1], dims[0]) and all(cases.equal_result(got.row, want.surface)), name
        cases.compare_sdf(got.sdf, want)
        # the lattice is the query on the materialised points: the same walk, the same sign pass
        assert same(got.lattice_stats[:ref.STAT_WORDS], got.stats), (name, got.lattice_stats, got.stats)
        with np.errstate(all="ignore"):
            assert same(np.abs(got.sdf).reshape(-1), np.sqrt(got.dist2.astype(np.float64)).astype(F))
        if not want.signed.unstable.any():
            assert same(got.lattice_stats[ref.STAT_WORDS:], want.signed.stats), (name, got.lattice_stats, want.signed.stats)
    print(name, dict(zip(V.LATTICE_NAMES, got.lattice_stats.tolist())))


def test_the_lattice_points_are_exact_and_a_tsdf_volume_s():
    # a float64 product and sum rounded again differs from the fma on some of these; the fractions do not
    origin, voxel = F(-0.45), F(0.1)
    exact = np.array([ref.fma32(i, voxel, origin) for i in range(4096)], F)
    twice = (np.arange(4096, dtype=np.float64) * np.float64(voxel) + np.float64(origin)).astype(F)
    separate = (np.arange(4096, dtype=F) * voxel + origin).astype(F)
    print("lattice points: rounded twice differs on", int((exact != twice).sum()), "of 4096; two float32 roundings differ on", int((exact != separate).sum()))
    assert (exact != separate).any() and np.abs(exact.astype(np.float64) - (np.arange(4096) * np.float64(voxel) + np.float64(origin))).max() <= 2.0 ** -24 * 512
    assert ref.round32(ref.Fraction(1) + ref.Fraction(1, 2 ** 24)) == F(1.0) and ref.round32(ref.Fraction(1) + ref.Fraction(3, 2 ** 24)) == F(1.0 + 2.0 ** -22)      # ties to even
    core = open(os.path.join(abi_check.ROOT, "gaussianprediction_amd", "csrc", "volume_core.h")).read()
    tsdf = open(os.path.join(abi_check.ROOT, "gaussianprediction_amd", "csrc", "tsdf_core.h")).read()
    assert "return fmaf((float)i, voxel, origin);" in core and "return fmaf((float)i, voxel, origin);" in tsdf


def test_no_input_without_a_face(emulator):
    got = emulator.run(np.zeros((0, 3), F), np.zeros((0, 3), I), np.zeros((3, 3), F), tables=sdf_ref.tables(np.zeros((0, 3), F), np.zeros((0, 3), I), np.zeros((0, 2), I)),
                       lattice=((F(0),) * 3, F(0.5), (3, 2, 2)))
    assert np.isinf(got.sdf).all() and (got.sdf > 0).all() and (got.face == -1).all() and got.lattice_stats[ref.STAT_WORDS + sdf_ref.EXCLUDED] == 12


@pytest.mark.parametrize("n", list(cases.COMPARES))
def test_the_emulated_comparison(emulator, n):
    a, b = cases.COMPARES[n]
    got = emulator.run(np.zeros((0, 3), F), np.zeros((0, 3), I), np.zeros((0, 3), F), pair=(a, b))
    want = ref.compare(a, b)
    assert same(got.counts, want) and want[4] > 0 and want[5] == n, (got.counts, want)
    ok = np.isfinite(a) & np.isfinite(b)
    assert want[0] == sum(1 for x, y in zip(a, b) if np.isfinite(x) and np.isfinite(y) and x < 0) and want[3] == want[0] + want[1] - want[2] and want[4] == (~ok).sum()


def test_foreign_input_is_never_read_through(emulator):
    v, f, origin, voxel, dims = cases.LATTICES["cube_543"]
    want = cases.lattice("cube_543")
    bad = f.copy()
    bad[3, 1], bad[7, 0], bad[9, 2] = 99, -5, 2 ** 31 - 1                                      # indices outside the vertices: those faces are no candidates
    got = emulator.run(v, bad, want.points, tables=want.tables, lattice=(origin, voxel, dims))          # (exact arrays under the sanitizers)
    assert all(cases.equal_result(got.row, ref.surface_ref.point_mesh(want.points, v, bad))) and got.stats[ref.EXCLUDED_FACES] == 3
    nan = v.copy()
    nan[5, 1], nan[2, 0] = np.nan, np.inf
    got = emulator.run(nan, f, want.points)
    assert all(cases.equal_result(got.row, ref.surface_ref.point_mesh(want.points, nan, f)))
    tables = sdf_ref.tables(v, f, want.topology.edge)
    tables.face_edges = np.full_like(tables.face_edges, 10 ** 6)                               # a table that is not this mesh's: counted, never an index
    got = emulator.run(v, f, want.points, tables=tables, lattice=(origin, voxel, dims))
    edge_rows = want.signed.kind == 1
    assert got.lattice_stats[ref.STAT_WORDS + sdf_ref.STATUS] == int(edge_rows.any()) and same(np.abs(got.sdf), np.abs(want.sdf))
    huge = np.array([[3e38, 3e38, 3e38], [-3e38, 1e30, 0]], F)                                 # squared distances beyond float32: dist2 is +inf with a face
    got = emulator.run(v, f, huge)
    with np.errstate(over="ignore"):
        assert all(cases.equal_result(got.row, ref.surface_ref.point_mesh(huge, v, f)))
    for sizes, word in (((-1, 1, 0, 1, 4, 0, 0, 0, 0), ">= 0"), ((8, 2 ** 26, 0, 1, 4, 0, 0, 0, 0), "nf must be below 2^26"), ((8, 12, 37, 1, 4, 0, 0, 0, 0), "n_edges must be 0 .. 3*nf"),
                        ((8, 12, 0, -1, 4, 0, 0, 0, 0), "2^31 - 1"), ((8, 12, 0, 1, 4, 0, 1, 1, 0), "nx, ny and nz must be >= 1"), ((8, 12, 0, 1, 4, 2048, 2048, 512, 0), "below 2^31"),
                        ((8, 12, 0, 1, 0, 0, 0, 0, 0), "leaf must be")):
        assert word in emulator.run(v, f, want.points[:1], code=3, sizes=sizes, lattice=((0, 0, 0), 0.1, (0, 0, 0)))


def test_the_tree_tests_less_than_the_grid_where_the_queries_lie_deep(emulator, tmp_path):
    """The requirement on the feature: summed over the finite queries of the deep cases, the boxes and records the tree tests are
    strictly fewer than the records the grid tests (tests/surface_emulate.cpp's CANDIDATES) on the same queries."""
    grid = surface_cases.build_emulator(tmp_path, sanitize=False)
    for name in cases.DEEP:
        v, f, q = cases.CASES[name]
        q = q[np.isfinite(q).all(axis=1)]
        tree = emulator.run(v, f, q)
        stats = grid.query(v, f, q)[5]
        work = int(tree.stats[ref.NODES] + tree.stats[ref.CANDIDATES])
        print(name, "queries", len(q), "tree nodes", int(tree.stats[ref.NODES]), "tree candidates", int(tree.stats[ref.CANDIDATES]), "grid candidates",
              int(stats[S.STAT_NAMES.index("candidates")]), "swept", int(stats[S.STAT_NAMES.index("swept")]), "ratio", stats[S.STAT_NAMES.index("candidates")] / work)
        assert same(tree.dist2, grid.query(v, f, q)[0]) and work < stats[S.STAT_NAMES.index("candidates")]


# ---- the refusals that need no device ----
def test_refusals_before_any_pointer_is_looked_at():
    l = V.lib()

    def refused(rc, word):
        assert rc == 1 and word in l.gp_last_error(), (word, l.gp_last_error())

    for nf, word in ((-1, b">= 0"), (2 ** 26, b"nf must be below 2^26")):
        assert l.gp_volume_tree_scratch_bytes(nf) == -1 and word in l.gp_last_error()
    assert l.gp_volume_tree_scratch_bytes(0) > 0 and l.gp_volume_tree_scratch_bytes(2 * 10 ** 6) >= (96 + 32 + 16) * 2 * 10 ** 6

    def tree(vertices=16, faces=16, nv=4, nf=2, scratch=16):
        return l.gp_volume_tree(vertices, faces, nv, nf, scratch, None)

    for kw, word in ((dict(nv=-1), b">= 0"), (dict(nv=2 ** 31), b"nv must be below 2^31"), (dict(nf=2 ** 26), b"nf must be below 2^26"), (dict(scratch=None), b"null"),
                     (dict(scratch=8), b"16-byte aligned"), (dict(vertices=None), b"null"), (dict(faces=None), b"null")):
        refused(tree(**kw), word)

    def query(queries=16, nq=5, scratch=16, nf=2, dist2=16, face=16, region=16, closest=16, bary=16, stats=16):
        return l.gp_volume_query(queries, nq, scratch, nf, dist2, face, region, closest, bary, stats, None)

    for kw, word in ((dict(nq=-1), b"2^31 - 1"), (dict(nq=2 ** 31), b"2^31 - 1"), (dict(nf=2 ** 26), b"2^26"), (dict(nf=-1), b">= 0"), (dict(scratch=None), b"null"),
                     (dict(scratch=24), b"16-byte aligned"), (dict(queries=None), b"null"), (dict(dist2=None), b"null"), (dict(face=None), b"null"), (dict(region=None), b"null"),
                     (dict(closest=None), b"null"), (dict(bary=None), b"null"), (dict(stats=None), b"null")):
        refused(query(**kw), word)

    def lattice(scratch=16, vertices=16, faces=16, nv=4, nf=2, face_edges=16, edge_normal=16, ne=5, vertex_normal=16, ox=0.0, oy=0.0, oz=0.0, voxel=0.1, nx=4, ny=4, nz=4, sdf=16,
                stats=16):
        return l.gp_volume_lattice(scratch, vertices, faces, nv, nf, face_edges, edge_normal, ne, vertex_normal, ox, oy, oz, voxel, nx, ny, nz, sdf, stats, None)

    inf, nan = float("inf"), float("nan")
    for kw, word in ((dict(nv=2 ** 31), b"nv must be below"), (dict(nf=2 ** 26), b"2^26"), (dict(ne=7), b"n_edges must be"), (dict(ox=nan), b"must be finite"), (dict(oy=inf), b"must be finite"),
                     (dict(oz=-inf), b"must be finite"), (dict(voxel=nan), b"must be finite"), (dict(voxel=inf), b"must be finite"), (dict(voxel=0.0), b"voxel must be > 0"),
                     (dict(voxel=-1.0), b"voxel must be > 0"), (dict(nx=0), b"must be >= 1"), (dict(ny=-3), b"must be >= 1"), (dict(nz=0), b"must be >= 1"),
                     (dict(nx=2048, ny=2048, nz=512), b"below 2^31"), (dict(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1), b"below 2^31"), (dict(scratch=None), b"null"),
                     (dict(scratch=4), b"16-byte aligned"), (dict(vertices=None), b"null"), (dict(faces=None), b"null"), (dict(face_edges=None), b"null"), (dict(edge_normal=None), b"null"),
                     (dict(vertex_normal=None), b"null"), (dict(sdf=None), b"null"), (dict(stats=None), b"null")):
        refused(lattice(**kw), word)

    def compare(a=16, b=16, n=5, counts=16):
        return l.gp_volume_compare(a, b, n, counts, None)

    for kw, word in ((dict(n=-1), b"2^31 - 1"), (dict(n=2 ** 31), b"2^31 - 1"), (dict(a=None), b"null"), (dict(b=None), b"null"), (dict(counts=None), b"null")):
        refused(compare(**kw), word)


def test_the_python_surface_refuses_before_the_device(monkeypatch):
    for module in (V, D, S, G, MS, T):
        monkeypatch.setattr(module, "lib", lambda: pytest.fail("a launch was reached"))
    faces, vertices, cloud = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, 3), torch.zeros(5, 3)
    mesh = (vertices, faces)
    for call in (lambda: V.MeshTree(mesh), lambda: V.SignedTree(mesh), lambda: V.lattice_for(mesh), lambda: V.lattice_for([mesh, mesh], voxel_size=0.1),
                 lambda: V.sdf_volume(mesh), lambda: V.sdf_volume(mesh, voxel_size=0.1, origin=(0, 0, 0), dims=(2, 2, 2)), lambda: V.volume_iou(mesh, mesh), lambda: V.remesh(mesh),
                 lambda: V.compare(torch.zeros(3), torch.zeros(3))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for call, word in ((lambda: V.MeshTree((vertices, faces.long())), "int32"), (lambda: V.MeshTree((vertices[0], faces)), r"\[Nv, 3\]"),
                       (lambda: V.compare(torch.zeros(3, dtype=torch.float64), torch.zeros(3)), "float32")):
        with pytest.raises(RuntimeError, match=word):
            call()
    for call, word in ((lambda: V.sdf_volume(mesh, origin=(0, 0, 0)), "origin and dims go together"), (lambda: V.sdf_volume(mesh, origin=(0, 0, 0), dims=(2, 2, 2)), "need a voxel_size"),
                       (lambda: V.lattice_rule((0, 0, 0), (1, 1, 1), resolution=6), "resolution must be above"), (lambda: V.lattice_rule((0, 0, 0), (1, 1, 1), margin=-1), "margin must be >= 0"),
                       (lambda: V.lattice_rule((0, 0, 0), (0, 0, 0)), "no extent"), (lambda: V.lattice_rule((0, 0, 0), (1, 1, 1), voxel_size=0.0), "voxel_size must be finite and > 0"),
                       (lambda: V.lattice_rule((0, 0, 0), (1, 1, 1), voxel_size=float("nan")), "voxel_size must be"), (lambda: V.lattice_rule((float("inf"),) * 3, (float("-inf"),) * 3), "no vertex with finite"),
                       (lambda: V.lattice_rule((0, 0, 0), (1, 1, 1), voxel_size=1e-4), "below 2\\^31")):
        with pytest.raises(_lib.GpHipError, match=word):
            call()
    for args, word in ((((0, 0, float("nan")), 0.1, (2, 2, 2)), "origin and voxel must be finite"), (((0, 0, 0), 0.0, (2, 2, 2)), "voxel must be > 0"), (((0, 0, 0), 0.1, (2, 0, 2)), "must be >= 1"),
                       (((0, 0, 0), 0.1, (2048, 2048, 512)), "nx\\*ny\\*nz must be below 2\\^31")):
        assert re.search(word, V.check_lattice(*args))
    assert V.check_lattice((0, 0, 0), 0.1, (2047, 2048, 512)) is None


def test_lattice_for_s_rule():
    # pinned numbers: the unit cube at voxel 0.07f, the IoU pair at 0.1f, and the automatic voxel
    f32 = lambda x: float(F(x))
    assert V.lattice_rule((0, 0, 0), (1, 1, 1), voxel_size=0.07) == ((f32(-0.175),) * 3, f32(0.07), (21, 21, 21)) == ref.lattice_for(cases.CUBE_V, F(0.07))
    assert V.lattice_rule((0, 0, 0), (1.5, 1, 1), voxel_size=0.1) == ((-0.25,) * 3, f32(0.1), (21, 16, 16)) == ref.lattice_for(np.concatenate([cases.IOU.a[0], cases.IOU.b[0]]), F(0.1))
    up = lambda x: int(np.ceil(x))
    origin, voxel, dims = V.lattice_rule((-1, 0, 2), (3, 1, 2.5))
    assert voxel == f32(4 / 122) and origin == (f32(-1 - 2.5 * voxel), f32(-2.5 * voxel), f32(2 - 2.5 * voxel)) and dims == (up(4 / voxel) + 6, up(1 / voxel) + 6, up(0.5 / voxel) + 6)
    assert dims[0] in (128, 129) and dims[1:] == (37, 22)
    small = f32(4 / 62)
    assert V.lattice_rule((-1, 0, 2), (3, 1, 2.5), resolution=64, margin=0) == ((f32(-1 - 0.5 * small), f32(-0.5 * small), f32(2 - 0.5 * small)), small, (up(4 / small) + 2, 18, 10))
    rng = np.random.default_rng(7)
    for _ in range(50):
        lo = rng.uniform(-5, 5, 3)
        hi = lo + rng.uniform(0.01, 4, 3)
        resolution, margin = int(rng.integers(8, 300)), int(rng.integers(0, 3))
        origin, voxel, dims = V.lattice_rule(lo, hi, None, resolution, margin)
        last = [o + (d - 1) * voxel for o, d in zip(origin, dims)]
        assert all(o <= l - margin * voxel for o, l in zip(origin, lo)) and all(e >= h + margin * voxel for e, h in zip(last, hi))      # the lattice reaches the margin on every side
        assert resolution <= max(dims) <= resolution + 1
    for name in ("33_sphere", "33_torus"):
        v = cases.geometry_cases.MESHES[name][0]
        lo, hi = v.min(axis=0), v.max(axis=0)
        assert V.lattice_rule(lo, hi) == ref.lattice_for(v) and V.lattice_rule(lo, hi, 0.05, 64, 3) == ref.lattice_for(v, 0.05, 64, 3)
    doc = V.lattice_for.__doc__
    assert "(margin + 0.5) * voxel_size" in doc and "2 * margin + 2" in doc and "ONE read of 24 bytes" in doc


def test_signatures_and_docstrings():
    assert list(inspect.signature(V.MeshTree.__init__).parameters) == ["self", "mesh"] and list(inspect.signature(V.SignedTree.__init__).parameters) == ["self", "mesh", "topology"]
    assert list(inspect.signature(V.SignedTree.lattice).parameters) == ["self", "origin", "voxel_size", "dims"]
    sig = inspect.signature(V.lattice_for)
    assert list(sig.parameters) == ["meshes", "voxel_size", "resolution", "margin"] and [p.default for p in sig.parameters.values()][1:] == [None, 128, 2]
    sig = inspect.signature(V.sdf_volume)
    assert list(sig.parameters) == ["mesh", "voxel_size", "resolution", "margin", "origin", "dims"] and [p.default for p in sig.parameters.values()][1:] == [None, 128, 2, None, None]
    assert list(inspect.signature(V.volume_iou).parameters) == ["mesh_a", "mesh_b", "voxel_size", "resolution"] and list(inspect.signature(V.remesh).parameters) == ["mesh", "voxel_size", "resolution", "trunc"]
    assert V.SdfVolume.__slots__ == ("sdf", "origin", "voxel_size", "dims") and hasattr(V.SdfVolume, "inside") and hasattr(V.SdfVolume, "to_tsdf") and hasattr(V.SignedTree, "contains")
    assert "byte-equal to" in V.MeshTree.query.__doc__ and "Nothing is read" in V.MeshTree.query.__doc__ and "reads nothing" in V.MeshTree.__doc__
    assert "byte-equal to" in V.SignedTree.query.__doc__ and "ONE for the counts" in V.volume_iou.__doc__ and "to_tsdf(trunc).extract()" in V.remesh.__doc__
    assert "D._sign(" in inspect.getsource(V.SignedTree.query)                                  # the sign pass is sdf_ops' own
    # the modules the feature was told to leave alone do not know of it
    for module in (G, D, S, T):
        assert "volume_ops" not in inspect.getsource(module)
