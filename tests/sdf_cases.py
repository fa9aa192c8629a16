"""Seeded cases of the signed distance, shared by the host test (the stand-alone build of csrc/sdf_core.h) and the GPU test (sdf_ops).
Small on purpose; each names what it can break.  A case is (vertices, faces, queries).

  flat_tet, flat_tet_backwards    a nearly flat tetrahedron, its faces in both numberings: the winning face's own normal gives the wrong
                                  sign for queries nearest to its sharp edges and corners; the pseudonormal does not
  cube, cube_flipped              12 faces; the flipped one has every sign inverted and a negative volume
  triangle, shared_edge           surface_cases' open meshes: the sign is the side of the sheet
  three_on_edge                   a non-manifold edge: three faces on one edge
  duplicate_face                  a face twice: counted twice in the sums
  against                         two faces on the same corners wound against each other: every edge and vertex normal cancels to
                                  zero, the queries nearest to an edge or a corner are undetermined and counted
  degenerate                      a face (a, a, b), a collinear face and a proper one
  hub                             surface_cases' 2000 corners at one vertex: one lane's walk
  33_sphere, 33_torus             rows 150:450 of surface_cases' queries (rows 0:150 are samples ON the surface: not sign rows at all)
  nq_1, nq_63, nq_65, nq_257      wave and workgroup boundaries, on the cube
  nan_query                       queries with NaN and inf: excluded

At import, on the CPU, the module asserts what the tests rest on (see the end of the file)."""
import functools
from types import SimpleNamespace

import numpy as np

import geometry_cases
import mesh_smooth_ref
import sdf_ref as ref
import surface_cases
import surface_ref

F = np.float32
I = np.int32
same = surface_cases.same

# The float64 tables pass through sqrt and atan2, whose device and host libraries may differ in the last bits: a component of
# edge_normal or vertex_normal is held to TABLE_K * 2^-53 * (the sum of |term| of that component).  MEASURED_K is the largest such
# ratio of the device's tables against tests/sdf_ref.py over all cases below; TABLE_K is four times it, because
# other inputs reach other arguments.
MEASURED_K = 4.94               # on an MI355X: 4.934 on vertex_normal of 33_torus (4.873 on 33_sphere, 3.72 on hub); 0 on every edge_normal (no atan2 there)
TABLE_K = 4 * MEASURED_K
UNSTABLE_CAP = 0.01             # a case may leave out at most 1 % of its rows as unstable (|g| <= 2^-30 |r| |N|) ...
NO_UNSTABLE = ("flat_tet", "flat_tet_backwards", "cube", "cube_flipped")          # ... and these none at all
NEAR = 1e-4                     # against the winding number: rows within NEAR of the mesh extent of the surface are left out, under the same cap
CLOSED = ("flat_tet", "flat_tet_backwards", "cube", "cube_flipped", "33_sphere", "33_torus")


def _box(rng, vertices, n, margin=0.5):
    lo, hi = vertices.min(axis=0).astype(np.float64), vertices.max(axis=0).astype(np.float64)
    ext = float((hi - lo).max())
    return rng.uniform(lo - margin * ext, hi + margin * ext, (n, 3)).astype(F)


CUBE_V = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], F)
CUBE_F = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]], I)
CUBE_CORNERS = (CUBE_V.astype(np.float64) * 1.5 - 0.25).astype(F)          # eight queries beyond the corners: outside, nearest to a vertex
CUBE_CENTRES = np.array([[0.5, 0.5, 0.5], [0.25, 0.5, 0.5], [0.5, 0.75, 0.25], [0.9, 0.9, 0.9], [0.1, 0.1, 0.1], [0.5, 0.5, 0.95]], F)      # inside


def _cases():
    C = {}
    rng = np.random.default_rng(33)
    tet = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.3, 0.3, 0.05]], F)
    tet_f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], I)
    q = np.concatenate([_box(rng, tet, 250, 0.3), rng.uniform([-0.2, -0.2, -0.05], [1.2, 1.2, 0.1], (150, 3)).astype(F)])          # a box around it, and a slab that holds it
    C["flat_tet"] = (tet, tet_f, q)
    C["flat_tet_backwards"] = (tet, tet_f[::-1].copy(), q)
    q = np.concatenate([CUBE_CORNERS, CUBE_CENTRES, _box(rng, CUBE_V, 386)])
    C["cube"] = (CUBE_V, CUBE_F, q)
    C["cube_flipped"] = (CUBE_V, CUBE_F[:, ::-1].copy(), q)
    for name in ("triangle", "shared_edge"):          # (without row 6 of either: a query in the sheet's own plane beyond its rim, where g is 0 up to rounding -- no sign row)
        v, f, q = surface_cases.CASES[name]
        C[name] = (v, f, np.delete(q, 6, axis=0))
    fin = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0.5], [-0.5, 1, 0.5], [-0.5, -1, 0.5]], F)
    C["three_on_edge"] = (fin, np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]], I), np.concatenate([np.array([[0, 0, 0.5], [-1, 0, 0.5], [0.1, 0.05, 2]], F), _box(rng, fin, 60)]))
    tri = surface_cases.CASES["triangle"][0]
    wing = np.concatenate([tri, np.array([[2, 2, 1]], F)])
    C["duplicate_face"] = (wing, np.array([[0, 1, 2], [1, 3, 2], [0, 1, 2]], I), _box(rng, wing, 60))
    C["against"] = (tri, np.array([[0, 1, 2], [1, 0, 2]], I), np.concatenate([np.array([[1, -1, 0.5], [-1, -1, 1], [3, 3, 0], [0.5, 0.5, 1], [0.5, 0.5, -1]], F), _box(rng, tri, 40)]))
    line = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0], [0, 2, 0], [0, 0, 1]], F)
    C["degenerate"] = (line, np.array([[0, 0, 3], [0, 1, 2], [0, 3, 4]], I), np.concatenate([np.array([[2, 1, 0], [0, 1, 0.5], [-1, 1, 0.5], [1, 1, 0]], F), _box(rng, line, 40)]))
    v, f, q = surface_cases.CASES["hub"]
    C["hub"] = (v, f, q)
    for name in ("33_sphere", "33_torus"):
        v, f, q = surface_cases.CASES[name]
        C[name] = (v, f, q[150:450])
    for nq in (1, 63, 65, 257):
        C[f"nq_{nq}"] = (CUBE_V, CUBE_F, _box(rng, CUBE_V, nq))
    bad = _box(rng, CUBE_V, 12)
    bad[::3, 0], bad[1::6, 2], bad[4::6, 1] = np.nan, np.inf, -np.inf
    C["nan_query"] = (CUBE_V, CUBE_F, bad)
    return {k: tuple(np.ascontiguousarray(a) for a in c) for k, c in C.items()}


CASES = _cases()


@functools.lru_cache(maxsize=None)
def result(name):
    """The restatement's whole answer for a case; do not modify.  surface: surface_ref.point_mesh; topology: mesh_smooth_ref.edges;
    tables: sdf_ref.tables; signed: sdf_ref.sign on the restated (dist2, face, region)."""
    v, f, q = CASES[name]
    surface = surface_ref.point_mesh(q, v, f)
    topology = mesh_smooth_ref.edges(f, len(v))
    tables = ref.tables(v, f, topology.edge)
    signed = ref.sign(q, surface.dist2, surface.face, surface.region, v, f, tables)
    return SimpleNamespace(surface=surface, topology=topology, tables=tables, signed=signed, means=ref.means(signed.sdf, signed.sign))


def table_ratio(got, want, size):
    """The largest |got - want| / (2^-53 * size) over the components (size: the sum of |term|); inf where a component with size 0 differs."""
    got, want, size = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(size, np.float64)
    if not got.size:
        return 0.0
    with np.errstate(all="ignore"):
        diff = np.abs(got - want)
        ratio = np.where(diff == 0.0, 0.0, diff / (2.0 ** -53 * size))
    return float(np.nan_to_num(ratio, nan=np.inf).max())


def compare(name, got):
    """got: SimpleNamespace(face_edges, edge_normal, vertex_normal, volume, counts, sdf, sign, kind, element, stats[, means]) of the
    device or of the emulator.  Asserts the issue's comparison against the restatement; returns the two measured table ratios."""
    want = result(name)
    t, s = want.tables, want.signed
    assert same(got.face_edges, t.face_edges) and same(got.counts, t.counts), name
    ratios = (table_ratio(got.edge_normal, t.edge_normal, t.edge_size), table_ratio(got.vertex_normal, t.vertex_normal, t.vertex_size))
    print(name, "table ratios (edge, vertex):", ratios, "unstable rows:", int(s.unstable.sum()), "of", len(s.sign))
    assert max(ratios) <= TABLE_K, (name, ratios)
    assert same(np.float64(got.volume), t.volume), (name, got.volume, t.volume)          # (products, sums and one division: no library function)
    assert same(got.kind, s.kind) and same(got.element, s.element), name
    stable = ~s.unstable
    assert same(got.sign[stable], s.sign[stable]) and same(got.sdf[stable], s.sdf[stable]), (name, np.nonzero(got.sign != s.sign)[0][:8])
    assert same(np.abs(got.sdf), np.abs(s.sdf)), name
    if not s.unstable.any():
        assert same(got.stats, s.stats), (name, got.stats, s.stats)
        if hasattr(got, "means"):
            assert same(got.means, want.means), (name, got.means, want.means)
    else:
        assert same(got.stats[[ref.FACE, ref.EDGE, ref.VERTEX, ref.EXCLUDED, ref.STATUS]], s.stats[[ref.FACE, ref.EDGE, ref.VERTEX, ref.EXCLUDED, ref.STATUS]]), name
    return ratios


def winding_rows(name):
    """(kept, inside): the rows of a closed case that are compared with the winding number -- finite queries farther than NEAR of the
    mesh extent from the surface -- and what the winding number says of every row (inside <=> |w| > 0.5)."""
    v, f, q = CASES[name]
    want = result(name)
    ok = np.isfinite(q).all(axis=1)
    extent = float((v.max(axis=0).astype(np.float64) - v.min(axis=0)).max())
    with np.errstate(all="ignore"):
        kept = ok & (np.sqrt(want.surface.dist2_f64) > NEAR * extent)
    w = ref.winding_number(np.where(ok[:, None], q, 0), v, f)
    return kept, np.abs(w) > 0.5


# ---- the stand-alone build of csrc/sdf_core.h, as a child process ----
def build_emulator(d, sanitize):
    """tests/sdf_emulate.cpp built into `d` (a pathlib directory), under the sanitizers where `sanitize` is set; returns
    run(vertices, faces, edge, queries, dist2, face, region) -> the SimpleNamespace compare() takes, one run of the child."""
    import struct
    import subprocess

    import emulate_build
    exe = emulate_build.build("sdf_emulate", d, sanitize=sanitize)

    def run(vertices, faces, edge, queries, dist2, face, region, code=0, sizes=None):
        nv, nf, ne, nq = sizes or (len(vertices), len(faces), len(edge), len(queries))
        job, out = str(d / "job.bin"), str(d / "out.bin")
        with open(job, "wb") as fp:
            fp.write(struct.pack("<8i", nv, nf, ne, nq, 0, 0, 0, 0))
            for a, dtype in ((vertices, F), (faces, I), (edge, I), (queries, F), (dist2, F), (face, I), (region, I)):
                fp.write(np.ascontiguousarray(a, dtype).tobytes())
        done = subprocess.run([exe, job, out], timeout=300, stderr=subprocess.PIPE)
        assert done.returncode == code, done.stderr.decode()
        if code:
            return done.stderr.decode()
        raw, got, at = open(out, "rb").read(), SimpleNamespace(), 0
        for key, dtype, shape in (("face_edges", I, (nf, 3)), ("edge_normal", np.float64, (ne, 3)), ("vertex_normal", np.float64, (nv, 3)), ("volume", np.float64, ()),
                                  ("counts", I, (ref.COUNT_WORDS,)), ("sdf", F, (nq,)), ("sign", np.int8, (nq,)), ("kind", I, (nq,)), ("element", I, (nq,)),
                                  ("stats", np.int64, (ref.STAT_WORDS,)), ("means", np.float64, (ref.MEAN_WORDS,))):
            n = int(np.prod(shape))
            setattr(got, key, np.frombuffer(raw, dtype, n, at).reshape(shape))
            at += n * np.dtype(dtype).itemsize
        assert at == len(raw)
        return got

    return SimpleNamespace(run=run)


# ---- what the tests rest on, asserted on the CPU at import ----
def _conditions():
    for name in CLOSED:
        v, f, _ = CASES[name]
        t = result(name)
        assert t.topology.stats["watertight"], name                                   # the closed cases are watertight by mesh_smooth_ref.edges
        assert (t.tables.volume > 0) == (name != "cube_flipped"), (name, t.tables.volume)
    for name in CASES:
        s = result(name).signed
        left = int(s.unstable.sum())
        assert left <= UNSTABLE_CAP * len(s.sign) and (left == 0 or name not in NO_UNSTABLE), (name, left)      # the restatement alone stays within the cap
    for name in CLOSED:
        kept, inside = winding_rows(name)
        s = result(name).signed
        assert (~kept & np.isfinite(CASES[name][2]).all(axis=1)).sum() <= UNSTABLE_CAP * len(kept), name
        negative = inside != (name == "cube_flipped")                                                           # (wound inward: every sign inverted)
        assert ((s.sign[kept] < 0) == negative[kept]).all() and (s.sign[kept] != 0).all(), name                 # the restatement agrees with the winding number
    for name in ("flat_tet", "flat_tet_backwards"):                                  # ... where the winning face's own normal does not
        v, f, q = CASES[name]
        kept, inside = winding_rows(name)
        want = result(name)
        naive = ref.face_normal_sign(q, want.surface.closest, want.surface.face, v, f)
        assert ((naive[kept] < 0) != inside[kept]).sum() >= 1, name


_conditions()
