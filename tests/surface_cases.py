"""Seeded cases of the point-to-surface distance, shared by the host test (the stand-alone build of csrc/surface_core.h) and the GPU
test (surface_ops).  Small on purpose; each names what it can break.  A case is (vertices, faces, queries).

  triangle        one triangle; queries in each of its seven Voronoi regions, on its plane inside, on an edge, and exactly at each corner
  point_face      a face (a, a, a): every candidate is the point
  segment_face    three collinear corners: no interior candidate, no zero denominator
  mixed           geometry_cases' mesh with NaN, inf, bad-index and zero-area faces and one area twice (faces 0 and 5: a tie everywhere)
  no_faces        every query gets (+inf, -1)
  identical       two identical coplanar faces and a third with the corners rotated: the smallest number wins
  shared_edge     two faces with a common edge, queries on it and in the wedge above it, where both faces give the edge's distance
  mid_plane       two parallel faces, queries in the plane half way between them
  uneven          10^12 to 1 in area: the large face's box holds every cell and goes to the wide list
  slivers, fan    the thin and the hub meshes of mesh_render_cases
  hub             2000 thin triangles around one vertex: the hub's cell holds every face
  far_origin      a small mesh near 10^6: an ulp of a coordinate is larger than a cell of the finer rules
  sizes_*         nf of 1, 63, 65, 257 with nq of 1, 255, 257, 256: wave and workgroup boundaries
  33_sphere, 33_torus     surface samples of the same mesh and of the other, a seeded cube around both, queries 10^3 extents away
                  (the sweep), queries with NaN and inf

Every case runs under every rule of RULES and under both WIDE (the shipped W, and 1: every face with a box of two cells or more is
wide), so that both the wide path and the cell path see every face."""
import functools
from types import SimpleNamespace

import numpy as np

import geometry_cases
import geometry_ref
import surface_ref as ref

F = np.float32
I = np.int32
RULES = geometry_cases.RULES                    # cells along the longest axis: "1", "2", "7", "auto", "1024" (halved to the 2^24 cells)
WIDE = (ref.WIDE_CELLS, 1)
ATTRIBUTES = 4


def _cube(rng, vertices, n, margin=0.3):
    v = vertices[np.isfinite(vertices).all(axis=1)].astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = max(float((hi - lo).max()), 1e-3)
    return rng.uniform(lo - margin * ext, hi + margin * ext, (n, 3)).astype(F)


def _cases():
    C = {}
    rng = np.random.default_rng(31)
    tri = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0]], F)
    q = [(0.5, 0.5, 1), (1, -1, 0.5), (2, 2, 0.25), (-1, 1, -0.25), (-1, -1, 0.5), (3, -0.5, 0.125), (-0.5, 3, 0),      # the seven regions
         (0.5, 0.5, 0), (1, 0, 0), (1, 1, 0), (0, 0.5, 0), (0, 0, 0), (2, 0, 0), (0, 2, 0)]                             # on the triangle itself
    C["triangle"] = (tri, np.array([[0, 1, 2]], I), np.concatenate([np.array(q, F), _cube(rng, tri, 40)]))
    C["point_face"] = (np.array([[1, 2, 3]], F), np.array([[0, 0, 0]], I), np.concatenate([np.array([[1, 2, 4], [1, 2, 3]], F), rng.uniform(-4, 4, (20, 3)).astype(F)]))
    C["segment_face"] = (np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0]], F), np.array([[0, 1, 2]], I),
                         np.concatenate([np.array([[2, 1, 0], [0.5, 0, 1], [4, 0, 0], [-1, 0, 0]], F), rng.uniform(-2, 5, (20, 3)).astype(F)]))
    v, f = geometry_cases.MESHES["mixed"]
    C["mixed"] = (v, f, np.concatenate([np.array([[0.25, 0.25, 1], [3, 3, 3.5], [0.25, 0.25, 0]], F), rng.uniform(-1, 4, (40, 3)).astype(F)]))
    v, f = geometry_cases.MESHES["no_faces"]
    C["no_faces"] = (v, f, rng.uniform(-1, 1, (10, 3)).astype(F))
    C["identical"] = (tri, np.array([[0, 1, 2], [0, 1, 2], [1, 2, 0]], I), np.concatenate([np.array(q, F), _cube(rng, tri, 30)]))
    roof = np.array([[0, 0, 0], [2, 0, 0], [1, 1, 1], [1, -1, 1]], F)
    C["shared_edge"] = (roof, np.array([[0, 1, 2], [1, 0, 3]], I),
                        np.concatenate([np.array([[1, 0, 0], [0.5, 0, 0], [1, 0, -1], [0.25, 0, -2], [1, 0, 0.5], [0, 0, 0], [-1, 0, 0]], F), _cube(rng, roof, 40)]))
    two = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 2], [2, 0, 2], [0, 2, 2]], F)
    C["mid_plane"] = (two, np.array([[3, 4, 5], [0, 1, 2]], I),
                      np.concatenate([np.array([[0.5, 0.5, 1], [0.25, 1, 1], [3, 3, 1], [-1, 0.5, 1]], F), _cube(rng, two, 40)]))
    v, f = geometry_cases.MESHES["uneven"]
    C["uneven"] = (v, f, np.concatenate([np.array([[1e-4, 0, 1e-4], [500, 500, 1], [0, 0, 5e-4]], F), _cube(rng, v, 60), rng.uniform(-2e-3, 2e-3, (30, 3)).astype(F)]))
    for name in ("slivers", "fan"):
        v, f = geometry_cases.MESHES[name]
        C[name] = (v, f, _cube(rng, v, 80))
    k = 2000
    angle = np.linspace(0, 2 * np.pi, k, endpoint=False)
    rim = np.stack([np.cos(angle), np.sin(angle), 0.2 * np.sin(7 * angle)], axis=1)
    v = np.concatenate([np.zeros((1, 3)), rim]).astype(F)
    C["hub"] = (v, np.stack([np.zeros(k), 1 + np.arange(k), 1 + (np.arange(k) + 1) % k], axis=1).astype(I),
                np.concatenate([np.array([[0, 0, 0.5], [0, 0, 0], [1e-3, 2e-3, 1e-2]], F), _cube(rng, v, 100)]))
    v, f = geometry_cases.MESHES["random"]
    far = (v - v[np.isfinite(v).all(axis=1)].mean(axis=0).astype(F)) * F(0.01) + F(1e6)
    C["far_origin"] = (far.astype(F), f, _cube(rng, far.astype(F), 80))
    for nf, nq in ((1, 1), (63, 255), (65, 257), (257, 256)):
        v = rng.uniform(-1, 1, (nf + 2, 3)).astype(F)
        C[f"sizes_{nf}"] = (v, np.stack([np.arange(nf), np.arange(nf) + 1, np.arange(nf) + 2], axis=1).astype(I), rng.uniform(-1.2, 1.2, (nq, 3)).astype(F))
    both = np.concatenate([geometry_cases.MESHES["33_sphere"][0], geometry_cases.MESHES["33_torus"][0]])
    cube = _cube(rng, both, 150, 0.1)
    for name, other in (("33_sphere", "33_torus"), ("33_torus", "33_sphere")):
        v, f = geometry_cases.MESHES[name]
        own = geometry_ref.sample_surface(v, f, 150, 5).points
        others = geometry_ref.sample_surface(*geometry_cases.MESHES[other], 150, 6).points
        ext = float((v.max(axis=0) - v.min(axis=0)).max())
        away = (rng.normal(size=(8, 3)) * 1e3 * ext).astype(F)
        bad = rng.uniform(-1, 1, (8, 3)).astype(F)
        bad[::2, 0], bad[1::4, 2], bad[3::4, 1] = np.nan, np.inf, -np.inf
        C[name] = (v, f, np.concatenate([own, others, cube, away, bad]).astype(F))
    return {k: tuple(np.ascontiguousarray(a) for a in c) for k, c in C.items()}


CASES = _cases()
SAMPLE_ROWS = {"33_sphere": slice(0, 150), "33_torus": slice(0, 150)}          # the rows that are samples of the case's own mesh
CUBE_ROWS = slice(300, 450)


def cell_of(name, rule):
    """The cell size that gives `rule` cells along the longest axis of the corners of the usable faces (0.0: the automatic rule)."""
    if rule == "auto":
        return 0.0
    v, f, _ = CASES[name]
    usable = ref.usable_faces(v, f)
    p = v[f[usable]].reshape(-1, 3)
    extent = float((p.max(axis=0).astype(np.float64) - p.min(axis=0)).max()) if len(p) else 0.0
    if not extent > 0:
        return 1.0
    cell = F(extent / int(rule))
    return float(cell if float(cell) * int(rule) >= extent else np.nextafter(cell, F(np.inf)))          # rounded up: never rule + 1 cells


RUNS = [(name, rule, wide) for name in CASES for rule in RULES for wide in WIDE]


@functools.lru_cache(maxsize=None)
def result(name):
    """surface_ref.point_mesh of a case (no rule enters it); do not modify."""
    v, f, q = CASES[name]
    return ref.point_mesh(q, v, f)


def attributes_of(name):
    return np.random.default_rng(51).uniform(-1, 1, (len(CASES[name][0]), ATTRIBUTES)).astype(F)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def equal_result(got, want):
    """got: (dist2, face, region, closest, bary) arrays; want: a result of surface_ref.point_mesh.  Bit for bit, all five."""
    return [same(g, w) for g, w in zip(got, (want.dist2, want.face, want.region, want.closest, want.bary))]


# ---- the stand-alone build of csrc/surface_core.h, as a child process ----
def build_emulator(d, sanitize):
    """tests/surface_emulate.cpp built into `d` (a pathlib directory), under the sanitizers where `sanitize` is set; returns
    query(vertices, faces, queries, cell, wide_cells, ...) -> (dist2, face, region, closest, bary, stats, dims), one run of the child."""
    import struct
    import subprocess

    import emulate_build
    exe = emulate_build.build("surface_emulate", d, sanitize=sanitize)

    def query(vertices, faces, queries, cell=0.0, wide_cells=ref.WIDE_CELLS, backwards=False, short_by=0, code=0, sizes=None):
        nv, nf, nq = sizes or (len(vertices), len(faces), len(queries))
        job, out = str(d / "job.bin"), str(d / "out.bin")
        with open(job, "wb") as fp:
            fp.write(struct.pack("<8i", nv, nf, nq, wide_cells, int(backwards), short_by, 0, 0) + struct.pack("<2f", cell, 0))
            for a in (vertices, faces, queries):
                fp.write(np.ascontiguousarray(a).tobytes())
        done = subprocess.run([exe, job, out], timeout=300, stderr=subprocess.PIPE)
        assert done.returncode == code, done.stderr.decode()
        if code:
            return done.stderr.decode()
        raw, arrays, at = open(out, "rb").read(), [], 0
        for dtype, shape in ((F, (nq,)), (I, (nq,)), (I, (nq,)), (F, (nq, 3)), (F, (nq, 2)), (np.int64, (ref.STAT_WORDS,)), (I, (4,))):
            n = int(np.prod(shape))
            arrays.append(np.frombuffer(raw, dtype, n, at).reshape(shape))
            at += n * np.dtype(dtype).itemsize
        assert at == len(raw)
        return arrays

    return SimpleNamespace(query=query)
