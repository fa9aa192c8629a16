"""Seeded cases of the geometry metrics, shared by the host test (the stand-alone build of csrc/geometry_core.h) and the GPU test
(geometry_ops).  Small on purpose; each names what it can break.

CLOUDS (points, queries): the nearest neighbour on a grid against the brute force, each under every rule of RULES
  uniform         3000 uniform points, 200 queries reaching 30 % outside the bounds: clamped home cells, rings of 2 and more
  shifted         the same moved by 10^6: an ulp of a coordinate is 0.0625, a cell of the finer rules is smaller
  lattice         an 8^3 lattice in shuffled order, queries at the cell centres: eight equidistant points, the smallest index wins
  repeated        50 points, each 20 times: ties at distance 0 and at every other
  identical       70 times one point: extent 0, one cell
  collinear, coplanar      one or two flat axes
  boundaries      points exactly on cell boundaries of the rule of 7, queries on them and beside them
  sphere          3000 points on a sphere, queries 1 % outside it: most cells are empty
  far             20 queries at 50 times the extent: the walk ends with the pass over all records
  sizes_*         np of 1, 63, 64, 65, 257 with nq of 1, 255, 256, 257, 256: wave and workgroup boundaries
  nonfinite       NaN and infinity among points and queries
  none_usable     every point has a NaN: every query gets (+inf, -1)
  overflow        coordinates near 3e38, point 0 unusable: every float32 distance is +inf and the answer is (+inf, 1), not -1; one cell
MESHES: the meshes of the sampling (33_sphere and 33_torus of tsdf_cases, small meshes of mesh_render_cases, degenerate ones)
METRICS: pairs of dist2 arrays around the tile size, with entries that do not count"""
import functools
from types import SimpleNamespace

import numpy as np

import geometry_ref as ref
import mesh_render_cases
import tsdf_cases

F = np.float32
I = np.int32
RULES = ("1", "2", "7", "auto", "1024")          # cells along the longest axis; 1024 is halved to the 2^24 cells
THRESHOLDS = (0.05, 0.1, 0.25)
SAMPLES = 5000
ATTRIBUTES = 4


def _uniform():
    rng = np.random.default_rng(1)
    p = rng.uniform(0, 1, (3000, 3)).astype(F)
    q = rng.uniform(-0.3, 1.3, (200, 3)).astype(F)
    return p, q


def _clouds():
    C = {}
    p, q = _uniform()
    C["uniform"] = (p, q)
    C["shifted"] = ((p + F(1e6)).astype(F), (q + F(1e6)).astype(F))
    rng = np.random.default_rng(2)
    g = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    C["lattice"] = (g[rng.permutation(len(g))].astype(F), (g[(g < 7).all(axis=1)] + 0.5).astype(F))
    base = rng.uniform(-2, 2, (50, 3)).astype(F)
    C["repeated"] = (np.tile(base, (20, 1))[rng.permutation(1000)], np.concatenate([base[:25], rng.uniform(-2, 2, (40, 3)).astype(F)]))
    C["identical"] = (np.tile(np.array([[0.25, -1.5, 3.0]], F), (70, 1)), rng.uniform(-4, 4, (30, 3)).astype(F))
    line = rng.uniform(0, 5, (400, 1)).astype(F)
    C["collinear"] = (np.concatenate([line, np.full_like(line, 2), np.full_like(line, -1)], axis=1), rng.uniform(-1, 6, (60, 3)).astype(F))
    plane = rng.uniform(-1, 1, (1500, 2)).astype(F)
    C["coplanar"] = (np.concatenate([plane, np.full((1500, 1), 0.5, F)], axis=1), rng.uniform(-1.2, 1.2, (80, 3)).astype(F))
    edges = (np.arange(8) * 0.5).astype(F)                         # extent 3.5, rule 7: cells of 0.5
    b = np.stack(np.meshgrid(edges, edges, edges, indexing="ij"), axis=-1).reshape(-1, 3)
    C["boundaries"] = (b, np.concatenate([b[::3], np.nextafter(b[::5], F(10)), np.nextafter(b[::7], F(-10)), b[::4] + F(0.25)]).astype(F))
    n = rng.normal(size=(3000, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    C["sphere"] = ((1.5 * n).astype(F), (1.5 * 1.01 * n[::15]).astype(F))
    C["far"] = (p, ((rng.uniform(-1, 1, (20, 3)) * 50) + 0.5).astype(F))
    for np_, nq in ((1, 1), (63, 255), (64, 256), (65, 257), (257, 256)):
        C[f"sizes_{np_}"] = (rng.uniform(-1, 1, (np_, 3)).astype(F), rng.uniform(-1.2, 1.2, (nq, 3)).astype(F))
    bp, bq = rng.uniform(-1, 1, (300, 3)).astype(F), rng.uniform(-1, 1, (100, 3)).astype(F)
    bp[::17, 0], bp[5::29, 2], bp[7::31, 1] = np.nan, np.inf, -np.inf
    bq[::9, 1], bq[4::13, 0] = np.nan, np.inf
    C["nonfinite"] = (bp, bq)
    C["none_usable"] = (np.full((40, 3), np.nan, F), rng.uniform(-1, 1, (10, 3)).astype(F))
    huge = (rng.uniform(0.5, 1, (50, 3)) * 3e38).astype(F)
    huge[0, 1] = np.nan
    C["overflow"] = (huge, np.concatenate([-huge[5:17], np.zeros((1, 3), F)]).astype(F))
    return C


CLOUDS = _clouds()
NEAREST_RUNS = [(name, rule) for name in CLOUDS for rule in RULES]


def cell_of(name, rule):
    """The cell size that gives `rule` cells along the longest axis of the cloud's usable points (0.0: the automatic rule)."""
    if rule == "auto":
        return 0.0
    p = CLOUDS[name][0]
    p = p[np.isfinite(p).all(axis=1)]
    extent = float((p.max(axis=0).astype(np.float64) - p.min(axis=0)).max()) if len(p) else 0.0
    return float(F(extent / int(rule))) if extent > 0 else 1.0


@functools.lru_cache(maxsize=None)
def nearest_result(name):
    """geometry_ref.nearest of a cloud (no rule enters it); do not modify."""
    p, q = CLOUDS[name]
    return ref.nearest(q, p)


def _meshes():
    M = {}
    for volume in ("33_sphere", "33_torus"):
        _, vertices, _, faces = tsdf_cases.extracted(volume)
        M[volume] = (np.ascontiguousarray(vertices, F), np.ascontiguousarray(faces, I))
    for name in ("diagonal", "fan", "slivers", "bad_index", "random"):
        c = mesh_render_cases.CASES[name]
        M[name] = (c.vertices, c.faces)
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [0, 0, np.inf], [3, 3, 3]], F)
    M["mixed"] = (v, np.array([[0, 1, 2], [0, 1, 3], [4, 1, 2], [0, 1, 9], [5, 5, 5], [2, 1, 0], [-1, 0, 1]], I))      # one area twice; NaN, inf, bad, zero
    M["uneven"] = (np.array([[0, 0, 0], [1000, 0, 0], [0, 1000, 0], [0, 0, 1e-3], [1e-3, 0, 0]], F), np.array([[0, 1, 2], [0, 3, 4]], I))      # 10^12 to 1 in area
    M["no_area"] = (np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], F), np.array([[0, 1, 2], [0, 0, 1]], I))
    M["no_faces"] = (np.zeros((3, 3), F), np.zeros((0, 3), I))
    return M


MESHES = _meshes()
REFUSED = ("no_area", "no_faces")
SAMPLE_RUNS = [(name, SAMPLES if name.startswith("33_") else 300) for name in MESHES]


def attributes_of(name):
    return np.random.default_rng(50).uniform(-1, 1, (len(MESHES[name][0]), ATTRIBUTES)).astype(F)


@functools.lru_cache(maxsize=None)
def sample_result(name, n, seed=0):
    """geometry_ref.sample_surface of a mesh; do not modify."""
    v, f = MESHES[name]
    return ref.sample_surface(v, f, n, seed, attributes_of(name))


def _metrics():
    rng = np.random.default_rng(3)
    M = {}
    for name, (na, nb) in {"one": (1, 1), "tile": (1023, 1025), "tiles": (5000, 3000), "many": (300000, 1024), "empty_b": (10, 0)}.items():
        a, b = (rng.uniform(0, 0.3, n).astype(F) ** 2 for n in (na, nb))
        if na > 100:
            a[::97] = np.inf
            b[3::101] = np.inf
        M[name] = (a.astype(F), b.astype(F))
    M["nothing_counts"] = (np.full(5, np.inf, F), np.array([0.01, 0.04], F))
    return M


METRICS = _metrics()


@functools.lru_cache(maxsize=None)
def metrics_result(name):
    a, b = METRICS[name]
    return ref.metrics(a, b, THRESHOLDS)


def lattice_pair(s=0.25, t=0.0625, k=6):
    """A k^3 lattice of spacing s and the same moved by t < s / 2 along x, exactly representable."""
    g = np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(F) * F(s)
    return g, (g + np.array([t, 0, 0], F)).astype(F)


def sphere_points(n, seed=9):
    """n points on tsdf_cases.SPHERE, computed analytically."""
    d = np.random.default_rng(seed).normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (np.asarray(tsdf_cases.SPHERE.c, np.float64) + tsdf_cases.SPHERE.r * d).astype(F)


SPHERE_BOUND = np.sqrt(3.0) * tsdf_cases.EXTRACT["33_sphere"][0].voxel          # a sample lies in a cell the surface crosses


# ---- the stand-alone build of csrc/geometry_core.h, as a child process ----
def build_emulator(d, sanitize):
    """tests/geometry_emulate.cpp built into `d` (a pathlib directory), under the sanitizers where `sanitize` is set (the host test's; a GPU test
    builds plain); returns an object with samples(),
    nearest() and metrics(), each one run of the child, and refused(head, arrays), the words of a refusal."""
    import struct
    import subprocess

    import emulate_build
    exe = emulate_build.build("geometry_emulate", d, sanitize=sanitize)

    def run(head, arrays, code=0):
        job, out = str(d / "job.bin"), str(d / "out.bin")
        with open(job, "wb") as fp:
            fp.write(head)
            for a in arrays:
                fp.write(np.ascontiguousarray(a).tobytes())
        done = subprocess.run([exe, job, out], timeout=300, stderr=subprocess.PIPE)
        assert done.returncode == code, done.stderr.decode()
        return done.stderr.decode() if code else open(out, "rb").read()

    def split(raw, shapes):
        out, at = [], 0
        for dtype, shape in shapes:
            n = int(np.prod(shape))
            out.append(np.frombuffer(raw, dtype, n, at).reshape(shape))
            at += n * np.dtype(dtype).itemsize
        assert at == len(raw)
        return out

    def samples(vertices, faces, n, seed=0, attributes=None, code=0):
        k = 0 if attributes is None else attributes.shape[1]
        raw = run(struct.pack("<8i", 0, len(vertices), len(faces), n, k, 0, 0, 0) + struct.pack("<Q", seed), [vertices, faces] + ([attributes] if k else []), code)
        return raw if code else split(raw, [(I, (8,)), (F, (n, 3)), (I, (n,)), (F, (n, 2)), (F, (n, k))])

    def nearest(points, queries, cell=0.0, backwards=False, code=0):
        raw = run(struct.pack("<8i", 1, len(points), len(queries), int(backwards), 0, 0, 0, 0) + struct.pack("<2f", cell, 0), [points, queries], code)
        return raw if code else split(raw, [(F, (len(queries),)), (I, (len(queries),)), (np.int64, (8,)), (I, (4,))])

    def metrics(ab, ba, thresholds=THRESHOLDS, nt=None, code=0):
        t = list(thresholds) + [0.0] * (8 - len(thresholds))
        raw = run(struct.pack("<8i", 2, len(ab), len(ba), len(thresholds) if nt is None else nt, 0, 0, 0, 0) + struct.pack("<8f", *t), [ab, ba], code)
        return raw if code else split(raw, [(np.float64, (ref.COLUMNS,))])[0]

    return SimpleNamespace(samples=samples, nearest=nearest, metrics=metrics)


# ---- facts that do not come from the restatement: the same checks for the emulator's output and for the device's ----
def check_samples(vertices, faces, weights, n, points, face, bary):
    """Every sample lies in its face's plane and inside the face, to a float32 bound from the corner magnitudes; the count of every face
    is within 2 of n * w_f / T.  Returns (the largest error over its bound, the largest count deviation)."""
    vertices, faces = np.asarray(vertices, np.float64), np.asarray(faces)
    assert (face >= 0).all() and (face < len(faces)).all() and (weights[face] > 0).all()
    corners = vertices[faces[face]]                                        # [n, 3, 3]
    a, b, c = corners[:, 0], corners[:, 1], corners[:, 2]
    u1, u2 = bary[:, 0].astype(np.float64), bary[:, 1].astype(np.float64)
    assert (u1 >= 0).all() and (u2 >= 0).all() and (u1 + u2 <= 1).all()    # inside the face: exact in the integers k / 2^24
    exact = a + u1[:, None] * (b - a) + u2[:, None] * (c - a)
    # six float32 operations per component, none on a value beyond 3 M (M the largest corner magnitude): 16 * 2^-24 * M covers them
    bound = 16 * 2.0 ** -24 * np.abs(corners).max(axis=(1, 2)) + 1e-45
    error = np.abs(points.astype(np.float64) - exact).max(axis=1)
    assert (error <= bound).all(), float((error / bound).max())
    normal = np.cross(b - a, c - a)
    length = np.linalg.norm(normal, axis=1)
    off = np.abs(((points.astype(np.float64) - a) * normal).sum(axis=1)) / np.where(length > 0, length, 1)
    assert (off <= np.sqrt(3.0) * bound).all()                             # in the face's plane
    expected = n * weights.astype(np.float64) / float(weights.astype(object).sum())
    deviation = np.abs(np.bincount(face, minlength=len(faces)) - expected)
    assert (deviation < 2).all(), float(deviation.max())
    return float((error / bound).max()), float(deviation.max())


def check_sphere_samples(points):
    """Every sample of 33_sphere lies within sqrt(3) voxels of the analytic sphere.  Returns the largest distance."""
    d = np.abs(np.linalg.norm(points.astype(np.float64) - np.asarray(tsdf_cases.SPHERE.c, np.float64), axis=1) - tsdf_cases.SPHERE.r)
    assert (d <= SPHERE_BOUND).all(), float(d.max())
    return float(d.max())


def row_dict(row, nt=len(THRESHOLDS)):
    names = ("accuracy", "completeness", "chamfer_l1", "chamfer_l2", "hausdorff")
    out = {k: float(row[ref.ACCURACY + i]) for i, k in enumerate(names)}
    for name, at in (("precision", ref.PRECISION), ("recall", ref.RECALL), ("fscore", ref.FSCORE)):
        out[name] = [float(row[at + k]) for k in range(nt)]
    return out


def check_metric_facts(distance):
    """distance(a, b, thresholds) -> a dict with accuracy, completeness, ..., precision, recall, fscore (lists) and, as "index_ab", the
    nearest indices of a in b.  The facts: a cloud against itself; a shifted lattice; swapping; thresholds beyond the range."""
    p = CLOUDS["uniform"][0][:700]
    same = distance(p, p, (0.0, 0.5))
    assert same["accuracy"] == same["completeness"] == same["chamfer_l1"] == same["chamfer_l2"] == same["hausdorff"] == 0.0
    assert same["fscore"] == [1.0, 1.0] and same["precision"] == [1.0, 1.0] and np.array_equal(same["index_ab"], np.arange(700))
    s, t = 0.25, 0.0625
    g, moved = lattice_pair(s, t)
    lat = distance(g, moved, (t / 2, t, 2 * t))
    for k in ("accuracy", "completeness", "hausdorff", "chamfer_l1"):
        assert abs(lat[k] - t) <= 2.0 ** -23 * 2, (k, lat[k])          # (these coordinates are exact in float32: the distance is t itself)
    assert lat["precision"] == [0.0, 1.0, 1.0] and lat["recall"] == [0.0, 1.0, 1.0] and lat["fscore"] == [0.0, 1.0, 1.0]
    a, b = CLOUDS["uniform"][0][:900], CLOUDS["sphere"][0][:500] * F(0.3) + F(0.5)
    one, two = distance(a, b, THRESHOLDS), distance(b, a, THRESHOLDS)
    assert one["accuracy"] == two["completeness"] and one["completeness"] == two["accuracy"] and one["precision"] == two["recall"] and one["recall"] == two["precision"]
    assert one["hausdorff"] == two["hausdorff"] and one["accuracy"] != one["completeness"] and one["fscore"] == two["fscore"]
    ends = distance(a, b, (1e-9, 100.0))
    assert ends["precision"] == [0.0, 1.0] and ends["recall"] == [0.0, 1.0] and ends["fscore"] == [0.0, 1.0]
    return lat
