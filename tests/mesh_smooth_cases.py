"""The meshes, rows and option sets of the mesh-topology and smoothing tests (tests/test_mesh_smooth_host.py on the CPU,
tests/test_gpu_mesh_smooth.py on the device) and what tests/mesh_smooth_ref.py makes of them, computed once.  Built on
tests/mesh_cases.py and tests/mesh_simplify_cases.py where possible; each is the smallest shape at which a rule can go wrong: see
DESIGN section 32."""
import functools
from types import SimpleNamespace

import numpy as np

import mesh_cases
import mesh_simplify_cases
import mesh_smooth_ref as ref

F = np.float32
I = np.int32
WIDTHS = (1, 4, 7)                           # the columns of the attribute rows; the positions are the rows of width 3
OCTAHEDRON = mesh_cases.OCTAHEDRON
TETRAHEDRON = (np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], F), np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], I))


def mesh(vertices, faces, seed):
    vertices, faces = np.asarray(vertices, F).reshape(-1, 3), np.asarray(faces, I).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    return SimpleNamespace(vertices=vertices, faces=faces, rows=[rng.normal(size=(len(vertices), k)).astype(F) for k in WIDTHS])


def _torus(n, m, seed):
    """A closed n x m grid on a torus, every quad cut in two, consistently wound, the vertex numbers permuted and the positions
    jittered: nv = n m, E = 3 n m, nf = 2 n m, every vertex of degree 6."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    a, b = 2 * np.pi * i / n, 2 * np.pi * j / m
    p = np.stack([(2 + 0.7 * np.cos(b)) * np.cos(a), (2 + 0.7 * np.cos(b)) * np.sin(a), 0.7 * np.sin(b)], axis=-1).reshape(-1, 3)
    p = p + rng.normal(scale=0.02, size=p.shape)
    number = rng.permutation(n * m)
    at = lambda di, dj: number[(((i + di) % n) * m + (j + dj) % m).reshape(-1)]          # noqa: E731
    faces = np.concatenate([np.stack([at(0, 0), at(1, 0), at(1, 1)], axis=1), np.stack([at(0, 0), at(1, 1), at(0, 1)], axis=1)])
    vertices = np.zeros((n * m, 3))
    vertices[number] = p
    return mesh(vertices, faces, seed)


def _hub(n=2000, seed=41):
    """A closed fan: a hub of degree n, the rim's radii over forty powers of two, so that the order of the hub's sum shows."""
    rng = np.random.default_rng(seed)
    a = 2 * np.pi * np.arange(n) / n
    rim = np.stack([np.cos(a), np.sin(a), rng.uniform(-0.3, 0.3, n)], axis=1) * np.exp2(rng.integers(-30, 11, n))[:, None]
    f = np.arange(n)
    return mesh(np.concatenate([[[0.0, 0.0, 0.5]], rim]), np.stack([np.zeros(n, I), 1 + f, 1 + (f + 1) % n], axis=1), seed)


def _isolated():
    """The octahedron with vertices no face names in front, in the middle and at the end."""
    place = np.array([2, 3, 4, 7, 8, 10])
    vertices = np.arange(39, dtype=np.float64).reshape(13, 3)
    vertices[place] = OCTAHEDRON[0]
    return mesh(vertices, place[OCTAHEDRON[1]], 42)


def _not_finite():
    v = TETRAHEDRON[0].copy()
    v[1, 0], v[2] = np.nan, [-0.0, 0.0, -0.0]
    m = mesh(v, TETRAHEDRON[1], 43)
    m.rows[1][3, 2], m.rows[1][0, 0], m.rows[2][1, 1] = np.inf, -0.0, -np.inf
    return m


def _cases():
    tri = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    quad = tri + [[1, 1, 0.5]]
    welded = mesh_simplify_cases.result("cube_soup", 0)
    soup = mesh_simplify_cases.CASES["cube_soup"]
    c = {
        "empty": mesh(np.zeros((0, 3)), np.zeros((0, 3)), 1),
        "no_faces": mesh(np.arange(15).reshape(5, 3), np.zeros((0, 3)), 2),
        "one_triangle": mesh(tri, [[0, 1, 2]], 3),
        "two_consistent": mesh(quad, [[0, 1, 2], [2, 1, 3]], 4),
        "two_inconsistent": mesh(quad, [[0, 1, 2], [1, 2, 3]], 5),               # both run 1 -> 2: wind = +2
        "two_inconsistent_down": mesh(quad, [[0, 2, 1], [2, 1, 3]], 6),          # both run 2 -> 1: wind = -2
        "tetrahedron": mesh(*TETRAHEDRON, 7),
        "octahedron": mesh(*OCTAHEDRON, 8),
        "three_on_an_edge": mesh(quad + [[0.5, 0.5, -1]], [[0, 1, 2], [2, 1, 3], [1, 2, 4]], 9),
        "duplicated_face": mesh(quad, [[0, 1, 2], [2, 1, 3], [0, 1, 2]], 10),
        "cube_soup": mesh(soup.vertices, soup.faces, 11),
        "cube_welded": mesh(welded.vertices, welded.faces, 12),
        "repeated_index": mesh(quad, [[1, 1, 3], [2, 2, 2], [0, 1, 2]], 13),
        "not_finite": _not_finite(),
        "isolated": _isolated(),
        "hub": _hub(),
    }
    for n, m in ((7, 9), (8, 8), (5, 13), (31, 33), (32, 32), (25, 41)):          # nv about one wave and about GP_MESH_TILE
        c[f"torus_{n * m}"] = _torus(n, m, 100 + n * m)
    c["torus_20022"] = _torus(141, 142, 99)
    return c


CASES = _cases()
LARGE = "torus_20022"


def S(iterations, method="taubin", boundary="fixed", lambda_=0.5, mu=-0.53):
    return dict(iterations=iterations, method=method, boundary=boundary, lambda_=lambda_, mu=mu)


ALL = [S(i, m, b) for m in ("taubin", "laplacian") for b in ("fixed", "free") for i in (0, 1, 5)]
# the option sets of every case (mesh_smooth_ref.smooth's keywords): everything on the small ones; on the tiles what crosses them
RUNS = {name: ALL for name in CASES if not name.startswith("torus") and name != "hub"}
RUNS["hub"] = [S(1, "laplacian", "free"), S(5, "taubin", "fixed"), S(0)]
for _name in CASES:
    if _name.startswith("torus"):
        RUNS[_name] = [S(5, "taubin", "fixed"), S(1, "laplacian", "free", lambda_=0.3)]
RUNS[LARGE] = [S(1, "laplacian", "free"), S(5, "taubin", "fixed")]
VECTORISED = {(LARGE, 1)}                    # restated by step_vectorised, which the host test holds equal to the loop on every other run
assert set(RUNS) == set(CASES)
# face indices that must be refused: (case, face, corner, value relative to nv)
BAD = [("octahedron", 0, 1, -1), ("octahedron", 7, 2, 0), ("torus_1025", 1500, 0, 5), ("hub", 1999, 1, -7)]


def bad_faces(case, face, corner, value):
    m = CASES[case]
    faces = m.faces.copy()
    faces[face, corner] = len(m.vertices) + value if value >= 0 else value
    return faces


def runs_of(name):
    return list(range(len(RUNS[name])))


def table(m):
    """The positions and the attribute rows side by side: the columns do not know of each other, so one restatement serves all."""
    return np.concatenate([m.vertices] + m.rows, axis=1)


def split(t):
    return np.split(t, np.cumsum((3,) + WIDTHS)[:-1], axis=1)


@functools.lru_cache(maxsize=None)
def topology(name):
    """mesh_smooth_ref.edges of a case; do not modify."""
    m = CASES[name]
    return ref.edges(m.faces, len(m.vertices))


@functools.lru_cache(maxsize=None)
def smoothed(name, run):
    """[positions, rows of width 1, 4, 7] of option set `run` of a case; do not modify."""
    one_step = ref.step_vectorised if (name, run) in VECTORISED else ref.step
    return split(ref.smooth(table(CASES[name]), topology(name), one_step=one_step, **RUNS[name][run]))


@functools.lru_cache(maxsize=None)
def umbrella(name):
    return split(ref.umbrella(table(CASES[name]), topology(name)))


def check_properties(nv, nf, edge, face_count, wind, offsets, neighbors, vertex_flags, stats):
    """What holds of any topology, the restatement's or the device's."""
    ne = len(edge)
    assert edge.shape == (ne, 2) and face_count.shape == wind.shape == (ne,) and offsets.shape == (nv + 1,) and neighbors.shape == (2 * ne,) and vertex_flags.shape == (nv,)
    e = edge.astype(np.int64)
    assert (e[:, 0] < e[:, 1]).all() and (e >= 0).all() and (e < max(nv, 1)).all()
    key = e[:, 0] * max(nv, 1) + e[:, 1]
    assert (np.diff(key) > 0).all()                              # strictly ascending
    assert int(face_count.sum()) == 3 * stats["faces"] - stats["degenerate"] and (face_count >= 1).all()
    assert (np.abs(wind) <= face_count).all() and ((wind - face_count) % 2 == 0).all()
    assert offsets[0] == 0 and offsets[-1] == 2 * ne and (np.diff(offsets) >= 0).all()
    pairs = set()
    for v in range(nv):
        mine = neighbors[offsets[v]:offsets[v + 1]]
        assert (np.diff(mine) > 0).all() and v not in mine       # strictly ascending within each list
        pairs.update((v, int(u)) for u in mine)
    assert all((u, v) in pairs for v, u in pairs) and len(pairs) == 2 * ne          # the adjacency is symmetric
    assert {(min(p), max(p)) for p in pairs} == set(map(tuple, e.tolist()))
    degree = np.diff(offsets)
    assert np.array_equal((vertex_flags & 4) != 0, degree == 0) and stats["vertices"] == int((degree > 0).sum()) and stats["edges"] == ne
    assert stats["boundary"] == int((face_count == 1).sum()) and stats["nonmanifold"] == int((face_count > 2).sum())
    assert stats["euler"] == stats["vertices"] - ne + stats["faces"] and stats["faces"] <= nf
