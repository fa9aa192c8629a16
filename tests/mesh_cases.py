"""The meshes of the mesh-cleanup tests (tests/test_mesh_host.py on the CPU, tests/test_gpu_mesh.py on the device) and what
tests/mesh_ref.py makes of them, computed once.  Each is the smallest shape at which a kernel can go wrong: see DESIGN section 27."""
import functools
import math
from types import SimpleNamespace

import numpy as np

import mesh_ref as ref
import tsdf_ref

F = np.float32
I = np.int32


def mesh(vertices, faces, seed=None):
    vertices, faces = np.asarray(vertices, F).reshape(-1, 3), np.asarray(faces, I).reshape(-1, 3)
    rng = np.random.default_rng(1000 if seed is None else seed)
    return SimpleNamespace(vertices=vertices, faces=faces, colors=rng.uniform(0, 1, vertices.shape).astype(F),
                           attribute=rng.normal(size=(len(vertices), 5)).astype(F))


def _strip(n_faces=4096, seed=27):
    """Triangles (i, i + 1, i + 2) over n_faces + 2 vertices, the vertex numbers permuted: one component whose diameter is half its
    length, spanning several tiles."""
    nv = n_faces + 2
    rng = np.random.default_rng(seed)
    number = rng.permutation(nv)
    i = np.arange(nv)
    vertices = np.zeros((nv, 3), F)
    vertices[number] = np.stack([i // 2, i % 2, rng.uniform(-0.2, 0.2, nv)], axis=1)
    f = np.arange(n_faces)
    faces = number[np.stack([f, f + 1 + f % 2, f + 2 - f % 2], axis=1)]          # (alternating, so that the winding is consistent)
    return mesh(vertices, faces, seed)


def _fan(n_faces=5000, seed=28):
    rng = np.random.default_rng(seed)
    a = 2 * np.pi * np.arange(n_faces + 1) / (n_faces + 1)
    rim = np.stack([np.cos(a), np.sin(a), rng.uniform(-0.3, 0.3, n_faces + 1)], axis=1)
    f = np.arange(n_faces)
    return mesh(np.concatenate([[[0.0, 0.0, 0.5]], rim]), np.stack([np.zeros(n_faces, I), f + 1, f + 2], axis=1), seed)


OCTAHEDRON = (np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F),
              np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], I))


def _many_small(n=3000, seed=29):
    """n isolated triangles, then one octahedron: C = n + 1 > 1024."""
    rng = np.random.default_rng(seed)
    tri = rng.uniform(-1, 1, (n, 1, 3)) * 20 + rng.uniform(-0.5, 0.5, (n, 3, 3))
    vertices = np.concatenate([tri.reshape(-1, 3), OCTAHEDRON[0] + 40.0])
    faces = np.concatenate([np.arange(3 * n).reshape(n, 3), OCTAHEDRON[1] + 3 * n])
    return mesh(vertices, faces, seed)


TWO_SPHERES = SimpleNamespace(c0=(-0.3, 0.02, 0.01), r0=0.5, c1=(0.6, 0.1, 0.03), r1=0.15, n=33, origin=(-1.0, -1.0, -1.0), voxel=1.0 / 16, trunc=4.0 / 16)


def two_sphere_volume():
    """gp_tsdf.h's volume of the two-sphere field: 33^3 points, weight 1, no colour."""
    s = TWO_SPHERES
    vol = tsdf_ref.volume(s.n, s.n, s.n, s.origin, s.voxel, s.trunc, has_color=False)
    x, y, z = (a.astype(np.float64) for a in tsdf_ref.coords(vol))
    d0 = np.sqrt((x - s.c0[0]) ** 2 + (y - s.c0[1]) ** 2 + (z - s.c0[2]) ** 2) - s.r0
    d1 = np.sqrt((x - s.c1[0]) ** 2 + (y - s.c1[1]) ** 2 + (z - s.c1[2]) ** 2) - s.r1
    vol.tsdf = np.clip(np.minimum(d0, d1) / s.trunc, -1, 1).astype(F)
    vol.weight[:] = 1
    return vol


def _two_spheres():
    _, vertices, _, faces = tsdf_ref.extract(two_sphere_volume(), 0.0, 1.0)
    return mesh(vertices, faces, 30)


def _cases():
    tri = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    c = {
        "empty": mesh(np.zeros((0, 3)), np.zeros((0, 3))),
        "no_faces": mesh(np.arange(15).reshape(5, 3), np.zeros((0, 3))),
        "one_triangle": mesh(tri, [[0, 1, 2]]),
        "two_disjoint": mesh(tri + [[5, 5, 5], [6, 5, 5], [5, 5, 7]], [[3, 4, 5], [0, 1, 2]]),
        "shared_vertex": mesh(tri + [[-1, 0, 2], [0, -1, 3], [9, 9, 9]], [[2, 1, 0], [4, 0, 3]]),          # and vertex 5 is named by no face
        "repeated_index": mesh(tri + [[2, 2, 2]], [[1, 1, 3], [0, 1, 2]]),
        "collinear": mesh([[0, 0, 0], [1, 1, 1], [2, 2, 2], [0.5, 0.5, 0.5]], [[0, 1, 2], [2, 1, 3]]),
        "overflow": mesh([[0, 0, 0], [3e30, 0, 0], [0, 3e30, 0], [0, 0, 1]], [[0, 1, 2], [0, 1, 3]]),          # a face vector beyond float32: zeros, not NaN
        "strip": _strip(),
        "fan": _fan(),
        "many_small": _many_small(),
        "two_spheres": _two_spheres(),
    }
    return c


CASES = _cases()
STRIP_CAP = 4 * math.ceil(math.log2(len(CASES["strip"].vertices))) + 8          # the rounds a path of 4098 vertices may take
# (min_triangles, keep_largest) per case; every case also runs (None, None)
FILTERS = {"many_small": [(None, 1), (None, 2), (2, None), (1, 5), (None, 0)], "two_spheres": [(None, 1), (601, None), (600, 2)],
           "shared_vertex": [(None, 1), (3, None)], "two_disjoint": [(None, 1)], "strip": [(None, 1)], "fan": [(5001, None)]}
# face indices that must be refused: (case, face, corner, value relative to nv)
BAD = [("two_disjoint", 0, 1, -1), ("two_disjoint", 1, 2, 0), ("fan", 4999, 0, 0), ("many_small", 1500, 2, -1)]


def bad_faces(case, face, corner, value):
    m = CASES[case]
    faces = m.faces.copy()
    faces[face, corner] = len(m.vertices) + value if value >= 0 else value
    return faces


@functools.lru_cache(maxsize=None)
def components(name):
    """mesh_ref.components of a case; do not modify."""
    m = CASES[name]
    return ref.components(m.faces, len(m.vertices))


@functools.lru_cache(maxsize=None)
def filtered(name, min_triangles, keep_largest):
    m = CASES[name]
    return ref.filter_components(m.vertices, m.faces, [m.colors, m.attribute], min_triangles, keep_largest)


@functools.lru_cache(maxsize=None)
def normals(name):
    m = CASES[name]
    return ref.vertex_normals(m.vertices, m.faces)


def filters_of(name):
    return [(None, None)] + FILTERS.get(name, [])
