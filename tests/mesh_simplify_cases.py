"""The meshes and option sets of the mesh-simplification tests (tests/test_mesh_simplify_host.py on the CPU,
tests/test_gpu_mesh_simplify.py on the device) and what tests/mesh_simplify_ref.py makes of them, computed once.  Built on
tests/mesh_cases.py where possible; each is the smallest shape at which a rule can go wrong: see DESIGN section 28."""
import functools
from types import SimpleNamespace

import numpy as np

import mesh_cases
import mesh_simplify_ref as ref
import tsdf_cases

F = np.float32
I = np.int32
mesh = mesh_cases.mesh

CUBE_SIDE = 1.5


def _cube_soup(s=CUBE_SIDE):
    """A cube as triangle soup: 12 faces with three vertices of their own each, outward; one of the zeros is -0.0."""
    corners = []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for side in (0.0, s):
            quad = []
            for a, b in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = [0.0, 0.0, 0.0]
                p[axis], p[u], p[v] = side, a * s, b * s
                quad.append(p)
            if side == 0.0:
                quad.reverse()                           # (u x v points along +axis)
            corners += [quad[0], quad[1], quad[2], quad[0], quad[2], quad[3]]
    vertices = np.array(corners, F)
    assert vertices.shape == (36, 3) and vertices[0, 0] == 0
    vertices[0, 0] = -0.0
    return mesh(vertices, np.arange(36).reshape(12, 3), 31)


def _collapse():
    """voxel 1 on the box (0, 0, 0) .. (4, 4, 4): face 0 has two corners in one cell, face 1 all three, face 2 none, face 3 shares
    face 2's cells."""
    vertices = [[0.1, 0.1, 0.1], [0.3, 0.2, 0.1], [2.0, 0.1, 0.2],            # 0 and 1 share a cell
                [3.1, 3.1, 3.1], [3.2, 3.3, 3.1], [3.4, 3.2, 3.3],            # one cell
                [0.0, 2.0, 0.0], [2.0, 2.0, 0.0], [0.0, 4.0, 0.0],
                [0.2, 2.1, 0.2], [2.2, 2.3, 0.1], [0.3, 3.9, 0.3]]            # the cells of 6, 7, 8
    return mesh(vertices, [[0, 1, 2], [3, 4, 5], [6, 7, 8], [10, 11, 9]], 32)


def _duplicates():
    """One triple in its three rotations, an exact copy, its flip, and another face: the first, the flip and the other stay."""
    return mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 1, 2], [0, 2, 1], [0, 1, 3]], 33)


def _zero_area():
    """Face 0: three distinct collinear vertices; face 1: a face vector of NaNs, which stays; face 2: an ordinary face."""
    return mesh([[0, 0, 0], [1, 1, 1], [2, 2, 2], [np.nan, 0, 0], [0, 1, 0], [1, 0, 0]], [[0, 1, 2], [0, 1, 3], [0, 5, 4]], 34)


BOUNDARY = SimpleNamespace(voxel=0.25, bounds=((0.0, 0.0, 0.0), (2.0, 2.0, 2.0)), at=0.375)


def _cell_boundary():
    """voxel 0.25 on the box (0, 0, 0) .. (2, 2, 2): origin -0.125, so 0.375 is (p - origin) / voxel = 2 exactly; per axis that value
    and its float32 neighbours on either side."""
    at = F(BOUNDARY.at)
    below, above = np.nextafter(at, F(0)), np.nextafter(at, F(1))
    vertices = []
    for axis in range(3):
        for value in (below, at, above):
            p = [1.0, 1.0, 1.0]
            p[axis] = value
            vertices.append(p)
    vertices += [[1.6, 1.6, 1.6], [0.1, 1.9, 0.2]]
    faces = [[0, 1, 9], [1, 2, 9], [3, 4, 10], [4, 5, 10], [6, 7, 9], [7, 8, 10], [0, 3, 6], [2, 5, 8], [1, 4, 7]]
    return mesh(vertices, faces, 35)


def _lost_cluster():
    """Face 0 lies in one cell and collapses: its cluster is named by no kept face."""
    return mesh([[0.1, 0.1, 0.1], [0.2, 0.1, 0.1], [0.1, 0.2, 0.1], [2, 0, 0], [4, 0, 0], [2, 2, 0], [9, 9, 9]], [[0, 1, 2], [3, 4, 5]], 36)


def _fan_wide(seed=38):
    """mesh_cases' fan with every rim vertex scaled by a power of two between 2^-30 and 2^10.  The float64 sum of the plain fan's
    float32 coordinates is exact in any order (24-bit values of about one magnitude, 5002 of them, in 53 bits); here it rounds, so
    the order of the members shows in the mean."""
    fan = mesh_cases.CASES["fan"]
    rng = np.random.default_rng(seed)
    vertices = fan.vertices.copy()
    vertices[1:] *= np.exp2(rng.integers(-30, 11, len(vertices) - 1)).astype(F)[:, None]
    return mesh(vertices, fan.faces, seed)


def _equal_iso():
    out = tsdf_cases.extracted("13x11x7_equal_iso")
    return mesh(out[1], out[3], 37)


def _cases():
    c = {name: mesh_cases.CASES[name] for name in ("empty", "no_faces", "one_triangle", "shared_vertex", "fan", "strip", "many_small", "two_spheres")}
    c.update(cube_soup=_cube_soup(), collapse=_collapse(), duplicates=_duplicates(), zero_area=_zero_area(), cell_boundary=_cell_boundary(),
             lost_cluster=_lost_cluster(), fan_wide=_fan_wide(), equal_iso=_equal_iso())
    return c


CASES = _cases()


def W(**kw):
    return dict(voxel_size=None, **kw)


def G(voxel_size, **kw):
    return dict(voxel_size=voxel_size, **kw)


def box(name):
    """A box of whole numbers around a case: bounds to hand in."""
    v = CASES[name].vertices.astype(np.float64)
    return (tuple(np.floor(v.min(axis=0)).tolist()), tuple(np.ceil(v.max(axis=0)).tolist())) if len(v) else ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


OTHER = dict(drop_zero_area=True, drop_duplicates=False, keep_unreferenced=True)
FOUR = ((0.0, 0.0, 0.0), (4.0, 4.0, 4.0))
# the option sets of every case (mesh_simplify_ref.simplify's keywords)
RUNS = {
    "empty": [W(), W(**OTHER), G(0.5), G(0.5, contraction="first", bounds=FOUR, **OTHER)],
    "no_faces": [W(), W(keep_unreferenced=True), G(4.0, keep_unreferenced=True), G(4.0), G(3.0, contraction="first", bounds=box("no_faces"), keep_unreferenced=True)],
    "one_triangle": [W(), W(**OTHER), G(0.5), G(0.5, contraction="first", bounds=FOUR), G(8.0, keep_unreferenced=True)],
    "shared_vertex": [W(), W(**OTHER), G(1.5), G(1.5, contraction="first", bounds=box("shared_vertex"), **OTHER)],
    "cube_soup": [W(), W(**OTHER), G(0.5), G(1.0, contraction="first", bounds=FOUR, drop_zero_area=True)],
    "collapse": [W(), G(1.0, bounds=FOUR), G(1.0, bounds=FOUR, contraction="first", **OTHER), G(1.0)],
    "duplicates": [W(), W(drop_duplicates=False), W(**OTHER), G(0.25, bounds=FOUR)],
    "zero_area": [W(drop_zero_area=True), W(), W(**OTHER)],
    "cell_boundary": [G(BOUNDARY.voxel, bounds=BOUNDARY.bounds), G(BOUNDARY.voxel, bounds=BOUNDARY.bounds, contraction="first", **OTHER), W()],
    "lost_cluster": [G(1.0, bounds=((0.0, 0.0, 0.0), (9.0, 9.0, 9.0))), G(1.0, bounds=((0.0, 0.0, 0.0), (9.0, 9.0, 9.0)), keep_unreferenced=True), W(), W(keep_unreferenced=True)],
    "fan": [G(8.0, keep_unreferenced=True), G(8.0), W(), G(0.25, drop_zero_area=True), G(0.25, contraction="first", bounds=box("fan"))],
    "fan_wide": [G(8192.0, keep_unreferenced=True), G(8192.0, contraction="first", bounds=box("fan_wide"), keep_unreferenced=True), W()],
    "strip": [G(2.0), W(), G(2.0, contraction="first", bounds=box("strip"), **OTHER)],
    "many_small": [G(0.3), W(), G(0.3, contraction="first", bounds=box("many_small"), **OTHER)],
    "two_spheres": [G(0.05), G(0.1), G(0.4), W(), G(0.1, contraction="first", bounds=box("two_spheres"), **OTHER)],
    "equal_iso": [W(drop_zero_area=True), W(), G(0.2), G(0.2, contraction="first", bounds=box("equal_iso"), **OTHER)],
}
assert set(RUNS) == set(CASES)
# voxel_size -> (vertices kept, faces kept, collapsed, duplicates) of two_spheres on its own bounds, drop_zero_area off: from a sketch
# that shares no code with the restatement
TWO_SPHERES = {0.05: (1427, 2885, 4964, 7), 0.1: (423, 847, 7002, 7), 0.4: (34, 60, 7796, 0)}
BAD = mesh_cases.BAD
bad_faces = mesh_cases.bad_faces


def rows_of(m):
    return [m.colors, m.attribute]


@functools.lru_cache(maxsize=None)
def result(name, run):
    """mesh_simplify_ref.simplify of option set `run` of a case; do not modify."""
    m = CASES[name]
    return ref.simplify(m.vertices, m.faces, rows_of(m), **RUNS[name][run])


def runs_of(name):
    return list(range(len(RUNS[name])))


def parts(r):
    """The arrays of a result that are compared bit for bit, in the order the device hands them out."""
    return [r.vertices, r.faces, r.vertex_map, r.face_index, r.vertex_counts] + list(r.rows)


def check_properties(m, options, vertices, faces, vertex_map, vertex_counts):
    """What holds of any result, the restatement's or the device's: the counts against the map; under "average" every vertex in its
    cell's box to 2^-22 max|coordinate| (float32's half ulp with a margin of four)."""
    nv, nv2 = len(m.vertices), len(vertices)
    assert vertex_map.shape == (nv,) and vertex_counts.shape == (nv2,) and (vertex_counts >= 1).all()
    dropped = vertex_map < 0
    assert (vertex_map[dropped] == -1).all() and (vertex_map[~dropped] < nv2).all()
    assert np.array_equal(np.bincount(vertex_map[~dropped], minlength=nv2), vertex_counts)          # the members of the kept clusters, and only they
    if options.get("keep_unreferenced"):
        assert not dropped.any() and int(vertex_counts.sum()) == nv
    else:
        assert int(vertex_counts.sum()) + int(dropped.sum()) == nv
        assert len(np.unique(faces)) == nv2                       # every kept vertex is named by a kept face
    assert len(faces) == 0 or (faces.min() >= 0 and faces.max() < nv2)
    assert not len(faces) or ((faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])).all()
    if options["voxel_size"] is not None and options.get("contraction", "average") == "average" and nv:
        voxel = float(options["voxel_size"])
        bounds = np.concatenate(options["bounds"]) if options.get("bounds") is not None else ref.exact_bounds(m.vertices)[:6]
        origin, _ = ref.plan_grid(voxel, bounds)
        _, key = ref.keys(m.vertices, voxel, bounds)
        cell = np.zeros((nv2, 3), np.float64)
        cell[vertex_map[~dropped]] = key[~dropped].astype(np.float64)
        lo = origin + cell * voxel
        tol = 2.0 ** -22 * float(np.abs(m.vertices).max())
        v = vertices.astype(np.float64)
        assert (v >= lo - tol).all() and (v <= lo + voxel + tol).all()
