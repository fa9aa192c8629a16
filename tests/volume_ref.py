"""csrc/gp_volume.h's definitions restated in numpy, with no tree: the query is surface_ref.point_mesh (a brute force over every
face), the sign sdf_ref.sign on its float32-rounded row, the lattice points one EXACT float32 fma a coordinate (in fractions: a
float64 product and sum rounded again could round twice), the comparison's counts, and lattice_for's rule."""
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

import mesh_smooth_ref
import sdf_ref
import surface_ref

F = np.float32
I = np.int32
LEAF, STAT_WORDS, LATTICE_WORDS, COUNT_WORDS = 2, 8, 16, 6
STAT_NAMES = ("excluded_faces", "excluded_queries", "nodes", "candidates", "max_stack", "levels", "leaves", "status")
EXCLUDED_FACES, EXCLUDED_QUERIES, NODES, CANDIDATES, MAX_STACK, LEVELS, LEAVES, STATUS = range(8)
COUNT_NAMES = ("inside_a", "inside_b", "both", "either", "undetermined", "points")


def round32(x):
    """The float32 nearest to the fraction x, ties to the even mantissa (x within the finite range)."""
    near = F(float(x))
    best = None
    for c in (np.nextafter(near, F(-np.inf)), near, np.nextafter(near, F(np.inf))):
        if not np.isfinite(c):
            continue
        key = (abs(Fraction(float(c)) - x), int(np.array(c, F).view(np.uint32)) & 1)
        if best is None or key < best[0]:
            best = (key, c)
    return best[1]


def fma32(i, voxel, origin):
    """fmaf((float)i, voxel, origin), exactly: one rounding of the exact i * voxel + origin."""
    return round32(Fraction(float(F(i))) * Fraction(float(F(voxel))) + Fraction(float(F(origin))))


def lattice_points(origin, voxel, dims):
    """[nz * ny * nx, 3] float32, x fastest: the points of the lattice."""
    nx, ny, nz = (int(d) for d in dims)
    xs, ys, zs = (np.array([fma32(i, voxel, o) for i in range(n)], F) for n, o in zip((nx, ny, nz), origin))
    z, y, x = np.meshgrid(zs, ys, xs, indexing="ij")
    return np.ascontiguousarray(np.stack([x, y, z], axis=-1).reshape(-1, 3))


def levels(nf, leaf=LEAF):
    """(levels, leaves) of the tree of nf faces."""
    n = max(1, -(-nf // leaf))
    leaves, k = n, 1
    while n > 1:
        n, k = (n + 1) // 2, k + 1
    return k, leaves


def signed(queries, vertices, faces, surface=None):
    """SimpleNamespace(surface, topology, tables, signed) of queries against the mesh: what sdf_cases.result holds for a case.  surface:
    surface_ref.point_mesh of the same arguments, where the caller has it already."""
    surface = surface_ref.point_mesh(queries, vertices, faces) if surface is None else surface
    topology = mesh_smooth_ref.edges(faces, len(vertices))
    tables = sdf_ref.tables(vertices, faces, topology.edge)
    sg = sdf_ref.sign(queries, surface.dist2, surface.face, surface.region, vertices, faces, tables)
    return SimpleNamespace(surface=surface, topology=topology, tables=tables, signed=sg)


def lattice(vertices, faces, origin, voxel, dims):
    """signed() of the lattice's points, plus points and sdf [nz, ny, nx]."""
    points = lattice_points(origin, voxel, dims)
    out = signed(points, vertices, faces)
    nx, ny, nz = (int(d) for d in dims)
    out.points, out.sdf = points, out.signed.sdf.reshape(nz, ny, nx)
    return out


def compare(a, b):
    """gp_volume_compare's six counts."""
    a, b = np.asarray(a, F).reshape(-1), np.asarray(b, F).reshape(-1)
    ok = np.isfinite(a) & np.isfinite(b)
    ia, ib = ok & (a < 0), ok & (b < 0)
    return np.array([ia.sum(), ib.sum(), (ia & ib).sum(), (ia | ib).sum(), (~ok).sum(), len(a)], np.int64)


def lattice_for(vertices, voxel_size=None, resolution=128, margin=2):
    """volume_ops.lattice_for's rule on the stacked vertices of the meshes."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    v = v[np.isfinite(v).all(axis=1)].astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    voxel = float(F((hi - lo).max() / (resolution - 2 * margin - 2))) if voxel_size is None else float(F(voxel_size))
    origin = tuple(float(F(l - (margin + 0.5) * voxel)) for l in lo)
    dims = tuple(int(math.ceil(e / voxel)) + 2 * margin + 2 for e in (hi - lo))
    return origin, voxel, dims
