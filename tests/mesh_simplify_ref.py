"""csrc/gp_mesh_simplify.h restated in numpy: the keys as words, the clusters by np.unique numbered by their first occurrence (not by
the device's sort), the float64 means one addition at a time in member order, the faces by boolean masks, the duplicates by the first
occurrence of a rotated triple, the renumbering by cumulative sums."""
from types import SimpleNamespace

import numpy as np

import mesh_ref

F = np.float32
I = np.int32
MAX_DIM = 2 ** 21


def exact_bounds(vertices):
    """[8] float64: min xyz, max xyz over the finite coordinates (a zero is +0.0), the not-finite flag, 0."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    finite = np.isfinite(v)
    lo = np.where(finite, v, np.inf).min(axis=0).astype(np.float64) + 0.0
    hi = np.where(finite, v, -np.inf).max(axis=0).astype(np.float64) + 0.0
    return np.concatenate([lo, hi, [float(not finite.all()), 0.0]])


def plan_grid(voxel_size, bounds):
    """(origin [3] float64, dims [3] int), or the refusal as a string."""
    voxel = float(voxel_size)
    if not np.isfinite(voxel) or not voxel > 0:
        return "voxel_size must be finite and > 0"
    b = np.asarray(bounds, np.float64).reshape(6)
    if not np.isfinite(b).all() or (b[:3] > b[3:]).any():
        return "bounds must be finite with min <= max"
    origin = b[:3] - voxel / 2
    dims = np.floor((b[3:] + voxel / 2 - origin) / voxel) + 1.0
    if not (dims <= MAX_DIM).all():
        return "voxel_size is too small"
    return origin, np.maximum(dims, 1).astype(np.int64)


def keys(vertices, voxel_size=None, bounds=None):
    """(status, [nv, 3] uint32): weld keys without a voxel_size, grid keys with one (bounds: [6], min then max)."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    if voxel_size is None:
        w = np.ascontiguousarray(v).view(np.uint32).copy()
        w[w == 0x80000000] = 0
        return 0, w
    origin, dims = plan_grid(voxel_size, bounds)
    with np.errstate(all="ignore"):
        q = np.floor((v.astype(np.float64) - origin) / float(voxel_size))
    inside = (q >= 0) & (q < dims)                       # (false for a NaN)
    return int(not inside.all()), np.where(inside, q, 0).astype(np.int64).astype(np.uint32)


def clusters(key):
    """(cluster [nv] int32, C): equal keys, numbered in ascending order of their smallest member."""
    nv = len(key)
    if nv == 0:
        return np.zeros(0, I), 0
    _, inverse = np.unique(key, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    first = np.full(int(inverse.max()) + 1, nv, np.int64)
    np.minimum.at(first, inverse, np.arange(nv))
    number = np.empty(len(first), np.int64)
    number[np.argsort(first)] = np.arange(len(first))
    return number[inverse].astype(I), len(first)


def contract(rows, cluster, C, contraction):
    """[C, k] float32: per cluster the first member's row, or the float64 sum in ascending member order from +0.0 over the count."""
    rows = np.asarray(rows, F)
    order = np.argsort(cluster, kind="stable")
    sorted_cluster = cluster[order]
    begin = np.searchsorted(sorted_cluster, np.arange(C), side="left")
    if contraction == "first":
        return rows[order[begin]].reshape(C, rows.shape[1])
    assert contraction == "average"
    turn = np.arange(len(order)) - begin[sorted_cluster]
    by_turn = np.argsort(turn, kind="stable")
    cuts = np.searchsorted(turn[by_turn], np.arange(int(turn.max()) + 2 if len(turn) else 1))
    total = np.zeros((C, rows.shape[1]), np.float64)
    with np.errstate(all="ignore"):
        for k in range(len(cuts) - 1):                   # one member per cluster and turn: every addition is a single float64 one
            sel = order[by_turn[cuts[k]:cuts[k + 1]]]
            total[cluster[sel]] = total[cluster[sel]] + rows[sel].astype(np.float64)
        return (total / np.bincount(cluster, minlength=C).astype(np.float64)[:, None]).astype(F)


def rotate(g):
    """[n, 3]: every triple rotated so that its smallest entry comes first."""
    s = np.argmin(g, axis=1)
    n = np.arange(len(g))
    return np.stack([g[n, s], g[n, (s + 1) % 3], g[n, (s + 2) % 3]], axis=1)


def simplify(vertices, faces, rows=(), voxel_size=None, bounds=None, contraction="average", drop_zero_area=False, drop_duplicates=True,
             keep_unreferenced=False):
    """voxel_size None: weld (always "first").  bounds None: the exact bounds.  A namespace of status, vertices, faces, vertex_map,
    face_index, vertex_counts, rows (a list), stats."""
    vertices, faces = np.asarray(vertices, F).reshape(-1, 3), np.asarray(faces, I).reshape(-1, 3)
    nv = len(vertices)
    if voxel_size is None:
        contraction = "first"
    elif bounds is None:
        bounds = exact_bounds(vertices)[:6] if nv else np.zeros(6)
    status, key = keys(vertices, voxel_size, bounds)
    cluster, C = clusters(key)
    positions = contract(vertices, cluster, C, contraction)
    good = mesh_ref.good_faces(faces, nv)
    status |= int(not good.all())
    g = np.zeros((len(faces), 3), I)
    g[good] = cluster[faces[good]]
    collapsed = good & ((g[:, 0] == g[:, 1]) | (g[:, 1] == g[:, 2]) | (g[:, 0] == g[:, 2]))
    alive = good & ~collapsed
    zero = np.zeros(len(faces), bool)
    if drop_zero_area:
        zero[alive] = (mesh_ref.face_vectors(positions, g[alive]) == 0).all(axis=1)          # (a NaN is not zero)
        alive &= ~zero
    duplicate = np.zeros(len(faces), bool)
    if drop_duplicates:
        ids = np.flatnonzero(alive)
        _, firsts = np.unique(rotate(g[ids]), axis=0, return_index=True) if len(ids) else (None, np.zeros(0, np.int64))
        duplicate[ids] = True
        duplicate[ids[firsts]] = False
        alive &= ~duplicate
    keep = np.ones(C, bool) if keep_unreferenced else np.zeros(C, bool)
    keep[g[alive].reshape(-1)] = True
    new_id = (np.cumsum(keep) - 1).astype(I)
    vertex_map = np.where(keep[cluster], new_id[cluster], -1).astype(I) if nv else np.zeros(0, I)
    stats = dict(clusters=C, collapsed=int(collapsed.sum()), zero_area=int(zero.sum()), duplicates=int(duplicate.sum()), unreferenced=int(C - keep.sum()))
    return SimpleNamespace(status=status, vertices=positions[keep], faces=new_id[g[alive]].astype(I).reshape(-1, 3), vertex_map=vertex_map,
                           face_index=np.flatnonzero(alive).astype(I), vertex_counts=np.bincount(cluster, minlength=C)[keep].astype(I),
                           rows=[contract(r, cluster, C, contraction)[keep] for r in rows], stats=stats, cluster=cluster, key=key)
