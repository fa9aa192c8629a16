"""csrc/gp_mesh_smooth.h restated in numpy, in float64 and in the header's operation order, with no sort tricks: np.unique on pairs
and a Python loop per vertex.  What the device and the stand-alone build (tests/mesh_smooth_emulate.cpp) are compared with, bit for
bit.  step_vectorised is the same arithmetic a neighbour rank at a time (the j-th neighbour of every vertex at once: each vertex's
own sum still runs in ascending order); the host test holds it equal to the loop and tools/mesh_smooth_probe.py times it."""
from types import SimpleNamespace

import numpy as np

F = np.float32
I = np.int32
COUNT_NAMES = ("status", "edges", "boundary", "nonmanifold", "inconsistent", "degenerate", "vertices", "faces")
MAX_ITERATIONS = 10000


def check_options(method, boundary, iterations, lambda_, mu):
    if method not in ("laplacian", "taubin"):
        return "method must be \"laplacian\" or \"taubin\""
    if boundary not in ("fixed", "free"):
        return "boundary must be \"fixed\" or \"free\""
    if not 0 <= iterations <= MAX_ITERATIONS:
        return "iterations must be 0 .. 10000"
    if not np.isfinite(lambda_) or not np.isfinite(mu):
        return "lambda_ and mu must be finite"
    return None


def edges(faces, nv):
    """SimpleNamespace(edge, face_count, wind, offsets, neighbors, vertex_flags, counts, stats, status) of faces [nf][3] over nv vertices."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < nv)).all(axis=1)
    status = int((~ok).any())
    kept = f[ok]
    half = np.concatenate([kept[:, [0, 1]], kept[:, [1, 2]], kept[:, [2, 0]]]) if len(kept) else np.zeros((0, 2), np.int64)
    degenerate = int((half[:, 0] == half[:, 1]).sum())
    half = half[half[:, 0] != half[:, 1]]
    forward = half[:, 0] < half[:, 1]
    pair = np.where(forward[:, None], half, half[:, ::-1])
    if len(pair):
        edge, inverse, face_count = np.unique(pair, axis=0, return_inverse=True, return_counts=True)
        inverse = inverse.reshape(-1)
        wind = np.bincount(inverse, weights=np.where(forward, 1, -1), minlength=len(edge)).astype(np.int64)
    else:
        edge, face_count, wind = np.zeros((0, 2), np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    ne = len(edge)
    lists = [[] for _ in range(nv)]
    for lo, hi in edge.tolist():
        lists[lo].append(hi)
        lists[hi].append(lo)
    lists = [sorted(l) for l in lists]
    degree = np.array([len(l) for l in lists], np.int64)
    offsets = np.concatenate([[0], np.cumsum(degree)]).astype(I)
    neighbors = np.array([u for l in lists for u in l], I)
    flags = np.zeros(nv, np.uint8)
    for mask, bit in ((face_count == 1, 1), (face_count > 2, 2)):
        flags[np.unique(edge[mask])] |= bit
    flags[degree == 0] |= 4
    counts = [status, ne, int((face_count == 1).sum()), int((face_count > 2).sum()), int(((face_count == 2) & (wind != 0)).sum()), degenerate, int((degree > 0).sum()),
              int(len(kept))]
    stats = dict(zip(COUNT_NAMES[1:], counts[1:]))
    stats["euler"] = counts[6] - ne + counts[7]
    stats["watertight"] = counts[2] == 0 and counts[3] == 0 and counts[4] == 0 and ne > 0
    return SimpleNamespace(edge=edge.astype(I).reshape(-1, 2), face_count=face_count.astype(I), wind=wind.astype(I), offsets=offsets, neighbors=neighbors,
                           vertex_flags=flags, counts=np.array(counts, I), stats=stats, status=status)


def edges_vectorised(faces, nv):
    """edges() without its loops, on packed 64-bit keys: for meshes of millions of faces (tools/mesh_smooth_probe.py); the host test
    holds it equal to edges()."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < nv)).all(axis=1)
    kept = f[ok]
    half = np.concatenate([kept[:, [0, 1]], kept[:, [1, 2]], kept[:, [2, 0]]]) if len(kept) else np.zeros((0, 2), np.int64)
    degenerate = int((half[:, 0] == half[:, 1]).sum())
    half = half[half[:, 0] != half[:, 1]]
    forward = half[:, 0] < half[:, 1]
    base = max(nv, 1)
    key, inverse, face_count = np.unique(np.where(forward, half[:, 0] * base + half[:, 1], half[:, 1] * base + half[:, 0]), return_inverse=True, return_counts=True)
    wind = np.bincount(inverse.reshape(-1), weights=np.where(forward, 1, -1), minlength=len(key)).astype(np.int64)
    edge = np.stack([key // base, key % base], axis=1)
    ne = len(edge)
    both = np.unique(np.concatenate([key, edge[:, 1] * base + edge[:, 0]]))
    offsets = np.searchsorted(both // base, np.arange(nv + 1)).astype(I)
    degree = np.diff(offsets)
    flags = np.zeros(nv, np.uint8)
    for mask, bit in ((face_count == 1, 1), (face_count > 2, 2)):
        flags[np.unique(edge[mask])] |= bit
    flags[degree == 0] |= 4
    counts = [int((~ok).any()), ne, int((face_count == 1).sum()), int((face_count > 2).sum()), int(((face_count == 2) & (wind != 0)).sum()), degenerate, int((degree > 0).sum()),
              int(len(kept))]
    stats = dict(zip(COUNT_NAMES[1:], counts[1:]))
    stats["euler"] = counts[6] - ne + counts[7]
    stats["watertight"] = counts[2] == 0 and counts[3] == 0 and counts[4] == 0 and ne > 0
    return SimpleNamespace(edge=edge.astype(I).reshape(-1, 2), face_count=face_count.astype(I), wind=wind.astype(I), offsets=offsets, neighbors=(both % base).astype(I),
                           vertex_flags=flags, counts=np.array(counts, I), stats=stats, status=counts[0])


def parts(t):
    """The arrays of a topology that are compared bit for bit, in the order the device hands them out."""
    return [t.edge, t.face_count, t.wind, t.offsets, t.neighbors, t.vertex_flags]


def _mean(src, t, v):
    begin, end = int(t.offsets[v]), int(t.offsets[v + 1])
    total = np.zeros(src.shape[1], np.float64)
    for u in t.neighbors[begin:end]:
        total = total + src[u].astype(np.float64)
    return total / np.float64(end - begin)


def step(src, t, s, pinned=None):
    """One step with factor s: the loop per vertex."""
    src = np.asarray(src, F)
    dst = src.copy()
    with np.errstate(all="ignore"):
        for v in range(len(src)):
            if t.offsets[v + 1] == t.offsets[v] or (pinned is not None and pinned[v]):
                continue
            p = src[v].astype(np.float64)
            d = _mean(src, t, v) - p
            d = np.float64(s) * d
            dst[v] = (p + d).astype(F)
    return dst


def step_vectorised(src, t, s, pinned=None):
    src = np.asarray(src, F)
    offsets = t.offsets.astype(np.int64)
    degree = np.diff(offsets)
    total = np.zeros(src.shape, np.float64)
    with np.errstate(all="ignore"):
        for j in range(int(degree.max()) if len(degree) else 0):
            rows = np.nonzero(degree > j)[0]
            total[rows] = total[rows] + src[t.neighbors[offsets[rows] + j]].astype(np.float64)
        move = degree > 0
        if pinned is not None:
            move &= np.asarray(pinned) == 0
        p = src[move].astype(np.float64)
        d = total[move] / degree[move].astype(np.float64)[:, None] - p
        d = np.float64(s) * d
        dst = src.copy()
        dst[move] = (p + d).astype(F)
    return dst


def umbrella(src, t):
    src = np.asarray(src, F)
    out = np.zeros(src.shape, F)
    with np.errstate(all="ignore"):
        for v in range(len(src)):
            if t.offsets[v + 1] > t.offsets[v]:
                out[v] = (_mean(src, t, v) - src[v].astype(np.float64)).astype(F)
    return out


def factors(iterations, method, lambda_, mu):
    return [lambda_] * iterations if method == "laplacian" else [lambda_, mu] * iterations


def smooth(rows, t, iterations=10, method="taubin", lambda_=0.5, mu=-0.53, boundary="fixed", one_step=step):
    """`rows` [nv][k] after the steps of a method; the input is not written."""
    why = check_options(method, boundary, iterations, lambda_, mu)
    assert why is None, why
    pinned = (t.vertex_flags & 3) != 0 if boundary == "fixed" else None
    out = np.asarray(rows, F).copy()
    for s in factors(iterations, method, lambda_, mu):
        out = one_step(out, t, s, pinned)
    return out


def pinned_count(t, boundary):
    return int(((t.vertex_flags & 3) != 0).sum()) if boundary == "fixed" else 0


def enclosed_volume(vertices, faces):
    """The signed sum of the tetrahedra (origin, a, b, c), in float64."""
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float((a * np.cross(b, c)).sum() / 6.0)


def roughness(vertices, t):
    """The mean length of the umbrella vectors of the positions, in float64."""
    return float(np.linalg.norm(umbrella(vertices, t).astype(np.float64), axis=1).mean())
