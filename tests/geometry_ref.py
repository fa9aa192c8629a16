"""csrc/gp_geometry.h restated in numpy: the sampling integers and points, the nearest neighbour as a brute force (the definition
names no grid), the metric terms, the reduction tree and the table.  Everything here follows the header's words, not the kernels."""
from types import SimpleNamespace

import numpy as np

F = np.float32
I = np.int32
U = np.uint64
MAX_FACES, MAX_CHANNELS, MAX_AXIS, MAX_CELLS, MAX_THRESHOLDS, WEIGHT_BITS = 2 ** 26, 8, 1024, 2 ** 24, 8, 36
STATUS, BAD_INDEX, NON_FINITE, ZERO_WEIGHT, COUNT_WORDS = 0, 1, 2, 3, 8
REFUSED_EMPTY, REFUSED_TOO_MANY = 1, 2
EXCLUDED_POINTS, EXCLUDED_QUERIES, CANDIDATES, MAX_RING, DIM_X, DIM_Y, DIM_Z, SWEPT, STAT_WORDS = 0, 1, 2, 3, 4, 5, 6, 7, 8
COLUMNS, ACCURACY, COMPLETENESS, CHAMFER_L1, CHAMFER_L2, HAUSDORFF, PRECISION, RECALL, FSCORE = 37, 8, 9, 10, 11, 12, 13, 21, 29
TILE, BLOCK, TERMS = 1024, 256, 12


def mix(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def hash3(seed, i, k):
    """h(seed, i, k) for an array of i."""
    with np.errstate(over="ignore"):
        return mix(U(seed) + U(0x9E3779B97F4A7C15) * (U(3) * i.astype(U) + U(k + 1)))


def face_areas(vertices, faces):
    """(A [nf] float64, class [nf]: 0 ok, 1 bad index, 2 non-finite)."""
    vertices, faces = np.asarray(vertices, F).reshape(-1, 3), np.asarray(faces, I).reshape(-1, 3)
    nv = len(vertices)
    bad = ((faces < 0) | (faces >= nv)).any(axis=1)
    safe = np.where(bad[:, None], 0, faces) if nv else np.zeros_like(faces)
    corners = vertices[safe].astype(np.float64) if nv else np.zeros((len(faces), 3, 3))
    nonfinite = ~bad & ~np.isfinite(corners).all(axis=(1, 2))
    a, b, c = corners[:, 0], corners[:, 1], corners[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        e, g = b - a, c - a
        n = np.stack([e[:, 1] * g[:, 2] - e[:, 2] * g[:, 1], e[:, 2] * g[:, 0] - e[:, 0] * g[:, 2], e[:, 0] * g[:, 1] - e[:, 1] * g[:, 0]], axis=1)
        area = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    kind = np.where(bad, 1, np.where(nonfinite, 2, 0))
    return np.where(kind == 0, area, 0.0), kind


def face_weights(vertices, faces):
    """(w [nf] uint64, counts [8] int32 without STATUS)."""
    area, kind = face_areas(vertices, faces)
    counts = np.zeros(COUNT_WORDS, I)
    counts[BAD_INDEX], counts[NON_FINITE] = (kind == 1).sum(), (kind == 2).sum()
    m = area.max() if len(area) else 0.0
    if m == 0:
        w = np.zeros(len(area), U)
    else:
        exponent = np.frexp(m)[1] - 1                                  # m = 1.xxx * 2^exponent
        w = np.ldexp(area, WEIGHT_BITS - exponent).astype(U)           # (an exact product; the conversion truncates)
    counts[ZERO_WEIGHT] = ((kind == 0) & (w == 0)).sum()
    return w, counts


def mix3(a, b, c, u1, u2):
    t1 = (b - a).astype(F)
    t1 = (t1 * u1).astype(F)
    t1 = (t1 + a).astype(F)
    t2 = (c - a).astype(F)
    t2 = (t2 * u2).astype(F)
    return (t1 + t2).astype(F)


def sample_surface(vertices, faces, n, seed=0, attributes=None):
    """counts [8] int32, points [n, 3], face [n], bary [n, 2] (and interpolated [n, C]) as the header defines them."""
    vertices, faces = np.asarray(vertices, F).reshape(-1, 3), np.asarray(faces, I).reshape(-1, 3)
    w, counts = face_weights(vertices, faces)
    prefix = np.cumsum(w, dtype=U)
    T = int(prefix[-1]) if len(prefix) else 0
    counts[STATUS] = REFUSED_EMPTY if T == 0 else (REFUSED_TOO_MANY if T < n else 0)
    out = SimpleNamespace(counts=counts, weights=w, total=T)
    if counts[STATUS]:
        out.points, out.face, out.bary = np.full((n, 3), np.nan, F), np.full(n, -1, I), np.zeros((n, 2), F)
        out.interpolated = None if attributes is None else np.zeros((n, attributes.shape[1]), F)
        return out
    q = T // n
    i = np.arange(n, dtype=U)
    t = i * U(q) + hash3(seed, i, 0) % U(q)
    face = np.searchsorted(prefix, t, side="right").astype(I)          # the first f with P_f > t
    k1, k2 = (hash3(seed, i, 1) >> U(40)).astype(np.int64), (hash3(seed, i, 2) >> U(40)).astype(np.int64)
    flip = k1 + k2 > 2 ** 24
    k1, k2 = np.where(flip, 2 ** 24 - k1, k1), np.where(flip, 2 ** 24 - k2, k2)
    u1, u2 = (k1.astype(F) * F(2.0 ** -24)).astype(F), (k2.astype(F) * F(2.0 ** -24)).astype(F)
    a, b, c = (vertices[faces[face, k]] for k in range(3))
    out.q = q
    out.points, out.face, out.bary = mix3(a, b, c, u1[:, None], u2[:, None]), face, np.stack([u1, u2], axis=1)
    out.interpolated = None
    if attributes is not None:
        A = np.asarray(attributes, F)
        out.interpolated = mix3(A[faces[face, 0]], A[faces[face, 1]], A[faces[face, 2]], u1[:, None], u2[:, None])
    return out


def nearest(queries, points, chunk=256):
    """(dist2 [nq] float32, index [nq] int32, excluded points, excluded queries): the definition, by brute force."""
    queries, points = np.asarray(queries, F).reshape(-1, 3), np.asarray(points, F).reshape(-1, 3)
    usable = np.nonzero(np.isfinite(points).all(axis=1))[0]
    ok = np.isfinite(queries).all(axis=1)
    dist2, index = np.full(len(queries), np.inf, F), np.full(len(queries), -1, I)
    p = points[usable]
    if len(p):
        with np.errstate(over="ignore", invalid="ignore"):
            for s in range(0, len(queries), chunk):
                q = queries[s:s + chunk]
                d = [(q[:, None, a] - p[None, :, a]).astype(F) for a in range(3)]
                d2 = (((d[0] * d[0]).astype(F) + (d[1] * d[1]).astype(F)).astype(F) + (d[2] * d[2]).astype(F)).astype(F)
                j = np.argmin(np.where(np.isnan(d2), np.inf, d2), axis=1)          # the first minimum: the smallest index (usable ascends)
                dist2[s:s + chunk], index[s:s + chunk] = d2[np.arange(len(q)), j], usable[j]
        dist2[~ok], index[~ok] = np.inf, -1
    return dist2, index, len(points) - len(usable), int((~ok).sum())


def auto_cells(usable):
    """round(1.5 * cbrt(usable)) in the header's integers."""
    r = 1
    while 8 * (r + 1) ** 3 <= 27 * usable:
        r += 1
    if (2 * r + 1) ** 3 <= 27 * usable:
        r += 1
    return min(r, MAX_AXIS)


def terms(d2, thresholds):
    """[n, 12] float64."""
    d2 = np.asarray(d2, F)
    counts = np.isfinite(d2)
    with np.errstate(invalid="ignore"):
        dist = np.where(counts, np.sqrt(np.where(counts, d2, 0).astype(np.float64)), 0.0)
    t = np.zeros((len(d2), TERMS))
    t[:, 0], t[:, 1], t[:, 2], t[:, 3] = counts, dist, np.where(counts, d2.astype(np.float64), 0.0), dist
    for k, tau in enumerate(thresholds):
        t[:, 4 + k] = counts & (dist <= np.float64(F(tau)))
    return t


def reduce_direction(d2, thresholds):
    """The twelve totals of one direction through the header's tree."""
    t = terms(d2, thresholds)
    tiles = (len(t) + TILE - 1) // TILE
    padded = np.zeros((tiles * TILE, TERMS))
    padded[:len(t)] = t
    x = padded.reshape(tiles, TILE // BLOCK, BLOCK, TERMS)
    lane = x[:, 0]
    for u in range(1, TILE // BLOCK):
        lane = lane + x[:, u]
    wave = lane.reshape(tiles, BLOCK // 64, 64, TERMS)
    ids = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        wave = wave + wave[:, :, ids ^ s]
    slots = (wave[:, 0, 0] + wave[:, 1, 0]) + (wave[:, 2, 0] + wave[:, 3, 0]) if tiles else np.zeros((0, TERMS))
    rounds = (tiles + BLOCK - 1) // BLOCK
    padded = np.zeros((rounds * BLOCK, TERMS))
    padded[:tiles] = slots
    s = np.zeros((BLOCK, TERMS))
    for r in range(rounds):
        s = s + padded[r * BLOCK:(r + 1) * BLOCK]
    stride = BLOCK // 2
    while stride >= 1:
        s[:stride] = s[:stride] + s[stride:2 * stride]
        stride //= 2
    total = s[0].copy()
    total[3] = t[:, 3].max() if len(t) else 0.0          # a maximum, whatever the order
    return total


def metrics(d2_ab, d2_ba, thresholds):
    """[37] float64: the table."""
    ab, ba = reduce_direction(d2_ab, thresholds), reduce_direction(d2_ba, thresholds)
    nt = len(thresholds)
    row = np.zeros(COLUMNS)
    row[0:4], row[4:8] = ab[:4], ba[:4]
    with np.errstate(invalid="ignore", divide="ignore"):
        acc, com = ab[1] / ab[0], ba[1] / ba[0]
        row[ACCURACY], row[COMPLETENESS], row[CHAMFER_L1] = acc, com, (acc + com) / 2.0
        row[CHAMFER_L2] = ab[2] / ab[0] + ba[2] / ba[0]
        row[HAUSDORFF] = max(ab[3], ba[3]) if ab[0] > 0 and ba[0] > 0 else np.nan
        for k in range(nt):
            p, r = ab[4 + k] / ab[0], ba[4 + k] / ba[0]
            row[PRECISION + k], row[RECALL + k] = p, r
            row[FSCORE + k] = 2.0 * p * r / (p + r) if p + r > 0 else 0.0
    return row
