"""csrc/gp_surface.h's definition restated in numpy float64: the distance of a query to every usable face, as a brute force in the
header's operation order, and the lexicographic minimum.  No grid: the definition names none.  numpy never fuses a product into a sum,
so every operation below rounds once, as the library's build without contraction does."""
from types import SimpleNamespace

import numpy as np

F = np.float32
I = np.int32
WIDE_CELLS, MAX_WIDE_CELLS, STAT_WORDS, REFUSED_CAPACITY = 64, 64, 12, 1
EXCLUDED_FACES, EXCLUDED_QUERIES, CANDIDATES, MAX_RING, DIM_X, DIM_Y, DIM_Z, SWEPT, PAIRS, WIDE, STATUS = range(11)


def dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2], x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], axis=-1)


def usable_faces(vertices, faces):
    """The numbers of the usable faces, ascending."""
    vertices, faces = np.asarray(vertices, F).reshape(-1, 3), np.asarray(faces, I).reshape(-1, 3)
    nv = len(vertices)
    ok = ((faces >= 0) & (faces < nv)).all(axis=1)
    if nv:
        ok &= np.isfinite(vertices[np.where(ok[:, None], faces, 0)]).all(axis=(1, 2))
    return np.nonzero(ok)[0]


def edge(q, s, t):
    """(d, p, tau) of the segment candidates: q [n, 1, 3] against s, t [1, m, 3]."""
    e, w = t - s, q - s
    l2 = dot(e, e)
    with np.errstate(invalid="ignore", divide="ignore"):
        x = dot(w, e) / l2
    x = np.where(x < 0.0, 0.0, np.where(x > 1.0, 1.0, x))
    tau = np.where(l2 > 0.0, x, 0.0)
    p = s + e * tau[..., None]
    r = q - p
    return dot(r, r), p, tau


def interior(q, a, b, c):
    """(candidate, d, p, u, v) of the interior candidates."""
    e1, e2, w = b - a, c - a, q - a
    n = cross(e1, e2)
    nn = dot(n, n)
    with np.errstate(invalid="ignore", divide="ignore"):
        u = dot(cross(w, e2), n) / nn
        v = dot(cross(e1, w), n) / nn
        inside = (nn > 0.0) & (u >= 0.0) & (v >= 0.0) & (u + v <= 1.0)
        u, v = np.where(inside, u, 0.0), np.where(inside, v, 0.0)
        p = (a + e1 * u[..., None]) + e2 * v[..., None]
    r = q - p
    return inside, dot(r, r), p, u, v


def face_candidates(q, a, b, c):
    """(d, region, p, u1, u2) of every (query, face): the lexicographic minimum of (d_k, k)."""
    inside, d, p, u1, u2 = interior(q, a, b, c)
    d = np.where(inside, d, np.inf)
    region = np.zeros(d.shape, I)
    one, zero = np.ones(d.shape), np.zeros(d.shape)
    for k, (s, t) in enumerate(((a, b), (b, c), (c, a)), 1):
        dk, pk, tau = edge(q, s, t)
        better = dk < d
        if k == 1:
            better |= ~inside
        bu, bv = ((tau, zero), (one - tau, tau), (zero, one - tau))[k - 1]
        d, region = np.where(better, dk, d), np.where(better, I(k), region)
        p, u1, u2 = np.where(better[..., None], pk, p), np.where(better, bu, u1), np.where(better, bv, u2)
    return d, region, p, u1, u2


def point_mesh(queries, vertices, faces, chunk=32):
    """The definition, by brute force: dist2, face, region, closest, bary and the two counts that are defined without the grid; ties:
    {query: the faces at exactly the winning float64 distance} where they are more than one."""
    queries = np.asarray(queries, F).reshape(-1, 3)
    vertices, faces = np.asarray(vertices, F).reshape(-1, 3), np.asarray(faces, I).reshape(-1, 3)
    nq = len(queries)
    usable = usable_faces(vertices, faces)
    ok = np.isfinite(queries).all(axis=1)
    out = SimpleNamespace(dist2=np.full(nq, np.inf, F), face=np.full(nq, -1, I), region=np.zeros(nq, I), closest=np.full((nq, 3), np.nan, F), bary=np.zeros((nq, 2), F),
                          excluded_faces=len(faces) - len(usable), excluded_queries=int((~ok).sum()), dist2_f64=np.full(nq, np.inf), ties={})
    if not len(usable):
        return out
    corners = vertices[faces[usable]].astype(np.float64)
    a, b, c = corners[None, :, 0], corners[None, :, 1], corners[None, :, 2]
    rows = np.nonzero(ok)[0]
    for s in range(0, len(rows), chunk):
        i = rows[s:s + chunk]
        d, region, p, u1, u2 = face_candidates(queries[i].astype(np.float64)[:, None, :], a, b, c)
        j = np.argmin(d, axis=1)                      # the first minimum: the smallest face number (usable ascends)
        at = np.arange(len(i))
        out.dist2_f64[i] = d[at, j]
        for r in np.nonzero((d == d[at, j][:, None]).sum(axis=1) > 1)[0]:          # the faces at exactly the winning distance, where more than one
            out.ties[int(i[r])] = usable[np.nonzero(d[r] == d[r, j[r]])[0]]
        out.dist2[i], out.face[i], out.region[i] = d[at, j].astype(F), usable[j].astype(I), region[at, j]
        out.closest[i], out.bary[i] = p[at, j].astype(F), np.stack([u1[at, j], u2[at, j]], axis=1).astype(F)
    return out


def interpolate(result, faces, attributes):
    """gp_geometry_interpolate of the result's (face, bary): ((B - A) * u1 + A) + (C - A) * u2 in float32; zeros where face is -1."""
    faces, A = np.asarray(faces, I).reshape(-1, 3), np.asarray(attributes, F)
    ok = result.face >= 0
    f = faces[np.where(ok, result.face, 0)] if len(faces) else np.zeros((len(ok), 3), I)
    u1, u2 = result.bary[:, :1], result.bary[:, 1:]
    a, b, c = A[f[:, 0]], A[f[:, 1]], A[f[:, 2]]
    t1 = (((b - a).astype(F) * u1).astype(F) + a).astype(F)
    t2 = ((c - a).astype(F) * u2).astype(F)
    return np.where(ok[:, None], (t1 + t2).astype(F), F(0))


def auto_cells(usable):
    """round(sqrt(usable) / 4) in the header's integers, clamped to 1 .. 1024."""
    r = 0
    while 16 * (r + 1) ** 2 <= usable:
        r += 1
    if 4 * (2 * r + 1) ** 2 <= usable:
        r += 1
    return max(1, min(r, 1024))
