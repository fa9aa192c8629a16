"""csrc/gp_sdf.h's definitions restated in numpy float64, in the header's operation order: the face normals, face_edges, the ordered
sums of the edge and vertex pseudonormals (the j-th entry of every run at once: each run's own sum still goes in ascending entry),
the volume's tree, and the sign of a query from (dist2, face, region).  numpy never fuses a product into a sum.  And one thing that
is NOT the definition: winding_number, the Van Oosterom-Strackee solid angles, the independent arbiter of inside and outside."""
from types import SimpleNamespace

import numpy as np

import surface_ref
from surface_ref import cross, dot

F = np.float32
I = np.int32
BLOCK = 256
COUNT_NAMES = ("status", "skipped", "zero_area", "missing")
STAT_NAMES = ("face", "edge", "vertex", "inside", "outside", "undetermined", "excluded", "status")
FACE, EDGE, VERTEX, INSIDE, OUTSIDE, UNDETERMINED, EXCLUDED, STATUS = range(8)
COUNT_WORDS, STAT_WORDS, MEAN_WORDS = 4, 8, 4
UNSTABLE = 2.0 ** -30          # a row with |g| <= UNSTABLE * |r| * |N| is not a sign row


def _ordered_sum(keys, terms, rows):
    """sums [rows, 3] and sums of |term| of terms [m, 3] by key, each key's terms added in their order from +0.0."""
    order = np.argsort(keys, kind="stable")
    k, t = keys[order], terms[order]
    start = np.searchsorted(k, np.arange(rows))
    count = np.searchsorted(k, np.arange(rows), side="right") - start
    total, size = np.zeros((rows, 3)), np.zeros((rows, 3))
    with np.errstate(all="ignore"):
        for j in range(int(count.max()) if rows and len(k) else 0):
            r = np.nonzero(count > j)[0]
            total[r] = total[r] + t[start[r] + j]
            size[r] = size[r] + np.abs(t[start[r] + j])
    return total, size


def tree(x):
    """The partial of every block of 256 terms: x[i] = x[i] + x[i + d] for d = 128 .. 1."""
    x = np.asarray(x, np.float64)
    blocks = (len(x) + BLOCK - 1) // BLOCK
    x = np.concatenate([x, np.zeros(blocks * BLOCK - len(x))]).reshape(blocks, BLOCK)
    d = BLOCK // 2
    with np.errstate(all="ignore"):
        while d >= 1:
            x = x[:, :d] + x[:, d:2 * d]
            d //= 2
    return x[:, 0]


def total(partials):
    s = np.float64(0.0)
    with np.errstate(all="ignore"):
        for p in partials:
            s = s + p
    return s


def face_normals(vertices, faces):
    """(contributes [nf], bad [nf], corners [nf, 3, 3] float64, u [nf, 3], made [nf]: nn > 0)."""
    vertices, faces = np.asarray(vertices, F).reshape(-1, 3), np.asarray(faces, I).reshape(-1, 3)
    nv = len(vertices)
    bad = ~((faces >= 0) & (faces < nv)).all(axis=1)
    contributes = ~bad & (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 2] != faces[:, 0])
    p = vertices[np.where(bad[:, None], 0, faces)].astype(np.float64) if nv else np.zeros((len(faces), 3, 3))
    with np.errstate(all="ignore"):
        n = cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        nn = dot(n, n)
        made = contributes & (nn > 0.0)
        u = np.where(made[:, None], n / np.sqrt(nn)[:, None], 0.0)
    return contributes, bad, p, u, made


def tables(vertices, faces, edge):
    """SimpleNamespace(face_edges, edge_normal, vertex_normal, volume, counts; edge_size, vertex_size: the sums of |term| per component,
    what the float64 tables' bar is measured in)."""
    vertices, faces = np.asarray(vertices, F).reshape(-1, 3), np.asarray(faces, I).reshape(-1, 3)
    edge = np.asarray(edge, np.int64).reshape(-1, 2)
    nv, nf, ne = len(vertices), len(faces), len(edge)
    contributes, bad, p, u, made = face_normals(vertices, faces)
    base = max(nv, 1)
    packed = edge[:, 0] * base + edge[:, 1]
    face_edges = np.full((nf, 3), -1, I)
    missing = 0
    f64 = faces.astype(np.int64)
    for k in range(3):
        s, t = f64[:, k], f64[:, (k + 1) % 3]
        want = ~bad & (s != t)
        key = np.minimum(s, t) * base + np.maximum(s, t)
        at = np.searchsorted(packed, key)
        found = want & (at < ne)
        found[found] = packed[at[found]] == key[found]
        face_edges[found, k] = at[found]
        missing += int((want & ~found).sum())
    with np.errstate(all="ignore"):
        angle = np.zeros((nf, 3))
        for k in range(3):
            e1, e2 = p[:, (k + 1) % 3] - p[:, k], p[:, (k + 2) % 3] - p[:, k]
            x = cross(e1, e2)
            angle[:, k] = np.arctan2(np.sqrt(dot(x, x)), dot(e1, e2))
        entry_face = np.repeat(np.arange(nf), 3)                  # entry 3f + k, ascending
        entry_made = np.repeat(made, 3)
        corner_ok = entry_made
        vertex_normal, vertex_size = _ordered_sum(f64.reshape(-1)[corner_ok], (angle.reshape(-1)[:, None] * u[entry_face])[corner_ok], nv)
        side_ok = entry_made & (face_edges.reshape(-1) >= 0)
        edge_normal, edge_size = _ordered_sum(face_edges.reshape(-1)[side_ok].astype(np.int64), u[entry_face][side_ok], ne)
        term = np.where(contributes, dot(p[:, 0], cross(p[:, 1], p[:, 2])) / 6.0, 0.0)
        volume = total(tree(term)) if nf else np.float64(0.0)
    counts = np.array([int(bad.any()), int((~contributes).sum()), int((contributes & ~made).sum()), missing], I)
    return SimpleNamespace(face_edges=face_edges, edge_normal=edge_normal, vertex_normal=vertex_normal, volume=np.float64(volume), counts=counts, edge_size=edge_size,
                           vertex_size=vertex_size)


def sign(queries, dist2, face, region, vertices, faces, t):
    """SimpleNamespace(sdf, sign, kind, element, stats; g, unstable) of the header's steps (1) to (5) on gp_surface_grid_query's own
    (dist2, face, region).  unstable: the rows with |g| <= 2^-30 |r| |N|, where only |sdf| is compared."""
    queries, dist2 = np.asarray(queries, F).reshape(-1, 3), np.asarray(dist2, F)
    vertices, faces = np.asarray(vertices, F).reshape(-1, 3), np.asarray(faces, I).reshape(-1, 3)
    face, region = np.asarray(face, np.int64), np.asarray(region, np.int64)
    nq, nv, nf, ne = len(queries), len(vertices), len(faces), len(t.edge_normal)
    excluded = face == -1
    with np.errstate(all="ignore"):
        sdf = np.where(excluded, F(np.inf), np.sqrt(dist2.astype(np.float64)).astype(F)).astype(F)
    sg, kind, element = np.zeros(nq, np.int8), np.full(nq, -1, I), np.full(nq, -1, I)
    g, unstable = np.zeros(nq), np.zeros(nq, bool)
    foreign = ~excluded & ((face < 0) | (face >= nf) | (region < 0) | (region > 3))
    fi = faces[np.where(excluded | foreign, 0, face)].astype(np.int64) if nf else np.zeros((nq, 3), np.int64)
    foreign |= ~excluded & ~((fi >= 0) & (fi < nv)).all(axis=1)
    live = ~excluded & ~foreign
    c = vertices[np.where(live[:, None], fi, 0)].astype(np.float64) if nv else np.zeros((nq, 3, 3))
    q = queries.astype(np.float64)
    p, N = np.zeros((nq, 3)), np.zeros((nq, 3))
    with np.errstate(all="ignore"):
        inside, _, p0, _, _ = surface_ref.interior(q, c[:, 0], c[:, 1], c[:, 2])
        n = cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
        nn = dot(n, n)
        u = np.where((nn > 0.0)[:, None], n / np.sqrt(nn)[:, None], 0.0)
        rows = live & (region == 0)
        foreign |= rows & ~inside
        rows &= inside
        p[rows], N[rows], kind[rows], element[rows] = p0[rows], u[rows], 0, face[rows]
        for k in (1, 2, 3):
            s, e = k - 1, k % 3
            _, pk, tau = surface_ref.edge(q, c[:, s], c[:, e])
            d = c[:, e] - c[:, s]
            l2 = dot(d, d)
            rows = live & (region == k)
            at_s = rows & (~(l2 > 0.0) | (tau == 0.0) | (fi[:, s] == fi[:, e]))
            at_t = rows & ~at_s & (tau == 1.0)
            on = rows & ~at_s & ~at_t
            number = t.face_edges[np.where(on, face, 0), s].astype(np.int64) if nf else np.zeros(nq, np.int64)
            wrong = on & ((number < -1) | (number >= ne))
            foreign |= wrong
            on &= ~wrong
            p[rows] = pk[rows]
            kind[at_s | at_t], kind[on] = 2, 1
            element[at_s], element[at_t], element[on] = fi[at_s, s], fi[at_t, e], number[on]
            N[at_s], N[at_t] = t.vertex_normal[fi[at_s, s]], t.vertex_normal[fi[at_t, e]]
            have = on & (number >= 0)
            N[have] = t.edge_normal[number[have]]
        live &= ~foreign
        kind[foreign], element[foreign] = -1, -1
        r = q - p
        g = np.where(live, dot(r, N), 0.0)
        sg = np.where(g < 0.0, -1, np.where(g > 0.0, 1, 0)).astype(np.int8)
        sdf = np.where(sg < 0, -sdf, sdf).astype(F)
        bound = UNSTABLE * np.sqrt(dot(r, r)) * np.sqrt(dot(N, N))
        unstable = live & (bound > 0.0) & (np.abs(g) <= bound)          # (a bound of 0: r or N is exactly zero and so is g, in any arithmetic -- a sign row)
    stats = np.array([int((live & (kind == k)).sum()) for k in range(3)] + [int((sg < 0).sum()), int((sg > 0).sum()), int((foreign | (live & (sg == 0))).sum()),
                     int(excluded.sum()), int(foreign.any())], np.int64)
    return SimpleNamespace(sdf=sdf, sign=sg, kind=kind, element=element, stats=stats, g=g, unstable=unstable)


def face_normal_sign(queries, closest, face, vertices, faces):
    """What the winning face's own normal says: sign(dot(q - closest, n_f)) -- wrong at sharp folds, which is why the tables exist."""
    queries, closest = np.asarray(queries, np.float64), np.asarray(closest, np.float64)
    _, _, _, u, _ = face_normals(vertices, faces)
    return np.sign(dot(queries - closest, u[np.asarray(face, np.int64)])).astype(np.int8)


def means(sdf, sg):
    """gp_sdf_means: count, sum, outside, inside of the finite rows, through the tree."""
    sdf, sg = np.asarray(sdf, F), np.asarray(sg, np.int8)
    ok = np.isfinite(sdf)
    words = [ok.astype(np.float64), np.where(ok, sdf.astype(np.float64), 0.0), (ok & (sg > 0)).astype(np.float64), (ok & (sg < 0)).astype(np.float64)]
    return np.array([total(tree(w)) if len(w) else 0.0 for w in words], np.float64)


def winding_number(q, v, f):
    """The winding number of the mesh around every query: the solid angles of Van Oosterom and Strackee, summed, over 4 pi.  float64."""
    q, v, f = np.asarray(q, np.float64).reshape(-1, 3), np.asarray(v, np.float64).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)
    out = np.zeros(len(q))
    for s in range(0, len(q), 64):
        a, b, c = (v[f[:, k]][None, :, :] - q[s:s + 64, None, :] for k in range(3))
        la, lb, lc = (np.linalg.norm(x, axis=2) for x in (a, b, c))
        det = (a * np.cross(b, c)).sum(axis=2)
        den = la * lb * lc + (a * b).sum(axis=2) * lc + (b * c).sum(axis=2) * la + (c * a).sum(axis=2) * lb
        out[s:s + 64] = (2.0 * np.arctan2(det, den)).sum(axis=1) / (4.0 * np.pi)
    return out
