"""The numpy restatement of csrc/gp_tsdf.h: the same float32 operations in the same order, one rounding each (flow_ref.fma32 is the one
fused operation, exact).  A volume is anything with .nx, .ny, .nz, .origin ([3]), .voxel, .trunc and the flat arrays .tsdf, .weight
[nz*ny*nx] and .color ([3, nz*ny*nx] or None); a view anything with .vm ([16] float32: the camera's world_view_transform as it lies in
memory, m[col*4 + row]), .tanfovx and .tanfovy.

The sixteen cases of a tetrahedron are DERIVED here from the rule the header states (case_triangles), not copied from the header's
table: the tests hold the two against each other, and both against the facts of closed surfaces."""
import itertools
from types import SimpleNamespace

import numpy as np

from flow_ref import fma32

F = np.float32
TILE, MAX_VIEWS = 1024, 16
EDGE_BITS = (1, 2, 4, 3, 5, 6, 7)                 # the direction of edge e as corner bits (x = 1, y = 2, z = 4)
EDGE_OF_BITS = {b: e for e, b in enumerate(EDGE_BITS)}
LOCAL_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def _even(p):
    return sum(1 for a in range(len(p)) for b in range(a + 1, len(p)) if p[a] > p[b]) % 2 == 0


def tetrahedra():
    """[(corner bits of v0..v3, odd)]: the monotone paths 000 -> e_a -> e_a + e_b -> 111, the axis orders in lexicographic order;
    det[v1 - v0, v2 - v0, v3 - v0] is the sign of the permutation."""
    return [((0, 1 << a, (1 << a) | (1 << b), 7), not _even((a, b, c))) for a, b, c in itertools.permutations(range(3))]


def case_triangles(mask):
    """The triangles of a POSITIVELY oriented tetrahedron whose vertex q is inside iff bit q of mask: each a triple of local edges
    (pairs of vertices, smaller first).  One inside vertex i, the others j, k, l with (i, j, k, l) an even permutation:
    (ij, ik, il).  One outside vertex i: (ij, il, ik).  Two inside i < j, two outside k, l with (i, j, k, l) even: (ik, il, jl) and
    (ik, jl, jk) -- the quadrilateral ik, il, jl, jk cut along ik-jl."""
    inside = [q for q in range(4) if mask >> q & 1]
    outside = [q for q in range(4) if not mask >> q & 1]
    E = lambda a, b: (min(a, b), max(a, b))       # noqa: E731
    if len(inside) in (1, 3):
        i = (inside if len(inside) == 1 else outside)[0]
        j, k, l = [q for q in range(4) if q != i]
        if not _even((i, j, k, l)):
            k, l = l, k
        return [(E(i, j), E(i, k), E(i, l))] if len(inside) == 1 else [(E(i, j), E(i, l), E(i, k))]
    if len(inside) == 2:
        (i, j), (k, l) = inside, outside
        if not _even((i, j, k, l)):
            k, l = l, k
        return [(E(i, k), E(i, l), E(j, l)), (E(i, k), E(j, l), E(j, k))]
    return []


def case_table():
    """[16][6] local edge numbers (-1: none), as the header's table is laid out."""
    rows = []
    for mask in range(16):
        flat = [LOCAL_EDGES.index(e) for tri in case_triangles(mask) for e in tri]
        rows.append(flat + [-1] * (6 - len(flat)))
    return rows


def volume(nx, ny, nz, origin, voxel, trunc, tsdf=None, weight=None, color=None, has_color=True):
    n = nx * ny * nz
    return SimpleNamespace(nx=nx, ny=ny, nz=nz, origin=tuple(float(F(o)) for o in origin), voxel=float(F(voxel)), trunc=float(F(trunc)),
                           tsdf=np.zeros(n, F) if tsdf is None else np.asarray(tsdf, F).reshape(n).copy(),
                           weight=np.zeros(n, F) if weight is None else np.asarray(weight, F).reshape(n).copy(),
                           color=(np.zeros((3, n), F) if color is None else np.asarray(color, F).reshape(3, n).copy()) if has_color else None)


def coords(vol):
    """(x, y, z) float32 [n] of every grid point, n = (k*ny + j)*nx + i."""
    k, j, i = np.meshgrid(np.arange(vol.nz), np.arange(vol.ny), np.arange(vol.nx), indexing="ij")
    return tuple(fma32(a.reshape(-1).astype(F), F(vol.voxel), F(o)) for a, o in zip((i, j, k), vol.origin))


def integrate(vol, depth, valid, image, views, z_min=1e-3, view_weight=1.0, weight_max=64.0):
    """gp_tsdf_integrate: (tsdf, weight, color) after the views, in their order; vol is left as it is."""
    depth = np.asarray(depth, dtype=F)
    V, H, W = depth.shape
    assert 1 <= V <= MAX_VIEWS and len(views) == V and (image is None) == (vol.color is None)
    x, y, z = coords(vol)
    t, w = vol.tsdf.copy(), vol.weight.copy()
    c = None if vol.color is None else vol.color.copy()
    trunc, z_min, vw, wmax = F(vol.trunc), F(z_min), F(view_weight), F(weight_max)
    with np.errstate(all="ignore"):
        for v, view in enumerate(views):
            m = np.asarray(view.vm, dtype=F)
            P = [fma32(m[r], x, fma32(m[4 + r], y, fma32(m[8 + r], z, m[12 + r]))) for r in range(3)]
            ok = P[2] > z_min
            pix = []
            for Pa, tan, size in ((P[0], view.tanfovx, W), (P[1], view.tanfovy, H)):
                an = Pa / (P[2] * F(tan))
                pa = ((an + F(1)) * F(size) - F(1)) * F(0.5)
                fa = np.floor(pa + F(0.5))
                ok = ok & np.isfinite(fa) & (fa >= F(0)) & (fa < F(size))
                pix.append(fa)
            ix, iy = (np.where(ok, fa, F(0)).astype(np.int64) for fa in pix)
            d = depth[v, iy, ix]
            if valid is not None:
                ok = ok & (np.asarray(valid)[v, iy, ix] != 0)
            ok = ok & np.isfinite(d) & (d > 0)
            s = d - P[2]
            ok = ok & ~(s < -trunc)
            tt = np.minimum(F(1), s / trunc)
            wn = w + vw
            t = np.where(ok, (t * w + tt * vw) / wn, t)
            if c is not None:
                img = np.asarray(image, dtype=F)[v][:, iy, ix]
                c = np.where(ok[None], (c * w[None] + img * vw) / wn[None], c)
            w = np.where(ok, np.minimum(wn, wmax), w)
    return t.astype(F), w.astype(F), None if c is None else c.astype(F)


def _shift(a, bits, fill):
    """a[k + dz, j + dy, i + dx] for the corner `bits`, `fill` where that leaves the grid."""
    dx, dy, dz = bits & 1, bits >> 1 & 1, bits >> 2 & 1
    out = np.full_like(a, fill)
    nz, ny, nx = a.shape
    out[:nz - dz, :ny - dy, :nx - dx] = a[dz:, dy:, dx:]
    return out


def classify(vol, iso, min_weight):
    """(usable, inside, active) [nz, ny, nx] bool; active at a cell's corner 000."""
    shape = (vol.nz, vol.ny, vol.nx)
    t, w = vol.tsdf.reshape(shape), vol.weight.reshape(shape)
    with np.errstate(all="ignore"):
        usable = (w >= F(min_weight)) & np.isfinite(t)
        inside = t < F(iso)
    active = np.ones(shape, bool)
    for bits in range(8):
        active &= _shift(usable, bits, False)
    return usable, inside, active


def marks(vol, iso, min_weight):
    """[n, 7] bool: edge 7 n + e crosses."""
    _, inside, active = classify(vol, iso, min_weight)
    nz, ny, nx = inside.shape
    ap = np.zeros((nz + 1, ny + 1, nx + 1), bool)
    ap[1:, 1:, 1:] = active
    out = np.zeros((nz, ny, nx, 7), bool)
    for e, bits in enumerate(EDGE_BITS):
        exists = _shift(np.ones_like(inside), bits, False)
        differ = inside != _shift(inside, bits, False)
        cell = np.zeros_like(inside)
        for s in range(8):
            if s & bits:
                continue                          # the cells of an edge: its owner's, stepped back along the axes it does not run along
            sx, sy, sz = s & 1, s >> 1 & 1, s >> 2 & 1
            cell |= ap[1 - sz:1 - sz + nz, 1 - sy:1 - sy + ny, 1 - sx:1 - sx + nx]
        out[..., e] = exists & differ & cell
    return out.reshape(-1, 7)


def extract(vol, iso=0.0, min_weight=1.0):
    """gp_tsdf_extract_count and _fill: (counts [2] int32, vertices [Nv, 3] float32, colors [Nv, 3] float32 or None, faces [Nf, 3] int32)."""
    nx, ny, nz = vol.nx, vol.ny, vol.nz
    n_points = nx * ny * nz
    mk = marks(vol, iso, min_weight)
    ids = np.flatnonzero(mk.reshape(-1))
    rank = np.cumsum(mk.reshape(-1)) - 1                   # the vertex of a crossing edge
    n, e = ids // 7, ids % 7
    bits = np.array(EDGE_BITS)[e]
    n1 = n + (bits & 1) + (bits >> 1 & 1) * nx + (bits >> 2 & 1) * nx * ny
    xyz = coords(vol)
    isof = F(iso)
    with np.errstate(all="ignore"):
        a = (isof - vol.tsdf[n]) / (vol.tsdf[n1] - vol.tsdf[n])
        vertices = np.stack([fma32(a, p[n1] - p[n], p[n]) for p in xyz], axis=1).astype(F).reshape(-1, 3)
        colors = None if vol.color is None else np.stack([fma32(a, ch[n1] - ch[n], ch[n]) for ch in vol.color], axis=1).astype(F).reshape(-1, 3)
    _, inside, active = classify(vol, iso, min_weight)
    corner = [_shift(inside, b, False).reshape(-1) for b in range(8)]
    active = active.reshape(-1)
    faces = np.full((n_points, 6, 2, 3), -1, np.int64)
    point = np.arange(n_points)
    for q, (cb, odd) in enumerate(tetrahedra()):
        mask = sum(corner[cb[v]].astype(np.int64) << v for v in range(4))
        for case in range(1, 15):
            sel = active & (mask == case)
            if not sel.any():
                continue
            for s, tri in enumerate(case_triangles(case)):
                tri = (tri[0], tri[2], tri[1]) if odd else tri
                for r, (va, vb) in enumerate(tri):
                    lo, hi = cb[va], cb[vb]
                    owner = point[sel] + (lo & 1) + (lo >> 1 & 1) * nx + (lo >> 2 & 1) * nx * ny
                    eid = 7 * owner + EDGE_OF_BITS[hi ^ lo]
                    assert mk.reshape(-1)[eid].all()         # an active cell's sign change is a crossing edge
                    faces[sel, q, s, r] = rank[eid]
    faces = faces.reshape(-1, 3)
    faces = faces[faces[:, 0] >= 0].astype(np.int32)
    return np.array([len(ids), len(faces)], np.int32), vertices, colors, faces


# ---- the facts of a closed surface ----
def mesh_facts(vertices, faces):
    """{"V", "E", "F", "euler", "edge_uses" (the set of how many triangles an undirected edge lies in), "directed_max", "unreferenced",
    "volume"} of a triangle mesh, in float64 and integers."""
    f = np.asarray(faces, dtype=np.int64)
    v = np.asarray(vertices, dtype=np.float64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    _, directed = np.unique(d, axis=0, return_counts=True)
    _, undirected = np.unique(np.sort(d, axis=1), axis=0, return_counts=True)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return dict(V=len(v), E=len(undirected), F=len(f), euler=len(v) - len(undirected) + len(f), edge_uses=set(undirected.tolist()),
                directed_max=int(directed.max()) if len(directed) else 0, unreferenced=len(v) - len(np.unique(f)),
                volume=float((a * np.cross(b, c)).sum() / 6.0))
