"""The numpy restatement of csrc/gp_mesh_render.h: the same float32 operations in the same order, one rounding each (flow_ref.fma32 is
the one fused operation, exact), coverage in int64.  A view is anything with .vm ([16] float32: the camera's world_view_transform as
it lies in memory, m[col*4 + row]), .tanfovx and .tanfovy (tsdf_cases.look_at makes one); W and H travel beside it.

Nothing here walks triangles in an order: the candidates of all faces are one flat list, the visibility buffer is numpy's unordered
minimum over it."""
from types import SimpleNamespace

import numpy as np

import depth_ref
from flow_ref import fma32

F = np.float32
I64 = np.int64
NARROW_MAX, SPLIT, MAX_SIZE, MAX_CHANNELS, SUBPIXEL, GUARD = 64, 16, 16384, 8, 256, 2 ** 23
STATUS, DRAWN, NEAR, OUT_OF_RANGE, DEGENERATE, CULLED, WIDE, COUNT_WORDS = 0, 1, 2, 3, 4, 5, 6, 8
CULL = {"none": 0, "back": 1, "front": 2}
EMPTY = np.uint64(2 ** 64 - 1)


def camera_points(view, vertices):
    """(P_x, P_y, P_z) float32 [nv]."""
    m = np.asarray(view.vm, dtype=F)
    v = np.asarray(vertices, dtype=F).reshape(-1, 3)
    x, y, z = (np.ascontiguousarray(v[:, k]) for k in range(3))
    return tuple(fma32(m[r], x, fma32(m[4 + r], y, fma32(m[8 + r], z, m[12 + r]))) for r in range(3))


def _snap(p):
    s = np.floor(fma32(p, F(SUBPIXEL), F(0.5)))
    ok = np.isfinite(s) & (np.abs(s) <= F(GUARD))
    return np.where(ok, s, 0).astype(I64), ok


def records(vertices, view, W, H, z_near=0.01):
    """The vertex records: X, Y int64 [nv], r float32 [nv], near and out_of_range bool [nv]."""
    Px, Py, Pz = camera_points(view, vertices)
    with np.errstate(all="ignore"):
        near = ~(Pz > F(z_near))
        xn, yn = Px / (Pz * F(view.tanfovx)), Py / (Pz * F(view.tanfovy))
        px, py = ((xn + F(1)) * F(W) - F(1)) * F(0.5), ((yn + F(1)) * F(H) - F(1)) * F(0.5)
        (X, okx), (Y, oky) = _snap(px), _snap(py)
        return SimpleNamespace(X=X, Y=Y, r=F(1) / Pz, near=near, out_of_range=~(okx & oky))


def _edge(ux, uy, vx, vy, px, py):
    return (vx - ux) * (py - uy) - (vy - uy) * (px - ux)


def rasterize(vertices, faces, view, W, H, z_near=0.01, cull="none"):
    """gp_mesh_render_rasterize and gp_mesh_render_resolve: a namespace with counts [8] int32, coverage [H, W] int32, face [H, W] int32,
    depth [H, W] float32, valid [H, W] uint8, bary [3, H, W] float32, and rec, the vertex records."""
    vertices, faces = np.asarray(vertices, dtype=F).reshape(-1, 3), np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    nv, nf, plane = len(vertices), len(faces), H * W
    rec = records(vertices, view, W, H, z_near)
    counts = np.zeros(COUNT_WORDS, np.int32)
    vis, coverage = np.full(plane, EMPTY, np.uint64), np.zeros(plane, np.int32)
    out = SimpleNamespace(counts=counts, rec=rec, face=np.full(plane, -1, np.int32), depth=np.zeros(plane, F), valid=np.zeros(plane, np.uint8), bary=np.zeros((3, plane), F))
    f = faces.astype(I64)
    bad = ((f < 0) | (f >= nv)).any(axis=1) if nf else np.zeros(0, bool)
    counts[STATUS] = bad.sum()
    ids = np.nonzero(~bad)[0]
    f = f[ids]
    near = rec.near[f].any(axis=1)
    counts[NEAR] = near.sum()
    ids, f = ids[~near], f[~near]
    far = rec.out_of_range[f].any(axis=1)
    counts[OUT_OF_RANGE] = far.sum()
    ids, f = ids[~far], f[~far]
    X, Y, r = rec.X[f], rec.Y[f], rec.r[f]                    # [n, 3]
    area2 = _edge(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2])
    flat = area2 == 0
    counts[DEGENERATE] = flat.sum()
    culled = ~flat & ((area2 > 0) if CULL[cull] == 1 else (area2 < 0) if CULL[cull] == 2 else np.zeros(len(f), bool))
    counts[CULLED] = culled.sum()
    keep = ~flat & ~culled
    ids, X, Y, r, area2 = ids[keep], X[keep], Y[keep], r[keep], area2[keep]
    counts[DRAWN] = len(ids)
    sign, area = np.sign(area2), np.abs(area2)
    x0, x1 = np.maximum(-((-X.min(axis=1)) // SUBPIXEL), 0), np.minimum(X.max(axis=1) // SUBPIXEL, W - 1)
    y0, y1 = np.maximum(-((-Y.min(axis=1)) // SUBPIXEL), 0), np.minimum(Y.max(axis=1) // SUBPIXEL, H - 1)
    bw, bh = np.maximum(x1 - x0 + 1, 0), np.maximum(y1 - y0 + 1, 0)
    pixels = bw * bh
    counts[WIDE] = (pixels > NARROW_MAX).sum()
    # every candidate (face, pixel), flat
    t = np.repeat(np.arange(len(ids)), pixels)
    k = np.arange(pixels.sum()) - np.repeat(np.cumsum(pixels) - pixels, pixels)
    ix, iy = x0[t] + k % np.maximum(bw[t], 1), y0[t] + k // np.maximum(bw[t], 1)
    px, py = ix * SUBPIXEL, iy * SUBPIXEL
    inside = np.ones(len(t), bool)
    w = []
    for i in range(3):
        u, v = (i + 1) % 3, (i + 2) % 3
        wi = sign[t] * _edge(X[t, u], Y[t, u], X[t, v], Y[t, v], px, py)
        dx, dy = sign[t] * (X[t, v] - X[t, u]), sign[t] * (Y[t, v] - Y[t, u])
        owns = (dy > 0) | ((dy == 0) & (dx > 0))
        inside &= (wi > 0) | ((wi == 0) & owns)
        w.append(wi)
    with np.errstate(all="ignore"):
        l = [(wi.astype(np.float64) / area[t].astype(np.float64)).astype(F) for wi in w]
        q = fma32(l[0], r[t, 0], fma32(l[1], r[t, 1], l[2] * r[t, 2]))
        z = F(1) / q
        counting = inside & np.isfinite(z) & (z > 0)
    t, ix, iy, z, l = t[counting], ix[counting], iy[counting], z[counting], [li[counting] for li in l]
    pix = iy * W + ix
    key = (np.ascontiguousarray(z).view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids[t].astype(np.uint64)
    np.minimum.at(vis, pix, key)
    np.add.at(coverage, pix, 1)
    won = key == vis[pix]                                     # (a face meets a pixel once: one candidate per key)
    out.face[pix[won]] = ids[t[won]]
    out.depth[pix[won]] = z[won]
    out.valid[pix[won]] = 1
    for i in range(3):
        out.bary[i, pix[won]] = l[i][won]
    out.coverage = coverage.reshape(H, W)
    out.face, out.depth, out.valid, out.bary = out.face.reshape(H, W), out.depth.reshape(H, W), out.valid.reshape(H, W), out.bary.reshape(3, H, W)
    return out


def _winners(res, faces):
    ys, xs = np.nonzero(res.valid)
    return ys, xs, np.asarray(faces, dtype=I64).reshape(-1, 3)[res.face[ys, xs]]


def interpolate(res, faces, attributes, background):
    """gp_mesh_render_interpolate: [C, H, W] float32."""
    a = np.asarray(attributes, dtype=F)
    C = a.shape[1]
    H, W = res.valid.shape
    out = np.empty((C, H, W), F)
    out[:] = np.asarray(background, dtype=F).reshape(C, 1, 1)
    ys, xs, v = _winners(res, faces)
    l = [res.bary[i, ys, xs] for i in range(3)]
    r = [res.rec.r[v[:, i]] for i in range(3)]
    with np.errstate(all="ignore"):
        t = [l[i] * r[i] for i in range(3)]
        q = fma32(l[0], r[0], fma32(l[1], r[1], l[2] * r[2]))
        for c in range(C):
            out[c, ys, xs] = fma32(t[0], a[v[:, 0], c], fma32(t[1], a[v[:, 1], c], t[2] * a[v[:, 2], c])) / q
    return out


def _pixel_view(view, W, H):
    return SimpleNamespace(W=W, H=H, tanfovx=view.tanfovx, tanfovy=view.tanfovy)


def normals(res, vertices, faces, view):
    """gp_mesh_render_normals: (normals [3, H, W] float32, nvalid [H, W] uint8)."""
    H, W = res.valid.shape
    n, nvalid = np.zeros((3, H, W), F), np.zeros((H, W), np.uint8)
    ys, xs, v = _winners(res, faces)
    P = np.stack(camera_points(view, vertices), axis=1)       # [nv, 3]
    with np.errstate(all="ignore"):
        A, B, Cc = P[v[:, 0]], P[v[:, 1]], P[v[:, 2]]
        e1, e2 = B - A, Cc - A
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        length = np.sqrt((nx * nx + ny * ny) + nz * nz)
        ok = np.isfinite(length) & (length > 0)
        nx, ny, nz = nx / length, ny / length, nz / length
        Qx, Qy, Qz = depth_ref.point(_pixel_view(view, W, H), xs, ys, res.depth[ys, xs])
        away = (nx * Qx + ny * Qy) + nz * Qz > 0
    for c, comp in enumerate((nx, ny, nz)):
        n[c, ys[ok], xs[ok]] = np.where(away, -comp, comp)[ok]
    nvalid[ys[ok], xs[ok]] = 1
    return n, nvalid


def shade(color, n, nvalid, depth, view, ambient=0.3, background=(0, 0, 0)):
    """gp_mesh_render_shade: [3, H, W] float32."""
    H, W = nvalid.shape
    out = np.empty((3, H, W), F)
    out[:] = np.asarray(background, dtype=F).reshape(3, 1, 1)
    ys, xs = np.nonzero(nvalid)
    with np.errstate(all="ignore"):
        Qx, Qy, Qz = depth_ref.point(_pixel_view(view, W, H), xs, ys, depth[ys, xs])
        nx, ny, nz = (n[c, ys, xs] for c in range(3))
        s = np.abs((nx * Qx + ny * Qy) + nz * Qz) / np.sqrt((Qx * Qx + Qy * Qy) + Qz * Qz)
        L = fma32(F(1) - F(ambient), s, F(ambient))
        for c in range(3):
            out[c, ys, xs] = np.asarray(color, dtype=F)[c, ys, xs] * L
    return out
