"""The numpy restatement of csrc/gp_flow.h: the same float32 operations in the same order, one rounding each (fma32 is the one fused
operation, exact).  A view is anything with .vm and .pm ([16] float32, m[col*4 + row]: the camera's world_view_transform and
full_proj_transform as they lie in memory), .W and .H."""
import numpy as np

F = np.float32
TILE, SUMS, COLUMNS, WHEEL = 1024, 7, 8, 55
PI32 = F(3.14159265358979323846)


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 values, correctly rounded: the product is exact in float64, the sum is rounded to odd there (TwoSum
    gives its error), and 53 bits rounded to odd round to 24 as the exact value does."""
    a, b, c = (np.asarray(v, dtype=F).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        t = s - p
        e = (p - (s - t)) + (c - t)
        need = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(need, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F)


def pixel(view, xyz):
    """(pix.x, pix.y, front) of the rows of xyz [N, 3] in `view`."""
    v, p = np.asarray(view.vm, dtype=F), np.asarray(view.pm, dtype=F)
    x, y, z = (np.ascontiguousarray(xyz[:, k], dtype=F) for k in range(3))
    row = lambda m, r: fma32(m[r], x, fma32(m[4 + r], y, fma32(m[8 + r], z, m[12 + r])))          # noqa: E731
    with np.errstate(all="ignore"):
        depth = row(v, 2)
        hx, hy, hw = row(p, 0), row(p, 1), row(p, 3)
        pw = F(1) / (hw + F(0.0000001))
        ndcx, ndcy = hx * pw, hy * pw
        px = ((ndcx + F(1)) * F(view.W) - F(1)) * F(0.5)
        py = ((ndcy + F(1)) * F(view.H) - F(1)) * F(0.5)
        return px, py, depth > F(0.2)


def project(view0, view1, xyz0, xyz1):
    """gp_flow_project: [N, 3] float32."""
    x0, y0, f0 = pixel(view0, xyz0)
    x1, y1, f1 = pixel(view1, xyz1)
    with np.errstate(all="ignore"):
        ok = f0 & f1 & np.isfinite(x0) & np.isfinite(y0) & np.isfinite(x1) & np.isfinite(y1)
        out = np.zeros((len(xyz0), 3), dtype=F)
        out[:, 0] = np.where(ok, x1 - x0, F(0))
        out[:, 1] = np.where(ok, y1 - y0, F(0))
        out[:, 2] = np.where(ok, F(1), F(0))
    return out


def resolve(composite, alpha_min):
    """gp_flow_resolve: (flow [2, H, W] float32, alpha [H, W] float32, valid [H, W] uint8)."""
    c = np.asarray(composite, dtype=F)
    with np.errstate(all="ignore"):
        u, v = c[0] / c[2], c[1] / c[2]
        valid = (c[2] >= F(alpha_min)) & np.isfinite(u) & np.isfinite(v)
    flow = np.stack([np.where(valid, u, F(0)), np.where(valid, v, F(0))]).astype(F)
    return flow, c[2].copy(), valid.astype(np.uint8)


def wheel_bytes():
    """The [55, 3] integers of the Middlebury colour wheel."""
    rows = []
    for length, fn in ((15, lambda r: (255, r, 0)), (6, lambda r: (255 - r, 255, 0)), (4, lambda r: (0, 255, r)), (11, lambda r: (0, 255 - r, 255)),
                       (13, lambda r: (r, 0, 255)), (6, lambda r: (255, 0, 255 - r))):
        rows += [fn(255 * i // length) for i in range(length)]
    return np.array(rows, dtype=np.int64)


def wheel(dtype=F):
    return wheel_bytes().astype(dtype) / dtype(255)


def coloured(flow, valid):
    ok = np.isfinite(flow[0]) & np.isfinite(flow[1])
    return ok if valid is None else ok & (np.asarray(valid) != 0)


def max_magnitude(flow, valid=None):
    """The largest finite float32 magnitude over the coloured pixels, 0 where there is none."""
    flow = np.asarray(flow, dtype=F)
    with np.errstate(all="ignore"):
        m = np.sqrt(flow[0] * flow[0] + flow[1] * flow[1])
        m = m[coloured(flow, valid) & np.isfinite(m)]
    return F(m.max()) if m.size else F(0)


def colorize(flow, valid=None, max_flow=0.0, background=(0, 0, 0), dtype=F):
    """gp_flow_colorize: (out [3, H, W], scale written).  dtype=np.float64 evaluates the same formula in double (for the error bar of
    the float32 one); the scale and the flow stay the float32 values."""
    flow32 = np.asarray(flow, dtype=F)
    found = F(max_flow) if max_flow > 0 else max_magnitude(flow32, valid)
    s = F(max_flow) if max_flow > 0 else (found if found > 0 else F(1))
    T = dtype
    pi = PI32 if dtype is F else np.pi
    wh = wheel(T)
    with np.errstate(all="ignore"):
        u, v = flow32[0].astype(T) / T(s), flow32[1].astype(T) / T(s)
        rad = np.sqrt(u * u + v * v)
        a = np.arctan2(-v, -u) / T(pi)
        fk = ((a + T(1)) / T(2)) * T(54)
        k0f = np.floor(fk)
        k0f = np.where(k0f >= 0, k0f, T(0))
        k0f = np.where(k0f <= 54, k0f, T(54))
        k0 = k0f.astype(np.int64)
        k1 = (k0 + 1) % WHEEL
        f = (fk - k0f).astype(T)
        out = np.empty((3,) + flow32.shape[1:], dtype=T)
        take = coloured(flow32, valid)
        for c in range(3):
            x = (T(1) - f) * wh[k0, c] + f * wh[k1, c]
            x = np.where(rad <= 1, T(1) - rad * (T(1) - x), x * T(0.75))
            out[c] = np.where(take, x, T(F(background[c])))
    return out.astype(T), found


def _tile_sums(terms):
    """terms [SUMS, plane] float32 -> the slots [tiles, SUMS] float64, by the kernel's tree."""
    plane = terms.shape[1]
    tiles = (plane + TILE - 1) // TILE
    t = np.zeros((SUMS, tiles * TILE), dtype=F)
    t[:, :plane] = terms
    t = t.reshape(SUMS, tiles, TILE // 256, 256)
    acc = np.zeros((SUMS, tiles, 256), dtype=F)
    for u in range(TILE // 256):
        acc = acc + t[:, :, u, :]
    acc = acc.reshape(SUMS, tiles, 4, 64)
    lane = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lane ^ d]
    w = acc[..., 0]
    return ((w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])).astype(np.float64).T.copy()


def _finalize(slots):
    """slots [tiles, SUMS] float64 -> a row [COLUMNS] float64."""
    tiles = slots.shape[0]
    pad = np.zeros(((tiles + 255) // 256 * 256, SUMS))
    pad[:tiles] = slots
    a = np.zeros((256, SUMS))
    for k in range(0, len(pad), 256):
        a = a + pad[k:k + 256]
    stride = 128
    while stride >= 1:
        a[:stride] = a[:stride] + a[stride:2 * stride]
        stride //= 2
    s = a[0]
    if not s[0] > 0:
        return np.full(COLUMNS, np.nan)
    return np.concatenate([[s[0]], s[1:] / s[0], [0.0]])


def metrics(flow, gt, mask=None):
    """gp_flow_metrics: [B, 8] float64."""
    flow, gt = np.asarray(flow, dtype=F), np.asarray(gt, dtype=F)
    B = flow.shape[0]
    rows = []
    for b in range(B):
        fu, fv, gu, gv = (a.reshape(-1) for a in (flow[b, 0], flow[b, 1], gt[b, 0], gt[b, 1]))
        with np.errstate(all="ignore"):
            counts = np.isfinite(fu) & np.isfinite(fv) & np.isfinite(gu) & np.isfinite(gv)
            if mask is not None:
                counts &= np.asarray(mask[b]).reshape(-1) != 0
            du, dv = fu - gu, fv - gv
            epe, mag = np.sqrt(du * du + dv * dv), np.sqrt(gu * gu + gv * gv)
            one = lambda c: np.where(counts & c, F(1), F(0))                     # noqa: E731
            terms = np.stack([one(True), np.where(counts, epe, F(0)), one(epe > F(1)), one(epe > F(3)), one(epe > F(5)),
                              one((epe > F(3)) & (epe > F(0.05) * mag)), np.where(counts, mag, F(0))]).astype(F)
        rows.append(_finalize(_tile_sums(terms)))
    return np.stack(rows)


def warp(image, flow):
    """gp_flow_warp: [C, H, W] float32."""
    image, flow = np.asarray(image, dtype=F), np.asarray(flow, dtype=F)
    C, H, W = image.shape
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        sx, sy = xs.astype(F) + flow[0], ys.astype(F) + flow[1]
        x0f, y0f = np.floor(sx), np.floor(sy)
        ok = np.isfinite(sx) & np.isfinite(sy)
        ok &= (x0f >= F(-1)) & (x0f < F(W)) & (y0f >= F(-1)) & (y0f < F(H))
        ax, ay = np.where(ok, sx - x0f, F(0)), np.where(ok, sy - y0f, F(0))
        x0, y0 = np.where(ok, x0f, 0).astype(np.int64), np.where(ok, y0f, 0).astype(np.int64)
        w00, w01, w10, w11 = (F(1) - ay) * (F(1) - ax), (F(1) - ay) * ax, ay * (F(1) - ax), ay * ax

        def tap(plane, y, x):
            inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            return np.where(inside, plane[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], F(0))

        out = np.zeros_like(image)
        for c in range(C):
            p = image[c]
            v = ((w00 * tap(p, y0, x0) + w01 * tap(p, y0, x0 + 1)) + w10 * tap(p, y0 + 1, x0)) + w11 * tap(p, y0 + 1, x0 + 1)
            out[c] = np.where(ok, v, F(0))
    return out
