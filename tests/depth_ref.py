"""The numpy restatement of csrc/gp_depth.h: the same float32 operations in the same order, one rounding each (flow_ref.fma32 is the one
fused operation, exact).  A view is anything with .c2w ([16] float32, m[col*4 + row]: the inverse of the camera's world_view_transform
as it lies in memory), .tanfovx, .tanfovy, .W and .H."""
import numpy as np

from flow_ref import fma32

F = np.float32
TILE, SUMS, COLUMNS, LUT = 1024, 12, 12, 256


def resolve(accum, alpha, alpha_min):
    """gp_depth_resolve: (depth [H, W] float32, valid [H, W] uint8)."""
    accum, alpha = np.asarray(accum, dtype=F), np.asarray(alpha, dtype=F)
    with np.errstate(all="ignore"):
        d = accum / alpha
        valid = (alpha >= F(alpha_min)) & np.isfinite(d) & (d > 0)
    return np.where(valid, d, F(0)).astype(F), valid.astype(np.uint8)


def value(depth, valid, mode):
    """(v, coloured): the quantity mode colours (0: depth, 1: disparity) and the pixels that take a colour."""
    depth = np.asarray(depth, dtype=F)
    with np.errstate(all="ignore"):
        v = (F(1) / depth if mode == 1 else depth).astype(F)
        take = np.isfinite(v) & (v > 0)
    if valid is not None:
        take &= np.asarray(valid) != 0
    return v, take


def value_range(depth, valid, mode, lo=0.0, hi=0.0):
    """The pair gp_depth_colorize uses: the given one where lo < hi, else the smallest and largest coloured value, (0, 1) where none."""
    if F(lo) < F(hi):
        return F(lo), F(hi)
    v, take = value(depth, valid, mode)
    return (F(v[take].min()), F(v[take].max())) if take.any() else (F(0), F(1))


def lut_rows(depth, valid, mode, lo, hi):
    """The table row of every pixel (-1: the background) for the pair (lo, hi) used."""
    v, take = value(depth, valid, mode)
    lo, hi = F(lo), F(hi)
    with np.errstate(all="ignore"):
        t = np.zeros_like(v) if hi == lo else ((v - lo) / (hi - lo)).astype(F)
        inside = (t >= 0) & (t < 1)
        row = np.where(inside, (np.where(inside, t, F(0)) * F(256)).astype(np.int64), np.where(t >= 1, 255, 0))
    return np.where(take, row, -1)


def colorize(depth, valid, mode, lo, hi, lut, background):
    """gp_depth_colorize: (out [3, H, W] float32, range [2] float32, rows)."""
    pair = value_range(depth, valid, mode, lo, hi)
    rows = lut_rows(depth, valid, mode, *pair)
    lut = np.asarray(lut, dtype=F)
    out = np.where(rows[None] >= 0, lut[np.maximum(rows, 0)].transpose(2, 0, 1), np.asarray(background, dtype=F)[:, None, None]).astype(F)
    return out, np.array(pair, dtype=F), rows


def point(view, xs, ys, z):
    """The camera-space points of pixels (xs, ys) at depths z."""
    with np.errstate(all="ignore"):
        xn = (2 * np.asarray(xs, dtype=np.int64) + 1).astype(F) / F(view.W) - F(1)
        yn = (2 * np.asarray(ys, dtype=np.int64) + 1).astype(F) / F(view.H) - F(1)
        z = np.asarray(z, dtype=F)
        return xn * F(view.tanfovx) * z, yn * F(view.tanfovy) * z, z


def normals(depth, valid, view):
    """gp_depth_normals: (normals [3, H, W] float32, nvalid [H, W] uint8)."""
    depth = np.asarray(depth, dtype=F)
    H, W = depth.shape
    ok = np.ones((H, W), bool) if valid is None else np.asarray(valid) != 0
    pad = np.zeros((H + 2, W + 2), bool)
    pad[1:-1, 1:-1] = ok
    five = pad[1:-1, 1:-1] & pad[1:-1, :-2] & pad[1:-1, 2:] & pad[:-2, 1:-1] & pad[2:, 1:-1]
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    zp = np.zeros((H + 2, W + 2), dtype=F)
    zp[1:-1, 1:-1] = depth
    with np.errstate(all="ignore"):
        P = point(view, xs, ys, depth)
        r, l = point(view, xs + 1, ys, zp[1:-1, 2:]), point(view, xs - 1, ys, zp[1:-1, :-2])
        d, u = point(view, xs, ys + 1, zp[2:, 1:-1]), point(view, xs, ys - 1, zp[:-2, 1:-1])
        ax, ay, az = r[0] - l[0], r[1] - l[1], r[2] - l[2]
        bx, by, bz = d[0] - u[0], d[1] - u[1], d[2] - u[2]
        nx, ny, nz = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
        length = np.sqrt((nx * nx + ny * ny) + nz * nz)
        nvalid = five & np.isfinite(length) & (length > 0)
        nx, ny, nz = nx / length, ny / length, nz / length
        away = (nx * P[0] + ny * P[1]) + nz * P[2] > 0
        n = np.stack([np.where(away, -nx, nx), np.where(away, -ny, ny), np.where(away, -nz, nz)])
    return np.where(nvalid[None], n, F(0)).astype(F), nvalid.astype(np.uint8)


def normals_image(n, nvalid, background):
    n = np.asarray(n, dtype=F)
    return np.where(np.asarray(nvalid)[None] != 0, n * F(0.5) + F(0.5), np.asarray(background, dtype=F)[:, None, None]).astype(F)


def unproject(depth, valid, image, view):
    """gp_depth_unproject: (points [K, 3] float32, colors [K, 3] float32 or None, index [K] int32, count)."""
    depth = np.asarray(depth, dtype=F)
    H, W = depth.shape
    take = np.ones(H * W, bool) if valid is None else np.asarray(valid).reshape(-1) != 0
    index = np.flatnonzero(take).astype(np.int32)
    ys, xs = index // W, index % W
    m = np.asarray(view.c2w, dtype=F)
    with np.errstate(all="ignore"):
        px, py, pz = point(view, xs, ys, depth.reshape(-1)[index])
        rows = [fma32(m[r], px, fma32(m[4 + r], py, fma32(m[8 + r], pz, m[12 + r]))) for r in range(3)]
    points = np.stack(rows, axis=1).astype(F).reshape(-1, 3)
    colors = None if image is None else np.asarray(image, dtype=F).reshape(3, -1)[:, index].T.copy()
    return points, colors, index, len(index)


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


def _total(slots):
    """slots [tiles, SUMS] float64 -> their sums [SUMS], in the finalising workgroup's order."""
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
    return a[0]


def row_of(s):
    """The twelve sums -> a row [COLUMNS] float64."""
    if not s[0] > 0:
        return np.full(COLUMNS, np.nan)
    n = s[0]
    with np.errstate(all="ignore"):
        ml2, ml = s[4] / n, s[5] / n
        return np.array([n, s[1] / n, s[2] / n, np.sqrt(s[3] / n), np.sqrt(ml2), s[6] / n, s[7] / n, s[8] / n, ml2 - ml * ml, s[9] / s[10], s[11] / n, 0.0])


def metric_terms(pred, gt, mask, scale, gt_min, gt_max, dtype=F):
    """The twelve terms of every pixel of one image, [SUMS, plane] in `dtype`, zeros where the pixel does not count.  dtype=np.float64
    evaluates the same formulas in double from the same float32 d and g (for the error bar of the float32 ones)."""
    pred, g = np.asarray(pred, dtype=F).reshape(-1), np.asarray(gt, dtype=F).reshape(-1)
    with np.errstate(all="ignore"):
        d = pred if scale is None else (pred * F(scale)).astype(F)
        counts = np.isfinite(d) & np.isfinite(g) & (d > 0) & (g > 0) & (F(gt_min) <= g) & (g <= F(gt_max))
        if mask is not None:
            counts &= np.asarray(mask).reshape(-1) != 0
        T = dtype
        dd, gg = np.where(counts, d, F(1)).astype(T), np.where(counts, g, F(1)).astype(T)
        e = dd - gg
        # the header's logf: the float64 logarithm rounded once to float32 (numpy's own float32 log is a vector routine of several ulp)
        log = lambda a: np.log(a.astype(np.float64)).astype(T)               # noqa: E731
        l = log(dd) - log(gg)
        r = np.maximum(dd / gg, gg / dd)
        one = lambda c: np.where(c, T(1), T(0))                              # noqa: E731
        terms = np.stack([one(True) * np.ones_like(dd), np.abs(e) / gg, e * e / gg, e * e, l * l, l, one(r < T(1.25)), one(r < T(1.5625)),
                          one(r < T(1.953125)), dd * gg, dd * dd, gg]).astype(T)
    return np.where(counts[None], terms, T(0))


def metrics(pred, gt, mask=None, scale=None, gt_min=0.0, gt_max=np.inf):
    """gp_depth_metrics: [B, 12] float64."""
    pred, gt = np.asarray(pred, dtype=F), np.asarray(gt, dtype=F)
    rows = []
    for b in range(pred.shape[0]):
        terms = metric_terms(pred[b], gt[b], None if mask is None else mask[b], None if scale is None else scale[b], gt_min, gt_max)
        rows.append(row_of(_total(_tile_sums(terms))))
    return np.stack(rows)


def metrics64(pred, gt, mask=None, scale=None, gt_min=0.0, gt_max=np.inf):
    """The same rows with every term and every sum in float64 (from the same float32 d and g): what the float32 sums approximate."""
    pred, gt = np.asarray(pred, dtype=F), np.asarray(gt, dtype=F)
    rows = []
    for b in range(pred.shape[0]):
        terms = metric_terms(pred[b], gt[b], None if mask is None else mask[b], None if scale is None else scale[b], gt_min, gt_max, dtype=np.float64)
        rows.append(row_of(terms.sum(axis=1)))
    return np.stack(rows)
