"""The voxel-grid downsample of include/gp_voxel.h restated in numpy float64, and the clouds the host and the device tests share.

The formulae are Open3D's PointCloud::VoxelDownSample as its published source states them (Open3D itself is not installed where this
was written, so nothing here is pinned against its binary): min_bound = min - voxel_size / 2, index = floor((p - min_bound) /
voxel_size) as int32, per voxel the sum of its rows in ascending input row over float64(count).  np.lexsort gives the order
(ix, iy, iz); np.add.at is unbuffered, so it adds row by row in index order, which is the sequential sum."""
import numpy as np

INT32_MAX = 2 ** 31 - 1


def down_sample(points, voxel_size, colors=None, normals=None):
    """-> (points [M, 3], colors, normals, index int32 [M, 3]); ValueError for the refusals."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    voxel_size = float(voxel_size)
    if not voxel_size > 0.0:
        raise ValueError("voxel_size <= 0")
    attrs = [None if a is None else np.asarray(a, dtype=np.float64).reshape(-1, 3) for a in (colors, normals)]
    if points.shape[0] == 0:
        return (points, attrs[0], attrs[1], np.empty((0, 3), np.int32))
    if not np.isfinite(points).all():
        raise ValueError("a coordinate is not finite")
    min_bound = points.min(axis=0) - voxel_size / 2
    max_bound = points.max(axis=0) + voxel_size / 2
    if voxel_size * INT32_MAX < (max_bound - min_bound).max():
        raise ValueError("voxel_size is too small")
    index = np.floor((points - min_bound) / voxel_size).astype(np.int32)
    assert (index >= 0).all()
    order = np.lexsort((index[:, 2], index[:, 1], index[:, 0]))
    ordered = index[order]
    head = np.ones(len(order), bool)
    head[1:] = (ordered[1:] != ordered[:-1]).any(axis=1)
    seg = np.empty(len(order), np.int64)
    seg[order] = np.cumsum(head) - 1
    m = int(head.sum())
    count = np.bincount(seg, minlength=m).astype(np.float64)[:, None]

    def mean(a):
        if a is None:
            return None
        s = np.zeros((m, 3), np.float64)
        np.add.at(s, seg, a)
        return s / count

    return mean(points), mean(attrs[0]), mean(attrs[1]), ordered[head]


def until(points, colors=None, normals=None, max_points=40000, voxel_size=0.02, step=0.01):
    """The loop of the reference's downsample script on down_sample: ((points, colors, normals), [(voxel_size, count)])."""
    cloud, passes = (np.asarray(points, np.float64), colors, normals), []
    while len(cloud[0]) > max_points:
        cloud = down_sample(cloud[0], voxel_size, cloud[1], cloud[2])[:3]
        passes.append((voxel_size, len(cloud[0])))
        voxel_size += step
    return cloud, passes


# ---- the clouds ----
SIZES = [1, 2, 1023, 1024, 1025, 2049, 5000, 70001, 262145]      # 1024: the sort's block; 2049: past the scan's tile; 262145: past RS_SMALL_N
ATTRS = ["xyz", "xyz+colors", "xyz+colors+normals"]
LOOP_COUNTS = [5690, 4940, 3802, 2852, 1913, 1339, 1053, 860, 706, 560, 451]


def surface(n, seed, attrs="xyz"):
    """n points uniform in [-1, 1]^2 x [-0.05, 0.05], rounded through float32 (what a PLY of floats holds), float64; colours in [0, 1]
    as byte / 255, normals unnormalised."""
    rng = np.random.default_rng(seed)
    pts = (rng.uniform(-1.0, 1.0, (n, 3)) * np.array([1.0, 1.0, 0.05])).astype(np.float32).astype(np.float64)
    col = rng.integers(0, 256, (n, 3)).astype(np.float64) / 255.0 if "colors" in attrs else None
    nrm = rng.normal(size=(n, 3)) if "normals" in attrs else None
    return pts, col, nrm


def size_case(n, attrs):
    """The cloud and the voxel size of one (N, attributes) case: about six points a voxel at the large sizes."""
    return surface(n, 1000 + n, attrs) + (0.05 if n > 5000 else 0.1,)


def loop_cloud():
    """N = 6000, seed 0: with max_points = 500 the loop takes the eleven passes of LOOP_COUNTS."""
    rng = np.random.default_rng(0)
    return (rng.uniform(-1.0, 1.0, (6000, 3)) * np.array([1.0, 1.0, 0.05])).astype(np.float32).astype(np.float64)


def boundary_cloud():
    """voxel_size 0.5 and a minimum of 0 on every axis, so min_bound = -0.25: the coordinates k / 2 + 0.25 sit exactly on voxel
    boundaries (integral quotients).  With duplicated points and points a step to either side of a boundary."""
    rng = np.random.default_rng(7)
    on = rng.integers(0, 9, (400, 3)) * 0.5 + 0.25
    near = on[:100] + rng.choice([-2.0 ** -40, 2.0 ** -40], (100, 3))
    pts = np.concatenate([np.zeros((1, 3)), on, near, on[:50], rng.uniform(0.0, 4.5, (200, 3))])
    return pts[rng.permutation(len(pts))], 0.5


def negative_boundary_cloud():
    """The same on negative coordinates: the minimum is -3, voxel_size 0.25, min_bound = -3.125."""
    rng = np.random.default_rng(8)
    on = -3.0 + rng.integers(0, 20, (500, 3)) * 0.25 + 0.125
    pts = np.concatenate([np.full((1, 3), -3.0), on, on[:80], rng.uniform(-3.0, 2.0, (200, 3))])
    return pts[rng.permutation(len(pts))], 0.25


def one_voxel_cloud():
    """N = 5000 points in one voxel: the long segment."""
    return np.random.default_rng(9).uniform(0.0, 0.009, (5000, 3)), 0.02


def own_voxel_cloud():
    """Every point in a voxel of its own (M = N): a jittered lattice of 17 x 13 x 11 cells, shuffled."""
    rng = np.random.default_rng(10)
    g = np.stack(np.meshgrid(np.arange(17), np.arange(13), np.arange(11), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    pts = g + rng.uniform(0.3, 0.7, g.shape)
    return pts[rng.permutation(len(pts))], 1.0


def wide_axis_cloud(which):
    """Coordinates up to 1000 at voxel 0.01: the largest index passes 65 535 (17 bits an axis).  "x": on one axis only, with y past
    255 -- a key of 17 + 9 + 4 bits, one sort; "xyz": on all three -- 51 bits, two sorts through the running permutation; "far": up to 100 000 on all three (beyond what the issue
    asks) -- 72 bits, three sorts."""
    rng = np.random.default_rng({"x": 11, "xyz": 12, "far": 13}[which])
    n = 3000
    scale = {"x": np.array([1000.0, 3.0, 0.1]), "xyz": np.full(3, 1000.0), "far": np.full(3, 100000.0)}[which]
    base = rng.uniform(0.0, 1.0, (n // 3, 3)) * scale
    pts = np.concatenate([base, base + rng.uniform(0.0, 0.004, base.shape), base + rng.uniform(0.0, 0.004, base.shape), scale[None], np.zeros((1, 3))])
    return pts[rng.permutation(len(pts))], 0.01


def with_attrs(pts, seed):
    rng = np.random.default_rng(seed)
    return pts, rng.uniform(0.0, 1.0, pts.shape), rng.normal(size=pts.shape)


def special_cases():
    """{name: (points, colors, normals, voxel_size)}"""
    out = {}
    for k, (name, (pts, vs)) in enumerate((("boundary", boundary_cloud()), ("negative_boundary", negative_boundary_cloud()), ("one_voxel", one_voxel_cloud()),
                                           ("own_voxel", own_voxel_cloud()), ("wide_x", wide_axis_cloud("x")), ("wide_xyz", wide_axis_cloud("xyz")), ("wide_far", wide_axis_cloud("far")))):
        out[name] = with_attrs(pts, 50 + k) + (vs,)
    return out
