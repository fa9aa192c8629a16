"""Seeded cases of TSDF fusion and mesh extraction, shared by the host test (the stand-alone build of csrc/tsdf_core.h) and the GPU test
(tsdf_ops).  The shapes are the smallest at which each program can still go wrong:

  volumes   2x2x2, one cell; 5x4x3; 1x6x6, which has no cells (counts 0, 0); 13x11x7 = 1001 points, so 7007 edges cross six tile
            boundaries of 1024 while the points and the 720 cells stay inside one tile; 19x13x9 = 2223 points and 1728 cells, three tiles
            of points with a ragged last one; 33^3 for the closed surfaces (36 tiles)
  states    random samples (a triangle in almost every tetrahedron); nothing seen (weight 0); all inside; all outside; a block of unusable
            points in the middle (weight below min_weight, NaN and infinite samples): inactive cells, and edges whose ends differ in
            sign but lie in no active cell; samples exactly equal to a non-zero iso
  images    16x12 and 40x30
  integrate V = 1, 3 and 16 in one call, 17 as 16 + 1; a camera inside the volume (points behind it), a plane of points exactly at
            z_min; projections outside every border and exactly on a pixel boundary; invalid pixels; NaN, infinite, zero and negative
            depths; s exactly -trunc and one ulp to either side; the weight cap reached mid-batch; a volume without colour; a volume that
            is not empty at the start

EXTRACT: name -> (volume of tsdf_ref, iso, min_weight); INTEGRATE: name -> a namespace with vol, views, depth, valid, image, z_min,
view_weight, weight_max.  `extracted` and `integrated` hold tsdf_ref's answers, computed once."""
import functools
import math
from types import SimpleNamespace

import numpy as np

import tsdf_ref as ref

F = np.float32
NAN, INF = float("nan"), float("inf")


# ---- views ----
def look_at(eye, target, tanfovx, tanfovy, up=(0.0, -1.0, 0.0)):
    """A view of tsdf_ref: the camera at `eye` looking at `target`, +x right, +y down, +z forward; .vm as a camera stores it."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(-np.asarray(up, np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])                       # world -> camera
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, -R @ eye
    return SimpleNamespace(vm=m.T.astype(F).reshape(16).copy(), tanfovx=tanfovx, tanfovy=tanfovy)       # flat[col*4 + row]


def plain_view(tz, tanfovx, tanfovy):
    """The camera at (0, 0, -tz) looking along +z without a rotation: P = (x, y, z + tz), exactly where the sum is."""
    m = np.eye(4)
    m[2, 3] = tz
    return SimpleNamespace(vm=m.T.astype(F).reshape(16).copy(), tanfovx=tanfovx, tanfovy=tanfovy)


def ring(V, centre, radius, tan, seed):
    rng = np.random.default_rng(seed)
    out = []
    for v in range(V):
        a, h = 2 * math.pi * v / V + rng.uniform(-0.1, 0.1), rng.uniform(-0.6, 0.6)
        eye = np.asarray(centre) + radius * np.array([math.cos(a), h, math.sin(a)])
        out.append(look_at(eye, np.asarray(centre) + rng.uniform(-0.05, 0.05, 3), tan, tan * 0.75))
    return out


# ---- extraction ----
def _random_volume(nx, ny, nz, seed, has_color=True):
    rng = np.random.default_rng(seed)
    n = nx * ny * nz
    return ref.volume(nx, ny, nz, rng.uniform(-1, 1, 3), 0.1 + 0.05 * rng.uniform(), 0.4, tsdf=rng.uniform(-1, 1, n), weight=rng.uniform(1, 5, n),
                      color=rng.uniform(0, 1, (3, n)), has_color=has_color)


def sdf_volume(n, f, origin=(-1.6, -1.6, -1.6), voxel=0.1):
    """n^3 points of the function f(x, y, z) (float64 in, rounded once), every point seen once, coloured by its position."""
    v = ref.volume(n, n, n, origin, voxel, 4 * voxel)
    x, y, z = (a.astype(np.float64) for a in ref.coords(v))
    v.tsdf = f(x, y, z).astype(F)
    v.weight[:] = 1
    v.color = np.stack([(a - a.min()) / (a.max() - a.min()) for a in (x, y, z)]).astype(F)
    return v


SPHERE = SimpleNamespace(c=(0.013, -0.021, 0.007), r=1.03)
ELLIPSOID = SimpleNamespace(c=(0.31, -0.17, 0.23), s=(1.0, 0.7, 0.85), r=0.9)
TORUS = SimpleNamespace(c=(0.013, -0.021, 0.007), R=0.9, r=0.37)


def sphere_sdf(x, y, z, s=SPHERE):
    return np.sqrt((x - s.c[0]) ** 2 + (y - s.c[1]) ** 2 + (z - s.c[2]) ** 2) - s.r


def ellipsoid_sdf(x, y, z, s=ELLIPSOID):
    """Ellipsoid-like: the sphere's distance in stretched coordinates (not a true distance: only the topology is tested on it)."""
    return np.sqrt(((x - s.c[0]) / s.s[0]) ** 2 + ((y - s.c[1]) / s.s[1]) ** 2 + ((z - s.c[2]) / s.s[2]) ** 2) - s.r


def torus_sdf(x, y, z, s=TORUS):
    return np.sqrt((np.sqrt((x - s.c[0]) ** 2 + (y - s.c[1]) ** 2) - s.R) ** 2 + (z - s.c[2]) ** 2) - s.r


def _extract_cases():
    cases = {}
    for name, dims, seed in (("2x2x2_random", (2, 2, 2), 400), ("5x4x3_random", (5, 4, 3), 401), ("1x6x6_random", (1, 6, 6), 402),
                             ("13x11x7_random", (13, 11, 7), 403), ("19x13x9_random", (19, 13, 9), 404)):
        cases[name] = (_random_volume(*dims, seed), 0.0, 1.0)
    cases["5x4x3_plain"] = (_random_volume(5, 4, 3, 405, has_color=False), 0.0, 1.0)
    v = _random_volume(13, 11, 7, 406)
    v.weight[:] = 0
    cases["13x11x7_empty"] = (v, 0.0, 1.0)
    v = _random_volume(13, 11, 7, 407)
    v.tsdf = -np.abs(v.tsdf) - F(0.01)
    cases["13x11x7_inside"] = (v, 0.0, 1.0)
    v = _random_volume(13, 11, 7, 408)
    v.tsdf = np.abs(v.tsdf)
    cases["13x11x7_outside"] = (v, 0.0, 1.0)
    v = _random_volume(19, 13, 9, 409)                # a block of unusable points in the middle: low weights, and samples that are not finite
    w, t = v.weight.reshape(9, 13, 19), v.tsdf.reshape(9, 13, 19)
    w[3:6, 4:9, 6:13] = 0.5
    t[2, 3, 4], t[6, 9, 14], t[7, 2, 16] = NAN, INF, -INF
    cases["19x13x9_hole"] = (v, 0.0, 1.0)
    v = _random_volume(5, 4, 3, 410)                  # samples exactly on a non-zero iso, between inside and outside neighbours
    v.tsdf[::7] = F(0.25)
    cases["5x4x3_equal_iso"] = (v, 0.25, 2.0)         # (min_weight 2: about a quarter of the points are unusable)
    v = _random_volume(13, 11, 7, 411)
    v.tsdf[::5] = F(-0.125)
    cases["13x11x7_equal_iso"] = (v, -0.125, 0.0)
    cases["33_sphere"] = (sdf_volume(33, sphere_sdf), 0.0, 1.0)
    cases["33_ellipsoid"] = (sdf_volume(33, ellipsoid_sdf), 0.0, 1.0)
    cases["33_torus"] = (sdf_volume(33, torus_sdf), 0.0, 1.0)
    cases["13x11x7_open_sphere"] = (sdf_volume(13, lambda x, y, z: sphere_sdf(x, y, z), origin=(-0.2, -0.3, 0.1), voxel=0.11), 0.0, 1.0)
    return cases


EXTRACT = _extract_cases()


@functools.lru_cache(maxsize=None)
def extracted(name):
    """tsdf_ref.extract of a case: (counts, vertices, colors, faces); do not modify."""
    vol, iso, min_weight = EXTRACT[name]
    return ref.extract(vol, iso, min_weight)


# ---- integrate ----
def _images(V, H, W, seed, special=True):
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth = np.stack([2.0 + 0.25 * np.sin(xs / 3.0 + v) + 0.2 * np.cos(ys / 2.0 - v) + rng.normal(0, 0.01, (H, W)) for v in range(V)]).astype(F)
    valid = (rng.uniform(size=(V, H, W)) > 0.2).astype(np.uint8)
    valid[valid != 0] = rng.integers(1, 256, int((valid != 0).sum()))         # any byte but 0 counts
    if special:
        for v in range(V):
            depth[v, 1 + v % (H - 2), 1:7] = [NAN, INF, -INF, 0.0, -2.0, -0.0]
            valid[v, 1 + v % (H - 2), 1:7] = 1
    return depth, valid, rng.uniform(0, 1, (V, 3, H, W)).astype(F)


def _round_case(V, H, W, seed, has_color=True, masked=True, weight_max=64.0, view_weight=1.0, start=False, inside=False):
    vol = _random_volume(13, 11, 7, seed, has_color) if start else None
    if vol is None:
        vol = ref.volume(13, 11, 7, (-0.6, -0.5, -0.3), 0.1, 0.25, has_color=has_color)
    else:
        vol.origin, vol.voxel, vol.trunc = (-0.6, -0.5, -0.3), float(F(0.1)), 0.25
    views = ring(V, (0.0, 0.0, 0.0), 2.0, 0.3, seed)
    if inside:
        views[1] = look_at((0.05, 0.0, 0.02), (1.0, 0.2, 0.1), 0.3, 0.225)      # inside the volume: most points are behind it or too near
    depth, valid, image = _images(V, H, W, seed + 1)
    return SimpleNamespace(vol=vol, views=views, depth=depth, valid=valid if masked else None, image=image if has_color else None, z_min=1e-3,
                           view_weight=view_weight, weight_max=weight_max)


def _aligned_case():
    """Every coordinate exact: voxel 1/8, the origin a multiple of it, the camera at the world's origin without a rotation, tangents 1/2, a
    16 x 12 image.  P = (x, y, z); (px + 0.5) = (x / (z / 2) + 1) * 8 is integral for many points; z_min is the depth of the plane k = 1;
    trunc = 1/4 and the depth map holds z - 1/4 of the plane k = 4 and its two neighbours in float32, column by column."""
    vol = ref.volume(13, 11, 7, (-0.75, -0.625, 0.5), 0.125, 0.25)
    depth, valid, image = _images(1, 12, 16, 420, special=False)
    edge = F(1.0 - 0.25)                          # the plane k = 4 is at z = 1: s = -trunc exactly
    depth[0, 3:9, 0::3], depth[0, 3:9, 1::3], depth[0, 3:9, 2::3] = edge, np.nextafter(edge, F(0)), np.nextafter(edge, F(2))     # (rows 3 .. 8: |y| < z / 4)
    depth[0, 2, 3:9] = [NAN, INF, -INF, 0.0, -2.0, -0.0]
    valid[0, 3:, :] = 1
    return SimpleNamespace(vol=vol, views=[plain_view(0.0, 0.5, 0.5)], depth=depth, valid=valid, image=image, z_min=0.625, view_weight=1.0, weight_max=64.0)


def _integrate_cases():
    return {"aligned_16x12_v1": _aligned_case(),
            "round_40x30_v3": _round_case(3, 30, 40, 430),
            "round_16x12_v16_cap": _round_case(16, 12, 16, 432, weight_max=2.5, inside=True),
            "round_40x30_v17": _round_case(17, 30, 40, 434, inside=True),
            "plain_16x12_v3": _round_case(3, 12, 16, 436, has_color=False, masked=False),
            "started_40x30_v3": _round_case(3, 30, 40, 438, view_weight=0.5, weight_max=4.0, start=True)}


INTEGRATE = _integrate_cases()


def integrate_in_groups(fn, c):
    """fn(vol, depth, valid, image, views) -> (tsdf, weight, color) applied to the case's views in groups of 16, as tsdf_ops batches them."""
    vol = SimpleNamespace(**vars(c.vol))
    out = None
    for a in range(0, len(c.views), ref.MAX_VIEWS):
        b = min(len(c.views), a + ref.MAX_VIEWS)
        out = fn(vol, c.depth[a:b], None if c.valid is None else c.valid[a:b], None if c.image is None else c.image[a:b], c.views[a:b])
        vol.tsdf, vol.weight, vol.color = out
    return out


@functools.lru_cache(maxsize=None)
def integrated(name):
    """tsdf_ref.integrate of a case: (tsdf, weight, color); do not modify."""
    c = INTEGRATE[name]
    return integrate_in_groups(lambda vol, d, m, im, vs: ref.integrate(vol, d, m, im, vs, c.z_min, c.view_weight, c.weight_max), c)
