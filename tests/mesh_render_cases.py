"""Seeded cases of the triangle rasterizer, shared by the host test (the stand-alone build of csrc/mesh_render_core.h) and the GPU test
(mesh_render).  Small on purpose; each names what it can break:

  wide            a triangle larger than the 64 x 48 image, corners off-screen inside the guard band: the wide path, the clamped box
  diagonal        two triangles sharing a diagonal, corners exactly on pixel centres: every inside pixel once, the boundary by ownership
  fan             seven triangles around a hub that is exactly a pixel centre: the hub pixel once
  slivers         triangles that pass between the sample points (no coverage); one that snaps to area2 == 0, one collinear
  ties            two identical faces and two coplanar overlapping ones: the smaller id wins
  near            a corner at P_z <= z_near, a face wholly behind the camera, one ordinary face
  guard           a corner beyond 2^23 sub-pixels
  threshold       faces whose clamped box holds exactly NARROW_MAX and NARROW_MAX + 1 pixels
  bad_index       face indices -1 and nv: STATUS, and the rest is still drawn
  no_faces, nothing, no_vertices        nf = 0; nv = nf = 0; nv = 0 with a face
  random          300 random triangles of mixed sizes at 70 x 50, under all three cull modes
  sphere_*, ellipsoid_*, torus_*        tsdf_cases' closed surfaces from three cameras at 64 x 48, 96 x 64 and 33 x 17

A case: vertices, faces, attributes [nv, 4], view, W, H, z_near, culls.  `result` holds mesh_render_ref's answer, computed once."""
import functools
from types import SimpleNamespace

import numpy as np

import mesh_render_ref as ref
import tsdf_cases

F = np.float32
I = np.int32
BACKGROUND = (0.125, 0.25, 0.5, 0.75)
SHADE_BACKGROUND = (0.25, 0.5, 1.0)
AMBIENT = 0.3
CAMERAS = (((4.0, 0.5, 1.0), 64, 48), ((-2.0, 3.0, -2.5), 96, 64), ((0.3, -0.4, -4.2), 33, 17))        # eye, W, H
SURFACES = {"sphere": ("33_sphere", tsdf_cases.SPHERE.c), "ellipsoid": ("33_ellipsoid", tsdf_cases.ELLIPSOID.c), "torus": ("33_torus", tsdf_cases.TORUS.c)}
TAN = 0.45


def identity_view(tanfovx, tanfovy):
    return SimpleNamespace(vm=np.eye(4, dtype=F).reshape(16).copy(), tanfovx=tanfovx, tanfovy=tanfovy)


def _case(corners, faces, W=64, H=48, z_near=0.01, culls=("none",), seed=0):
    """corners: (pixel x, pixel y, z) under the identity view with tangents 0.5 and 0.375: the camera-space vertex that projects there
    (up to a rounding far below a sub-pixel step, which the snap takes away)."""
    view = identity_view(0.5, 0.375)
    c = np.asarray(corners, np.float64).reshape(-1, 3)
    x = ((2 * c[:, 0] + 1) / W - 1) * view.tanfovx * c[:, 2]
    y = ((2 * c[:, 1] + 1) / H - 1) * view.tanfovy * c[:, 2]
    vertices = np.stack([x, y, c[:, 2]], axis=1).astype(F)
    return _finish(vertices, faces, view, W, H, z_near, culls, seed)


def _finish(vertices, faces, view, W, H, z_near=0.01, culls=("none",), seed=0):
    vertices = np.ascontiguousarray(vertices, dtype=F).reshape(-1, 3)
    attributes = np.random.default_rng(1000 + seed).uniform(0, 1, (len(vertices), 4)).astype(F)
    return SimpleNamespace(vertices=vertices, faces=np.ascontiguousarray(faces, dtype=I).reshape(-1, 3), attributes=attributes, view=view, W=W, H=H, z_near=z_near,
                           culls=tuple(culls))


def _random_case():
    rng = np.random.default_rng(77)
    n = 300
    centre = np.stack([rng.uniform(-8, 78, n), rng.uniform(-8, 58, n)], axis=1)
    size = np.where(rng.uniform(size=n) < 0.8, rng.uniform(0.3, 4, n), rng.uniform(4, 40, n))          # most are pixel-sized, some are wide
    corners = np.concatenate([centre[:, None, :] + size[:, None, None] * rng.uniform(-1, 1, (n, 3, 2)), rng.uniform(1.5, 6, (n, 3, 1))], axis=2)
    corners[::37, 1, 2] = -1.0                        # some corners behind the camera
    corners[5::41, 2, :2] = corners[5::41, 1, :2]     # some degenerate
    return _case(corners.reshape(-1, 3), np.arange(3 * n).reshape(n, 3), W=70, H=50, culls=("none", "back", "front"), seed=11)


def _cases():
    C = {}
    C["wide"] = _case([(-300, -200, 2), (500, -100, 3), (20, 700, 2.5)], [(0, 1, 2)], seed=1)
    C["diagonal"] = _case([(10, 10, 2), (30, 10, 2.5), (30, 25, 3), (10, 25, 2.25)], [(0, 1, 2), (0, 2, 3)], seed=2)
    hub, angles = (40.0, 30.0), np.array([0.1, 0.9, 1.9, 2.6, 3.7, 4.4, 5.5])
    rim = [(hub[0] + 6.3 * np.cos(a), hub[1] + 6.3 * np.sin(a), 2 + 0.1 * k) for k, a in enumerate(angles)]
    C["fan"] = _case([(hub[0], hub[1], 2.5)] + rim, [(0, 1 + k, 1 + (k + 1) % 7) for k in range(7)], seed=3)
    C["slivers"] = _case([(5.2, 40.3, 2), (9.8, 40.4, 2), (7.5, 40.6, 2), (50.3, 5.2, 2), (50.7, 12.9, 3), (50.5, 12.9, 2),
                          (20.001, 20.001, 2), (20.0015, 20.001, 2), (20.001, 20.0012, 2), (1, 1, 2), (2, 2, 2), (3, 3, 2)],
                         [(0, 1, 2), (3, 4, 5), (6, 7, 8), (9, 10, 11)], seed=4)
    C["ties"] = _case([(12, 5, 2), (28, 6, 3), (20, 20, 2.5), (12, 30, 2), (28, 30, 2), (20, 44, 2), (16, 30, 2), (32, 30, 2), (24, 44, 2)],
                      [(0, 1, 2), (0, 1, 2), (6, 7, 8), (3, 4, 5)], seed=5)
    C["near"] = _case([(10, 10, 2), (30, 12, 2), (20, 30, 0.01), (10, 10, -2), (30, 12, -2), (20, 30, -3), (40, 10, 2), (60, 12, 2), (50, 30, 2)],
                      [(0, 1, 2), (3, 4, 5), (6, 7, 8)], seed=6)
    C["guard"] = _case([(10, 10, 2), (40000, 12, 2), (20, 30, 2), (10, 10, 2), (32767, 12, 2), (20, 30, 2)], [(0, 1, 2), (3, 4, 5)], seed=7)
    C["threshold"] = _case([(10, 5, 2), (17, 5, 2), (10, 12, 2), (30, 30, 2), (42, 30, 2), (30, 34, 2)], [(0, 1, 2), (3, 4, 5)], seed=8)
    C["bad_index"] = _case([(10, 10, 2), (30, 12, 2), (20, 30, 3)], [(0, 1, -1), (0, 1, 2), (3, 1, 2), (2, 1, 0), (0, 2 ** 31 - 1, 2)], seed=9)
    C["no_faces"] = _case([(10, 10, 2), (30, 12, 2), (20, 30, 3)], np.zeros((0, 3), I), seed=10)
    C["nothing"] = _case(np.zeros((0, 3)), np.zeros((0, 3), I), W=16, H=12)
    C["no_vertices"] = _case(np.zeros((0, 3)), [(0, 0, 0)], W=16, H=12)
    C["random"] = _random_case()
    for name, (volume, centre) in SURFACES.items():
        _, vertices, _, faces = tsdf_cases.extracted(volume)
        for k, (eye, W, H) in enumerate(CAMERAS):
            view = tsdf_cases.look_at(eye, centre, TAN, TAN * H / W)
            C[f"{name}_{k}"] = _finish(vertices, faces, view, W, H, culls=("none", "back", "front"), seed=20 + k)
    return C


CASES = _cases()
CLOSED = [n for n in CASES if n.split("_")[0] in SURFACES]
RUNS = [(name, cull) for name, c in CASES.items() for cull in c.culls]
PICTURES = ("diagonal", "random", "sphere_0")         # the cases of interpolate, normals and shade


@functools.lru_cache(maxsize=None)
def result(name, cull="none"):
    """mesh_render_ref.rasterize of a case; do not modify."""
    c = CASES[name]
    return ref.rasterize(c.vertices, c.faces, c.view, c.W, c.H, c.z_near, cull)


@functools.lru_cache(maxsize=None)
def pictures(name, cull="none"):
    """(interpolated [4, H, W], normals [3, H, W], nvalid [H, W], shaded [3, H, W]) of the restatement: the attributes over BACKGROUND, the
    shade of their first three channels over SHADE_BACKGROUND; do not modify."""
    c, r = CASES[name], result(name, cull)
    colour = ref.interpolate(r, c.faces, c.attributes, BACKGROUND)
    n, nvalid = ref.normals(r, c.vertices, c.faces, c.view)
    return colour, n, nvalid, ref.shade(colour[:3], n, nvalid, r.depth, c.view, AMBIENT, SHADE_BACKGROUND)


def planes(r):
    """The planes of a result in the order the emulator writes them."""
    return [r.counts, r.coverage, r.face, r.depth, r.valid, r.bary]
