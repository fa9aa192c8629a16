"""Seeded cases of the trajectory drawing, shared by the host test (the stand-alone build of csrc/trajectory_core.h) and the GPU test
(TrajectoryCanvas), at W x H = 67 x 45.  A case: view, H, W, steps (the [N, 3] float32 positions of each step), idx ([P] int32 or
None), P, min_depth, colors [P, 3] float32, base [3, H, W] float32.  `reference(case)` is trajectory_ref's answer, computed once."""
import functools
import math
from types import SimpleNamespace

import numpy as np

import trajectory_ref as ref

W, H = 67, 45
FOVX = 0.9
NAN, INF = float("nan"), float("inf")


def camera(rotated, Wc=W, Hc=H):
    """A camera with R (stored transposed, as the loaders do), T, FoVx.  rotated=False: R = I and T = 0, so zc is the point's z exactly."""
    if not rotated:
        R, T = np.eye(3), np.zeros(3)
    else:
        a, b = 0.3, -0.2
        Ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
        R, T = Ry @ Rx, np.array([0.1, -0.05, 2.5])
    return SimpleNamespace(R=R, T=T, FoVx=FOVX, image_width=Wc, image_height=Hc)


def centre(p):
    """A float coordinate that truncates to the integer p with half a pixel of room."""
    return p + 0.5 if p >= 0 else p - 0.5


def unproject(view, pixels, zc=1.0, Wc=W, Hc=H):
    """[P, 3] float32 world points that project to the integer `pixels` [P, 2] at depth zc (computed in float64; half a pixel of room
    covers the float32 projection's error up to coordinates of 2^20)."""
    pixels = np.asarray(pixels, dtype=np.int64).reshape(-1, 2)
    f, den = Wc / (2 * math.tan(view.FoVx / 2)), zc + 0.0001
    cam = np.array([[(centre(x) - Wc / 2) / f * den, (centre(y) - Hc / 2) / f * den, zc] for x, y in pixels.tolist()]).reshape(-1, 3)
    return ((cam - view.T) @ view.R.T).astype(np.float32)          # world = R (cam - T), R being the stored (transposed) matrix


def _case(name, view, steps, seed, idx=None, P=None, min_depth=None, Wc=W, Hc=H):
    rng = np.random.default_rng(seed)
    steps = [np.ascontiguousarray(s, dtype=np.float32).reshape(-1, 3) for s in steps]
    P = (len(steps[0]) if idx is None else len(idx)) if P is None else P
    return SimpleNamespace(name=name, view=view, H=Hc, W=Wc, steps=steps, idx=None if idx is None else np.asarray(idx, dtype=np.int32), P=P,
                           min_depth=min_depth, colors=rng.uniform(0.05, 1.0, (P, 3)).astype(np.float32),
                           base=rng.uniform(1.5, 2.5, (3, Hc, Wc)).astype(np.float32))       # (no colour equals a base pixel)


def _paths(name, view, paths, seed, **kw):
    """paths: [S][P] integer pixels -> a case whose points project exactly there (checked against the restatement's projection)."""
    paths = np.asarray(paths, dtype=np.int64)
    steps = [unproject(view, p) for p in paths]
    c = ref.constants(view, H, W)
    for p, xyz in zip(paths, steps):
        assert np.array_equal(ref.project(c, xyz), p.astype(np.int32)), name
    return _case(name, view, steps, seed, **kw)


def _from_deltas(name, deltas, seed, rotated=False):
    """One point per delta, both ways round: a -> a + d and a + d -> a, the starts spread over the image."""
    rng = np.random.default_rng(seed)
    a, b = [], []
    for dx, dy in deltas:
        s = [int(rng.integers(20, W - 20)), int(rng.integers(18, H - 18))]
        e = [s[0] + dx, s[1] + dy]
        a += [s, e]
        b += [e, s]
    return _paths(name, camera(rotated), [a, b], seed)


def build():
    v0, v1 = camera(False), camera(True)
    cases = []
    octants = [(17, 7), (7, 17), (-7, 17), (-17, 7), (-17, -7), (-7, -17), (7, -17), (17, -7)]
    cases.append(_from_deltas("octants", octants, 1, rotated=True))
    cases.append(_from_deltas("axes_diagonals_zero", [(19, 0), (-19, 0), (0, 16), (0, -16), (13, 13), (-13, 13), (13, -13), (-13, -13), (0, 0)], 2))
    ties = [(2, 1), (4, 2), (6, 3), (5, 5), (3, 0)]
    ties = [(sx * dx, sy * dy) for dx, dy in ties for sx in (1, -1) for sy in (1, -1)] + [(sx * dy, sy * dx) for dx, dy in ties for sx in (1, -1) for sy in (1, -1)]
    cases.append(_from_deltas("tie_slopes", ties, 3))
    far = 100000
    clip_a = [[-far, 10], [30, 20], [-far, -70000], [far, 20], [12, -far], [40, far], [-far + 7, -far], [far, -far + 31],
              [-far, 5], [80, -20], [-30, -30], [far, far]]
    clip_b = [[30, 20], [far, -40000], [far, 70040], [-far, 25], [50, far], [40, 3], [far, far - 11], [-far, far],
              [-50, 30], [90, 100], [-10, 200], [far - 3, far - 50]]
    cases.append(_paths("clip_from_far_outside", v0, [clip_a, clip_b, clip_a], 4))          # (and back again: leaving where they entered)
    # non-finite coordinates and the zero denominator, each at the first, the middle and the last of three steps
    rng = np.random.default_rng(5)
    walk = [rng.integers(5, [W - 5, H - 5], (12, 2)) for _ in range(3)]
    steps = [unproject(v0, p) for p in walk]
    bad = [(NAN, 0), (INF, 0), (-INF, 1), (NAN, 2), (INF, 2), (-INF, 2)]
    for j, (value, axis) in enumerate(bad):
        steps[j % 3][j, axis] = value
    for j, s in ((6, 0), (7, 1), (8, 2)):
        steps[s][j, 2] = -0.0001               # zc = -0.0001f exactly under the identity camera: den = 0
    cases.append(_case("nonfinite_and_zero_denominator", v0, steps, 5))
    c = ref.constants(v0, H, W)
    assert all((ref.project(c, steps[s])[j] == ref.NOT_DRAWABLE).all() for j, s in ((0, 0), (1, 1), (2, 2), (3, 0), (6, 0), (7, 1), (8, 2)))
    assert (ref.project(c, steps[0])[9:] != ref.NOT_DRAWABLE).all()
    # just under 2^20 is drawn (a line a million pixels long, of which the image sees its start); just over is not
    lim = 2 ** 20
    a = [[10, 10], [40, 30], [20, 5], [50, 40]]
    b = [[lim - 8, 20], [33, -(lim - 8)], [lim + 8, 9], [45, -(lim + 8)]]
    steps = [unproject(v0, a), unproject(v0, b)]
    got = ref.project(c, steps[1])
    assert np.array_equal(got[:2], np.asarray(b[:2], np.int32)) and (got[2:] == ref.NOT_DRAWABLE).all()
    cases.append(_case("coordinate_limit", v0, steps, 6))
    # identical paths: the highest j owns every pixel
    path = [[8, 8], [55, 30], [20, 40]]
    cases.append(_paths("identical_paths", v1, [[p] * 5 for p in path], 7))
    # a later step over an earlier one: point 1 draws first (step 1), point 0 crosses it at step 2 with the lower j and still wins
    cases.append(_paths("later_step_overdraws", v1, [[[33, 40], [5, 22]], [[33, 40], [60, 22]], [[33, 4], [60, 22]]], 8))
    # idx with duplicates into N = 500, and one row outside on either side
    rng = np.random.default_rng(9)
    cloud = unproject(v1, rng.integers(-10, [W + 10, H + 10], (500, 2)), zc=1.7)
    steps = [cloud + np.float32(0.04) * s * rng.normal(size=(500, 3)).astype(np.float32) for s in range(4)]
    idx = rng.integers(0, 500, 60)
    idx[10:20] = idx[0:10]
    idx[58], idx[59] = 500, -1
    cases.append(_case("idx_with_duplicates", v1, steps, 9, idx=idx))
    cloud_steps = steps
    # points behind the camera project into the image; min_depth leaves them out
    front, behind = rng.integers(5, [W - 5, H - 5], (2, 6, 2)), rng.integers(5, [W - 5, H - 5], (2, 6, 2))
    steps = [np.concatenate([unproject(v0, front[s]), unproject(v0, behind[s], zc=-1.0)]) for s in range(2)]
    cases.append(_case("behind_the_camera", v0, steps, 10))
    cases.append(_case("behind_the_camera_min_depth", v0, steps, 10, min_depth=0.0))
    cases.append(_paths("one_point_two_steps", v1, [[[3, 3]], [[60, 41]]], 11))
    cases.append(_paths("one_step", v1, [[[3, 3], [20, 20], [60, 41], [1, 44], [66, 0]]], 12))
    cases.append(_case("no_points", v1, [np.zeros((0, 3), np.float32)] * 2, 13))
    cases.append(_case("first_rows_of_a_longer_array", v1, [s[:40] for s in cloud_steps], 14, P=25))
    return {c.name: c for c in cases}


CASES = build()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(px per step, owner, image over zero [3, H, W], image over the base) of trajectory_ref; do not modify."""
    c = CASES[name]
    pxs, owner = ref.run(c.view, c.H, c.W, c.steps, c.idx, c.P, c.min_depth)
    return pxs, owner, ref.resolve(owner, c.colors, c.P), ref.resolve(owner, c.colors, c.P, c.base)


def random_walks(P=70000, Wc=320, Hc=240, S=4, seed=21):
    """The multi-workgroup regime: P short random walks, some leaving the image."""
    rng = np.random.default_rng(seed)
    view = camera(True, Wc, Hc)
    pos = rng.integers(-6, [Wc + 6, Hc + 6], (P, 2))
    steps = []
    for _ in range(S):
        steps.append(unproject(view, pos, zc=2.0, Wc=Wc, Hc=Hc))
        pos = pos + rng.integers(-5, 6, (P, 2))
    return _case("random_walks", view, steps, seed, Wc=Wc, Hc=Hc)
