"""Seeded cases of the depth entries, shared by the host test (the stand-alone build of csrc/depth_core.h) and the GPU test (depth_ops).
CASES: name -> a namespace with H, W, view, accum, alpha, alpha_min, depth, valid, image, pred, gt, mask, scale, gt_min, gt_max.  The
sizes are the smallest that reach each regime: 1 x 1; 3 x 5, where only the centre has four neighbours; 37 x 53, two tiles of 1024
pixels with a ragged last one; 240 x 320; 520 x 512, 260 tiles: the finalising workgroup's lane loop and the tile scan pass 256.
`reference` holds depth_ref's answers, computed once."""
import functools
import math
from types import SimpleNamespace

import numpy as np

import depth_ref as ref
import trajectory_cases as tc
from gaussianprediction_amd.cameras import Camera

F = np.float32
NAN, INF = float("nan"), float("inf")
ALPHA_MIN = 1e-3
BELOW = np.nextafter(F(ALPHA_MIN), F(0))           # one ulp below the float32 alpha_min


def view(rotated, W, H, tanfovx=None, tanfovy=None):
    """A view of depth_ref (and of flow_ref: .vm, .pm): the package's Camera for trajectory_cases' pose, on the host; .cam is that Camera."""
    c = tc.camera(rotated, W, H)
    tx = math.tan(c.FoVx / 2) if tanfovx is None else tanfovx
    ty = tx * H / W if tanfovy is None else tanfovy
    cam = Camera(R=c.R, T=c.T, FoVx=2 * math.atan(tx), FoVy=2 * math.atan(ty), width=W, height=H)
    vm = cam.world_view_transform.numpy()
    c2w = np.linalg.inv(vm.astype(np.float64)).astype(F)
    return SimpleNamespace(c2w=c2w.reshape(16).copy(), tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5), W=W, H=H, cam=cam,
                           vm=vm.reshape(16).copy(), pm=cam.full_proj_transform.numpy().reshape(16).copy())


def _pattern(kind, H, W, rng):
    plane = H * W
    v = np.ones(plane, np.uint8)
    if kind == "none":
        v[:] = 0
    elif kind == "checker":
        ys, xs = np.divmod(np.arange(plane), W)
        v = ((xs + ys) % 2).astype(np.uint8)
    elif kind == "straddle":                       # one run of valid pixels across the first tile boundary
        v[:] = 0
        v[max(0, min(plane, 1024) - 37):min(plane, 1024 + 29)] = 1
    elif kind == "tile_gap":                       # one whole tile empty between full ones
        v[1024:2048] = 0
    elif kind == "random":
        v = (rng.uniform(size=plane) > 0.3).astype(np.uint8)
        v[v != 0] = rng.integers(1, 256, int((v != 0).sum()))      # any byte but 0 counts
    else:
        assert kind == "all", kind
    return v.reshape(H, W)


def _case(name, H, W, seed, kind="random", rotated=True):
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    surface = 3.0 + 0.4 * np.sin(xs / 7.0) + 0.3 * np.cos(ys / 5.0) + rng.normal(0, 0.01, (H, W))
    alpha = rng.uniform(0.0, 1.0, (H, W)).astype(F)
    accum = (surface * alpha).astype(F)
    depth = surface.astype(F)
    valid = _pattern(kind, H, W, rng)
    image = rng.uniform(0, 1, (3, H, W)).astype(F)
    gt = (surface * rng.choice([0.7, 0.9, 1.0, 1.1, 1.3, 2.2], (H, W)) + rng.normal(0, 0.05, (H, W))).astype(F)
    pred = depth.copy()
    mask = _pattern("random", H, W, rng)
    gt_min, gt_max = F(1.5), F(6.0)
    if H >= 3 and W >= 5:                          # the special values, along the first rows
        k = min(W, 12)
        a_row = [0.0, BELOW, F(ALPHA_MIN), 0.5, 0.5, 0.5, 0.5, 0.5, 0.0, 0.5, 0.5, 1.0][:k]
        c_row = [1.0, 3 * BELOW, 3 * F(ALPHA_MIN), 0.0, NAN, INF, -INF, -1.5, 0.0, 3e38, 1e-45, 3.0][:k]     # x/0, below, at, 0, NaN, +-inf, negative, 0/0, big, tiny
        alpha[0, :k], accum[0, :k] = a_row, c_row
        if k > 9:
            alpha[0, 9] = 1e-3                     # 3e38 / 1e-3 overflows
        d_row = [0.0, NAN, INF, -2.0, 1.75, 4.75, -0.0, 2.5][:min(W, 8)]          # (1.75 and 4.75 are the extremes of every coloured depth)
        depth[1, :len(d_row)] = d_row
        if kind in ("all", "random"):
            valid[1, :len(d_row)] = 1              # (the special depths are offered as valid: the colour tests them again)
        pred[2, :5] = [2.5, 2.0, 3.0, 4.0, 0.0]
        gt[2, :5] = [2.0, 2.5, gt_min, gt_max, 2.0]                   # d/g and g/d exactly 1.25; gt on both bounds; a pred of 0
        mask[2, :5] = 1
        if W > 8:
            pred[2, 5:9] = [NAN, 2.0, 2.0, -1.0]
            gt[2, 5:9] = [2.0, INF, np.nextafter(gt_max, F(INF)), 2.0]    # just beyond gt_max
            mask[2, 5:9] = 1
    scale = F(rng.uniform(0.8, 1.2))
    return SimpleNamespace(name=name, H=H, W=W, view=view(rotated, W, H), accum=accum, alpha=alpha, alpha_min=ALPHA_MIN, depth=depth, valid=valid,
                           image=image, pred=pred, gt=gt, mask=mask, scale=scale, gt_min=float(gt_min), gt_max=float(gt_max))


def _cases():
    cases = [_case("1x1", 1, 1, 300, "all"), _case("1x1_invalid", 1, 1, 301, "none"), _case("3x5", 3, 5, 302, "all", rotated=False),
             _case("37x53_all", 37, 53, 303, "all"), _case("37x53_none", 37, 53, 304, "none"), _case("37x53_checker", 37, 53, 305, "checker"),
             _case("37x53_straddle", 37, 53, 306, "straddle"), _case("37x53_random", 37, 53, 307, "random", rotated=False),
             _case("240x320_tile_gap", 240, 320, 308, "tile_gap"), _case("240x320_random", 240, 320, 309, "random"),
             _case("520x512_random", 520, 512, 310, "random"), _case("520x512_straddle", 520, 512, 311, "straddle")]
    c = _case("37x53_constant", 37, 53, 312, "all")          # one coloured value: lo == hi
    c.depth[:] = 2.5
    cases.append(c)
    c = _case("37x53_extremes", 37, 53, 313, "all")          # the smallest denormal and a value whose reciprocal is one
    c.depth[1, 4:6] = [1e-45, 3e38]
    cases.append(c)
    return {c.name: c for c in cases}


CASES = _cases()
BG = (0.25, 0.5, 1.0)
# (name, mode, lo, hi): derived ranges, a given one, lo > hi (treated as derived), lo == hi given (derived as well)
COLOUR_MODES = (("disparity", 1, 0.0, 0.0), ("depth", 0, 0.0, 0.0), ("depth_given", 0, 2.5, 3.25), ("disparity_given", 1, 0.25, 0.5),
                ("swapped_is_derived", 0, 4.0, 2.0), ("equal_is_derived", 1, 2.0, 2.0))


def lut():
    """A table whose rows tell themselves apart: row r is (r / 255, 1 - r / 255, (r % 16) / 15)."""
    r = np.arange(256)
    return np.stack([r / 255.0, 1.0 - r / 255.0, (r % 16) / 15.0], axis=1).astype(F)


@functools.lru_cache(maxsize=None)
def reference(name):
    """depth_ref's answers for a case; do not modify.  resolve (depth, valid); colour {(mode name, masked): (out, range, rows)}; normals
    {masked: (normals, nvalid)}; picture; unproject {masked: (points, colors, index, count)}; metrics {(masked, scaled): row}, metrics64
    likewise."""
    c = CASES[name]
    colour = {(m, masked): ref.colorize(c.depth, c.valid if masked else None, mode, lo, hi, lut(), BG) for m, mode, lo, hi in COLOUR_MODES
              for masked in (False, True)}
    normals = {masked: ref.normals(c.depth, c.valid if masked else None, c.view) for masked in (False, True)}
    unproject = {masked: ref.unproject(c.depth, c.valid if masked else None, c.image, c.view) for masked in (False, True)}
    combos = [(masked, scaled) for masked in (False, True) for scaled in (False, True)]
    args = lambda masked, scaled: (c.pred[None], c.gt[None], c.mask[None] if masked else None, [c.scale] if scaled else None, c.gt_min, c.gt_max)   # noqa: E731
    return SimpleNamespace(resolve=ref.resolve(c.accum, c.alpha, c.alpha_min), colour=colour, normals=normals,
                           picture=ref.normals_image(*normals[True], BG), unproject=unproject,
                           metrics={k: ref.metrics(*args(*k))[0] for k in combos}, metrics64={k: ref.metrics64(*args(*k))[0] for k in combos})


LOG_COLUMNS, COUNT_COLUMN = (4, 8), 0
PLAIN_COLUMNS = (1, 2, 3, 5, 6, 7, 9, 10)          # no logf in them: AbsRel, SqRel, RMSE, the deltas, scale, mean gt


def log_bar(want32, want64):
    """The bar of the two log columns: max(8 x |float32 restatement - float64 restatement|, 1e-9), from the restatement alone."""
    return np.maximum(8.0 * np.abs(np.asarray(want32)[list(LOG_COLUMNS)] - np.asarray(want64)[list(LOG_COLUMNS)]), 1e-9)
