"""A numpy restatement of the trajectory drawing (gaussianprediction_amd/csrc/gp_trajectory.h), independent of csrc/trajectory_core.h:
the float32 projection operation by operation, the INCREMENTAL Bresenham line on Python integers, unclipped, with a bounds test per
pixel, and a dictionary of owners.  Deliberately not the closed form the kernels use."""
import math
from types import SimpleNamespace

import numpy as np

NOT_DRAWABLE = -2 ** 31
LIMIT = np.float32(2 ** 20)
f32 = np.float32


def constants(view, H, W):
    """R = view.R.T, t = view.T, f = fov2focal(view.FoVx, W), cx = W / 2, cy = H / 2, all float32."""
    return SimpleNamespace(R=np.asarray(view.R, dtype=np.float64).T.astype(f32), t=np.asarray(view.T, dtype=np.float64).astype(f32),
                           f=f32(W / (2 * math.tan(view.FoVx / 2))), cx=f32(W / 2), cy=f32(H / 2))


def uv(c, xyz):
    """(u, v, zc) float32 of xyz [P, 3] float32: every operation rounds once, in the order of the definition."""
    x, y, z = (np.ascontiguousarray(xyz[:, k], dtype=f32) for k in range(3))
    with np.errstate(all="ignore"):
        cam = [((c.R[r, 0] * x + c.R[r, 1] * y) + c.R[r, 2] * z) + c.t[r] for r in range(3)]
        den = cam[2] + f32(0.0001)
        u = (c.f * cam[0]) / den + c.cx
        v = (c.f * cam[1]) / den + c.cy
    assert u.dtype == v.dtype == cam[2].dtype == f32
    return u, v, cam[2]


def project(c, xyz, min_depth=None):
    """[P, 2] int32 pixels, NOT_DRAWABLE twice where the point is not drawable."""
    u, v, zc = uv(c, xyz)
    with np.errstate(all="ignore"):
        ok = np.isfinite(u) & np.isfinite(v) & (np.abs(u) < LIMIT) & (np.abs(v) < LIMIT)
        if min_depth is not None:
            ok &= ~(zc <= f32(min_depth))
    px = np.full((len(u), 2), NOT_DRAWABLE, dtype=np.int32)
    px[ok, 0] = np.trunc(u[ok]).astype(np.int32)
    px[ok, 1] = np.trunc(v[ok]).astype(np.int32)
    return px


def line(a, b):
    """Every pixel (x, y) of the segment from a to b, image or not, in drawing order."""
    ax, ay, bx, by = int(a[0]), int(a[1]), int(b[0]), int(b[1])
    dx, dy = bx - ax, by - ay
    xmajor = abs(dx) >= abs(dy)
    dm, dn = (abs(dx), abs(dy)) if xmajor else (abs(dy), abs(dx))
    sm, sn = ((-1 if dx < 0 else 1), (-1 if dy < 0 else 1)) if xmajor else ((-1 if dy < 0 else 1), (-1 if dx < 0 else 1))
    major, minor = (ax, ay) if xmajor else (ay, ax)
    if dm == 0:
        yield ax, ay
        return
    e = dm - 2 * dn
    for _ in range(dm + 1):
        yield (major, minor) if xmajor else (minor, major)
        if e < 0:
            minor += sn
            e += 2 * dm
        e -= 2 * dn
        major += sm


def draw(owners, prev, now, s, P, H, W):
    """Step s: the segments from prev to now [P, 2] into the dictionary {(y, x): key}."""
    for j in range(len(now)):
        if prev[j, 0] == NOT_DRAWABLE or now[j, 0] == NOT_DRAWABLE:
            continue
        key = s * P + j + 1
        for x, y in line(prev[j], now[j]):
            if 0 <= x < W and 0 <= y < H and owners.get((y, x), 0) < key:
                owners[(y, x)] = key


def resolve(owner, colors, P, base=None):
    """[3, H, W] float32: the owner's colour, else the base's pixel, else zero."""
    H, W = owner.shape
    out = np.zeros((3, H, W), f32) if base is None else np.array(base, dtype=f32, copy=True)
    touched = owner != 0
    if P > 0 and touched.any():
        j = (owner[touched].astype(np.int64) - 1) % P
        for ch in range(3):
            out[ch][touched] = colors[j, ch]
    return out


def run(view, H, W, steps, idx=None, P=None, min_depth=None):
    """steps: the [N, 3] float32 positions of each step.  Returns (px per step, owner [H, W] uint32)."""
    c = constants(view, H, W)
    owners, pxs, prev = {}, [], None
    for s, xyz in enumerate(steps):
        xyz = np.asarray(xyz, dtype=f32)
        if idx is None:
            pts, inside = xyz[:P], np.ones(P, bool)
        else:
            inside = (idx >= 0) & (idx < len(xyz))
            pts = xyz[np.where(inside, idx, 0)] if len(xyz) else np.zeros((len(idx), 3), f32)
        now = project(c, pts, min_depth)
        now[~inside] = NOT_DRAWABLE
        if s > 0:
            draw(owners, prev, now, s, len(now), H, W)
        pxs.append(now)
        prev = now
    owner = np.zeros((H, W), np.uint32)
    for (y, x), key in owners.items():
        owner[y, x] = key
    return pxs, owner
