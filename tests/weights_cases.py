"""Inputs, regime predicates and shared references for the direct tests of csrc/weights_kernels.hip
(test_weights_cases_host.py on the CPU, test_gpu_weights_direct.py on the device).  Plain numpy / torch, no GPU.

The predicates restate, on the host, the conditions under which the kernels take each of their branches, so that a test
named after a branch can assert that its inputs really enter it."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from oracle import weights_oracle as wo

MLP_FLOATS = 64 * 64 + 64 * 64 + 16 * 64
BOX_POINTS = 32          # points per workgroup of gp_hashgrid_bwd_slots_kernel
BOX_CAP = 1024           # HG_BOX_CAP
WM_BLOCK = 64            # points per block of gp_wm_fwd_kernel / gp_wm_bwd_kernel
WM_MAX_WORKGROUPS = 512
MIXED_SIDES = (0.02, 0.3, 3.0)


def grid(log2_T):
    return wo.grid_meta(16, 4, log2_T, 16)


def dense_levels(meta):
    """Indices of the levels that are indexed densely (res^3 fits the level's table)."""
    return [l for l in range(meta["n_levels"]) if meta["resolutions"][l] ** 3 <= meta["sizes"][l]]


def cells(xyz, scale):
    """floor(float32(fma(scale, x, 0.5))) as int64 [N, 3] (the double product of two floats is exact: one rounding)."""
    x = np.asarray(xyz, np.float32).astype(np.float64)
    return np.floor((x * float(np.float32(scale)) + 0.5).astype(np.float32)).astype(np.int64)


def boxed_map(xyz, perm, meta):
    """bool [workgroups, dense levels]: does the table-gradient kernel accumulate this workgroup's 32 slots of this dense level in
    its LDS box, i.e. do the cell extents (max - min + 2) per axis multiply to at most BOX_CAP."""
    x = np.asarray(xyz, np.float32)
    if perm is not None:
        x = x[np.asarray(perm, np.int64)]
    starts = np.arange(0, x.shape[0], BOX_POINTS)
    dl = dense_levels(meta)
    out = np.zeros((len(starts), len(dl)), dtype=bool)
    for k, l in enumerate(dl):
        c = cells(x, meta["scales"][l])
        ext = np.maximum.reduceat(c, starts, axis=0) - np.minimum.reduceat(c, starts, axis=0) + 2
        out[:, k] = np.prod(ext, axis=1) <= BOX_CAP
    return out


def wm_blocks_per_workgroup(n, cap=WM_MAX_WORKGROUPS):
    """(fewest, most) 64-point blocks one workgroup of the fused kernels walks."""
    # restates the launch arithmetic of gp_weights_forward / gp_weights_backward (blocks of 64 points, at most 512 workgroups): it
    # must be changed together with it.  Only the forward honours gp_debug_option(4, cap); the backward always launches up to 512
    nb = (n + WM_BLOCK - 1) // WM_BLOCK
    g = min(nb, cap)
    return nb // g, (nb + g - 1) // g


def knn_form(n, K, hybrid):
    # restates the launch arithmetic of gp_knn_keypoints (chunks of 256 points, `resident` workgroups, KNN_TILE = 256):
    # it must be changed together with it
    nchunks = (n + 255) // 256
    resident = 256 * (4 if hybrid else 8)
    if K > 256:
        return "restaged"
    return "persistent" if nchunks > resident else "one_chunk_per_workgroup"


def clustered_points(n, sides=MIXED_SIDES, seed=0):
    """Groups of 32 points in cubes around uniform centres in [-1.5, 1.5]^3; the cube side cycles through `sides`."""
    rng = np.random.default_rng(seed)
    groups = (n + 31) // 32
    centres = rng.uniform(-1.5, 1.5, size=(groups, 3))
    side = np.asarray(sides, np.float64)[np.arange(groups) % len(sides)]
    pts = centres[:, None, :] + side[:, None, None] * rng.uniform(-0.5, 0.5, size=(groups, 32, 3))
    return pts.reshape(-1, 3)[:n].astype(np.float32)


EXACT_ON_LEVEL0 = (0.5, -0.5, 1.5, 0.1)      # fma(15, x, 0.5) is an integer in float32: interpolation weight 0


def edge_points(meta):
    """Points at the places an index or a weight goes wrong: the origin, positions on a cell boundary of level 0 (weight 0: the
    kernels skip zero contributions), the last cell of every level on both sides, far outside (the cell index wraps), twins."""
    p = [(0.0, 0.0, 0.0), (0.0, 0.3, -0.7), (0.6, 0.0, 0.0)]
    p += [(v, v, v) for v in EXACT_ON_LEVEL0] + [(0.5, -0.5, 0.1), (1.5, 0.3, -0.5)]
    for l in range(meta["n_levels"]):
        s = np.float32(meta["scales"][l])
        e = float(np.float32(meta["resolutions"][l] - 1) / s)
        p += [(e, e, e), (-e, -e, -e), (e, -e, 0.25)]
    p += [(1e4, 1e4, 1e4), (-1e4, -1e4, -1e4), (1e4, -1e4, 0.25)]
    p += [(0.3, -0.2, 0.7), (0.3, -0.2, 0.7)]
    return np.asarray(p, np.float32)


def points_with_edges(n, meta, seed, half=1.7):
    rng = np.random.default_rng(seed)
    e = edge_points(meta)
    rest = rng.uniform(-half, half, size=(max(n - len(e), 0), 3)).astype(np.float32)
    return np.concatenate([e, rest])[:n]


def model_params(meta, seed):
    """Flat float32 parameters: three Xavier-uniform matrices (ALL 16 rows of the padded output layer non-zero, so that a kernel
    which forgets the n_out mask shows) and a standard-normal table (features of order 1)."""
    rng = np.random.default_rng(seed)

    def xavier(o, i):
        return rng.uniform(-1.0, 1.0, size=o * i) * math.sqrt(6.0 / (i + o))

    return np.concatenate([xavier(64, 64), xavier(64, 64), xavier(16, 64), rng.normal(size=meta["total"] * 4)]).astype(np.float32)


# ---- backward reference ---------------------------------------------------------------------------------------------
AMBIGUOUS_Z = 1e-5       # a hidden pre-activation closer to 0 than this has an ill-defined ReLU mask in float32: ten times the
#                          largest deviation of the float32 oracle from the float64 one on these inputs (1.04e-6)
AMBIGUOUS_CAP = 0.01     # at most this share of the points may be excluded

# name: (log2_T, n_out, n, points, seed)
BACKWARD_CASES = {
    "boxed_small_nout13": (15, 13, 300, "clustered", 313),
    "boxed_small_nout16": (15, 16, 300, "clustered", 326),
    "four_dense_levels": (17, 13, 4097, "clustered", 4110),
    "persistent_mixed": (15, 16, 65573, "clustered", 65589),
    "persistent_mixed_nout13": (15, 13, 65573, "clustered", 65602),      # the n_out mask across the multi-block accumulation
}


def case_points(kind, n, meta, seed):
    return clustered_points(n, MIXED_SIDES, seed) if kind == "clustered" else points_with_edges(n, meta, seed)


def grad_slices(meta):
    """name -> slice of the flat parameter vector: the three matrices, then every level's part of the table."""
    s = {"W1": slice(0, 4096), "W2": slice(4096, 8192), "W3": slice(8192, 9216)}
    for l in range(meta["n_levels"]):
        a = MLP_FLOATS + 4 * meta["offsets"][l]
        s[f"table[{l}]"] = slice(a, a + 4 * meta["sizes"][l])
    return s


def _oracle_grad(xyz, params, gy, meta, n_out, dtype):
    p = torch.tensor(params, dtype=dtype, requires_grad=True)
    out = wo.weights_model(torch.tensor(xyz, dtype=dtype), p, meta, n_out)
    (out * torch.tensor(gy, dtype=dtype)).sum().backward()
    return p.grad.numpy().astype(np.float64)


def ambiguous_rows(xyz, params, meta):
    """bool [N]: any of the 128 hidden pre-activations of the float64 oracle lies within AMBIGUOUS_Z of 0."""
    with torch.no_grad():
        p = torch.tensor(params, dtype=torch.float64)
        feat = wo.hash_encode(torch.tensor(xyz, dtype=torch.float64), p[MLP_FLOATS:].view(-1, 4), meta)
        z1 = feat @ p[0:4096].view(64, 64).t()
        z2 = torch.relu(z1) @ p[4096:8192].view(64, 64).t()
        zmin = torch.minimum(z1.abs().min(dim=1).values, z2.abs().min(dim=1).values)
    return (zmin < AMBIGUOUS_Z).numpy()


def errors(g, ref, meta):
    """name -> (rel-L2, max-abs relative to the reference's largest magnitude) per tensor and per table level."""
    out = {}
    for name, sl in grad_slices(meta).items():
        d, r = np.asarray(g[sl], np.float64) - ref[sl], ref[sl]
        out[name] = (float(np.linalg.norm(d) / max(np.linalg.norm(r), 1e-300)), float(np.abs(d).max() / max(np.abs(r).max(), 1e-300)))
    return out


@functools.lru_cache(maxsize=None)
def backward_reference(name):
    """Inputs and float64 gradients of a backward case, computed once and shared (arrays are read-only).  `yardstick` is the error
    of the SAME oracle run in float32 against the float64 one: what float32 accumulation alone costs at this size."""
    log2_T, n_out, n, kind, seed = BACKWARD_CASES[name]
    meta = grid(log2_T)
    xyz = case_points(kind, n, meta, seed)
    params = model_params(meta, seed + 1)
    excluded = ambiguous_rows(xyz, params, meta)
    gy = np.random.default_rng(seed + 2).normal(size=(n, n_out)).astype(np.float32)
    gy[excluded] = 0.0
    g64 = _oracle_grad(xyz, params, gy, meta, n_out, torch.float64)
    g32 = _oracle_grad(xyz, params, gy, meta, n_out, torch.float32)
    ref = dict(meta=meta, log2_T=log2_T, n_out=n_out, n=n, xyz=xyz, params=params, gy=gy, excluded=int(excluded.sum()), excluded_share=float(excluded.mean()), grad=g64,
               yardstick=errors(g32, g64, meta))
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def bar(yardstick):
    """The existing bar (1e-5 at n = 300), or four times the float32 oracle's own error where that is larger: the atomics of the
    kernels sum in another order than the oracle does."""
    return max(1e-5, 4.0 * yardstick)


# ---- kNN ------------------------------------------------------------------------------------------------------------
def knn_inputs(n, K, seed, feat_scale=0.1, ties=()):
    """Points and keypoints (positions + 32 features); `ties` lists pairs (a, b) of keypoints made coincident."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1.3, 1.3, size=(n, 3)).astype(np.float32)
    feat = (feat_scale * rng.uniform(-1, 1, size=(n, 32))).astype(np.float32)
    kp = rng.uniform(-1.3, 1.3, size=(K, 3)).astype(np.float32)
    kpf = (feat_scale * rng.uniform(-1, 1, size=(K, 32))).astype(np.float32)
    for a, b in ties:
        kp[b], kpf[b] = kp[a], kpf[a]
    return xyz, feat, kp, kpf


def knn_oracle(xyz, feat, kp, kpf, nn, hybrid, amplify=5.0):
    if not hybrid:
        return wo.knn(xyz, kp, nn)
    a = np.float32(amplify)
    return wo.knn(np.concatenate([xyz, a * feat], 1), np.concatenate([kp, a * kpf], 1), nn)


# (K, nn, coincident pairs): inside a packed pair (even j, j + 1), across the tile boundary (255, 256), at the unpaired last
# keypoint of an odd K together with its predecessor, at the last (odd) index of a full tile
KNN_TIE_CASES = [
    (9, 1, ((0, 1), (4, 5), (7, 8))),
    (9, 6, ((2, 3), (7, 8))),
    (256, 6, ((100, 101), (254, 255))),
    (257, 8, ((255, 256), (10, 11))),
    (301, 5, ((255, 256), (299, 300), (2, 3))),
]
