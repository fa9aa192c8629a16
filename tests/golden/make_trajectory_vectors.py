"""Build-container script (needs the reference tree; NOT run on the GPU box): records the reference's own projection of
project_trajectory [REF eval.py:48-62] -- `transpose` and `pi` of [REF utils/camera_utils.py:195-267] on CPU float32 tensors, then
`.numpy().astype(np.int32)` -- for a seeded cloud of 4000 points under three cameras.  The two functions are compiled from their `ast`
nodes alone: the module's top-level imports need CUDA-only packages.  Writes tests/golden/trajectory_projection.npz (data: inputs,
the reference's float32 (u, v) and its integer pixels); tests/test_trajectory_host.py holds the projection of csrc/trajectory_core.h and
of tests/trajectory_ref.py against it.

    python tests/golden/make_trajectory_vectors.py /path/to/reference
"""
import ast
import math
import os
import sys

import numpy as np
import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "trajectory_projection.npz")
N = 4000
SIZES = [(1352, 1014), (67, 45), (800, 800)]          # W, H


def reference_functions(ref):
    path = os.path.join(ref, "utils", "camera_utils.py")
    tree = ast.parse(open(path).read(), path)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("transpose", "pi")]
    assert [n.name for n in keep] == ["transpose", "pi"]
    scope = {"torch": torch, "np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), scope)
    return scope["transpose"], scope["pi"]


def cameras(rng):
    """(R as the loaders store it -- camera to world --, T, FoVx) of three cameras looking at the origin from a distance of about 4."""
    out = []
    for k in range(3):
        eye = rng.normal(size=3)
        eye *= (3.5 + k) / np.linalg.norm(eye)
        fwd = -eye / np.linalg.norm(eye)
        right = np.cross(fwd, [0.0, -1.0, 0.0])
        right /= np.linalg.norm(right)
        c2w = np.stack([right, np.cross(fwd, right), fwd], axis=1)
        out.append((c2w, -c2w.T @ eye, 0.6 + 0.25 * k))
    return out


def main():
    transpose, pi = reference_functions(sys.argv[1])
    rng = np.random.default_rng(38)
    xyz = rng.uniform(-1.6, 1.6, (N, 3)).astype(np.float32)
    Rs, Ts, fovs, uvs, pixels = [], [], [], [], []
    for (R, T, fov), (W, H) in zip(cameras(rng), SIZES):
        Rt = torch.from_numpy(R.T).to(torch.float32)                   # [REF eval.py:48-56], on the CPU
        t = torch.from_numpy(T).to(torch.float32)
        focal = W / (2 * math.tan(fov / 2))                            # fov2focal [REF utils/graphics_utils.py]
        K = torch.ones([3, 3], dtype=torch.float32)
        K[0, 0] = focal
        K[0, 2] = W / 2
        K[1, 1] = focal
        K[1, 2] = H / 2
        K[2, 2] = 1.0
        uv, _ = pi(K, transpose(Rt, t, torch.from_numpy(xyz)))
        uv = uv.cpu().numpy()
        assert uv.dtype == np.float32 and np.isfinite(uv).all() and np.abs(uv).max() < 2 ** 20
        Rs.append(R), Ts.append(T), fovs.append(fov), uvs.append(uv), pixels.append(uv.astype(np.int32))
    uvs = np.stack(uvs)
    near = (np.abs(uvs - np.round(uvs)) <= 1e-3).any(axis=-1)
    share = near.mean()
    assert share < 0.01, share                                         # the cap on the points a test may leave out
    np.savez(OUT, xyz=xyz, R=np.stack(Rs), T=np.stack(Ts), FoVx=np.array(fovs), sizes=np.array(SIZES), uv=uvs, pixels=np.stack(pixels))
    inside = [(p[:, 0] >= 0) & (p[:, 0] < W) & (p[:, 1] >= 0) & (p[:, 1] < H) for p, (W, H) in zip(pixels, SIZES)]
    print(f"wrote {OUT}: {uvs.shape}, within 1e-3 of an integer {share:.4%}, inside the image {[float(i.mean().round(3)) for i in inside]}")


if __name__ == "__main__":
    main()
