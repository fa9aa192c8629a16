"""Build-container script (needs the reference tree; NOT run on the GPU box): records the reference's own `lerp` / `slerp`
[REF utils/camera_utils.py:20-70] on numpy quaternions -- the branch that needs no device -- for 8 pairs at 4 ratios.  The two functions
are compiled from their `ast` nodes alone: the module's top-level imports need CUDA-only packages.  Writes
tests/golden/pose_interpolation.npz (data: inputs and recorded results); tests/test_png_host.py holds eval_render.slerp and
interpolation_pose against it.

    python tests/golden/make_pose_vectors.py [/path/to/reference]
"""
import ast
import os
import sys

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pose_interpolation.npz")
RATIOS = np.array([0.2, 0.5, 0.8, 1.0])


def reference_functions():
    path = os.path.join(REF, "utils", "camera_utils.py")
    tree = ast.parse(open(path).read(), path)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("lerp", "slerp")]
    assert [n.name for n in keep] == ["lerp", "slerp"]
    scope = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), scope)
    return scope["slerp"]


def pairs():
    """([8, 2, 4] float64 (w, x, y, z), canonical [8] bool): unit quaternions of random rotations, then the cases slerp branches on.
    canonical: both members have norm one and w >= 0, so they survive the round trip through a rotation matrix (interpolation_pose)."""
    rng = np.random.default_rng(20)

    def unit(v):
        return v / np.linalg.norm(v)

    def canonical_pair(accept):
        while True:
            a, b = unit(rng.normal(size=4)), unit(rng.normal(size=4))
            a, b = a * np.sign(a[0]), b * np.sign(b[0])
            if accept(np.sum(a * b)):
                return a, b

    q = rng.normal(size=(8, 2, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    q[1, 1] = q[1, 0] + 1e-3 * rng.normal(size=4)              # |dot| > 0.9995: the lerp branch, of inputs that are not normalised
    q[2, 1] = -q[2, 0] + 1e-3 * rng.normal(size=4)             # dot < -0.9995: the lerp branch through the origin (no shortest-arc flip)
    q[3] = canonical_pair(lambda d: -0.9 < d < -0.2)           # a negative dot below the threshold: the long way round
    q[4] *= np.array([[1.7], [0.6]])                           # norms other than one: the weights multiply the inputs as given
    q[5] = canonical_pair(lambda d: 0.2 < d < 0.9)
    a = unit(np.abs(rng.normal(size=4)) + 0.3)
    q[6] = a, unit(a + 1e-3 * rng.normal(size=4))              # the lerp branch between two unit quaternions
    q[7] = canonical_pair(lambda d: abs(d) < 0.2)
    canonical = np.array([bool(np.all(np.abs(np.linalg.norm(p, axis=-1) - 1) < 1e-15) and np.all(p[:, 0] > 0.05)) for p in q])
    return q, canonical


def main():
    slerp = reference_functions()
    q, canonical = pairs()
    out = np.zeros((len(q), len(RATIOS), 4))
    for i, (q0, q1) in enumerate(q):
        for j, t in enumerate(RATIOS):
            out[i, j] = slerp(float(t), q0.copy(), q1.copy())
    dots = np.array([np.sum(a / np.linalg.norm(a) * b / np.linalg.norm(b)) for a, b in q])
    assert (np.abs(dots) > 0.9995).any() and ((dots < 0) & (np.abs(dots) <= 0.9995)).any()
    assert canonical[[3, 5, 6, 7]].all()
    np.savez(OUT, pairs=q, ratios=RATIOS, slerp=out, dots=dots, canonical=canonical)
    print(f"wrote {OUT}: {out.shape}, dots {np.round(dots, 4)}")


if __name__ == "__main__":
    main()
