"""Seeded cases of the signed-distance volumes, shared by the host test (the stand-alone build of csrc/volume_core.h) and the GPU test
(volume_ops).  Small on purpose; each names what it can break.  A case of CASES is (vertices, faces, queries).

  surface/*, sdf/*        every case of surface_cases.CASES and of sdf_cases.CASES
  nf_0 .. nf_257          nf of 0, 1, 3, 4, 5, 63, 65, 257: leaf and level boundaries of the tree
  nq_1 .. nq_257          nq of 1, 63, 65, 257 on the cube: wave and workgroup boundaries
  unusable                every face has a bad index or a NaN corner: every box is empty
  same_faces              40 identical faces: every box is equal, every query ties, the smallest face number wins
  deep_sphere, deep_torus the centre, 64 points within half a radius of it, points on the torus's axis, points 3, 30 and 1000 extents
                          away along each axis and the diagonal, NaN and inf queries -- where the grid walks ring after empty ring
  sparse                  two small clusters at opposite corners of a long box: most of the tree's boxes are far from any query
  planar                  a flat sheet: every box has no extent along z
  far                     a mesh with coordinates near 10^6: the 2^-47 * M term of the bound matters

LATTICES: name -> (vertices, faces, origin, voxel, dims), dims of (1, 1, 1), (63, 1, 1), (65, 1, 1), (257, 1, 1) and (5, 4, 3) around
the cube and the flat tetrahedron, with voxels and origins that are no dyadic fractions; COMPARES: pairs of volumes of 1, 63, 65 and
257 values with inf, NaN and 0 entries; IOU and REMESH: the two end-to-end cases.

At import, on the CPU, the module asserts what the tests rest on (see the end of the file)."""
import functools
from types import SimpleNamespace

import numpy as np

import geometry_cases
import sdf_cases
import sdf_ref
import surface_cases
import surface_ref
import tsdf_cases
import volume_ref as ref

F = np.float32
I = np.int32
same = surface_cases.same
LEAVES = (1, 2, 4, 8)
CUBE_V, CUBE_F = sdf_cases.CUBE_V, sdf_cases.CUBE_F
TET_V, TET_F = sdf_cases.CASES["flat_tet"][0], sdf_cases.CASES["flat_tet"][1]


def _deep(name, centre, radius, rng):
    v, f = geometry_cases.MESHES[name]
    c = np.asarray(centre, np.float64)
    ext = float((v.max(axis=0).astype(np.float64) - v.min(axis=0)).max())
    ball = rng.normal(size=(64, 3))
    ball = c + ball / np.linalg.norm(ball, axis=1, keepdims=True) * (0.5 * radius * rng.uniform(0, 1, (64, 1)) ** (1 / 3))
    axis = c + np.array([[0, 0, z] for z in (-2.0, -0.5, -0.1, 0.0, 0.1, 0.5, 2.0)])
    away = np.array([c + np.array(d, np.float64) * (s * k * ext) for k in (3, 30, 1000) for s in (1, -1) for d in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1))])
    bad = rng.uniform(-1, 1, (6, 3))
    bad[0, 0], bad[1, 2], bad[2, 1], bad[3] = np.nan, np.inf, -np.inf, np.nan
    return v, f, np.concatenate([c[None], ball, axis, away, bad]).astype(F)


def _cases():
    C = {}
    rng = np.random.default_rng(34)
    for name, case in surface_cases.CASES.items():
        C["surface/" + name] = case
    for name, case in sdf_cases.CASES.items():
        C["sdf/" + name] = case
    for nf in (0, 1, 3, 4, 5, 63, 65, 257):
        v = rng.uniform(-1, 1, (nf + 2, 3)).astype(F)
        C[f"nf_{nf}"] = (v, np.stack([np.arange(nf), np.arange(nf) + 1, np.arange(nf) + 2], axis=1).astype(I), rng.uniform(-1.5, 1.5, (40, 3)).astype(F))
    for nq in (1, 63, 65, 257):
        C[f"nq_{nq}"] = (CUBE_V, CUBE_F, rng.uniform(-0.5, 1.5, (nq, 3)).astype(F))
    v = rng.uniform(-1, 1, (12, 3)).astype(F)
    v[::3, 1] = np.nan
    f = np.stack([np.arange(10), np.arange(10) + 1, np.arange(10) + 2], axis=1).astype(I)
    f[1::3, 2] = 99
    f[4, 0] = -1
    C["unusable"] = (v, f, rng.uniform(-1, 1, (20, 3)).astype(F))
    tri = surface_cases.CASES["triangle"][0]
    C["same_faces"] = (tri, np.tile(np.array([[0, 1, 2]], I), (40, 1)), surface_cases.CASES["triangle"][2])
    C["deep_sphere"] = _deep("33_sphere", tsdf_cases.SPHERE.c, tsdf_cases.SPHERE.r, rng)
    C["deep_torus"] = _deep("33_torus", tsdf_cases.TORUS.c, tsdf_cases.TORUS.R, rng)
    a, b = rng.uniform(0, 0.01, (60, 3)), rng.uniform(0, 0.01, (60, 3)) + np.array([100.0, 1.0, 1.0])
    v = np.concatenate([a, b]).astype(F)
    f = np.concatenate([rng.integers(0, 60, (50, 3)), rng.integers(60, 120, (50, 3))]).astype(I)
    q = np.concatenate([rng.uniform([-1, -1, -1], [101, 2, 2], (60, 3)), a[:5] + 0.02, b[:5] - 0.02, np.array([[50.0, 0.5, 0.5]])]).astype(F)
    C["sparse"] = (v, f, q)
    n = 9
    gx, gy = np.meshgrid(np.arange(n), np.arange(n), indexing="xy")
    v = np.stack([gx.reshape(-1) * 0.25, gy.reshape(-1) * 0.25, np.full(n * n, 0.5)], axis=1).astype(F)
    at = (gy[:-1, :-1] * n + gx[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([at, at + 1, at + n], axis=1), np.stack([at + 1, at + n + 1, at + n], axis=1)]).astype(I)
    C["planar"] = (v, f, np.concatenate([rng.uniform(-1, 3, (60, 3)), np.array([[1.0, 1.0, 0.5], [0.3, 0.7, 0.5], [5, 5, 0.5], [1, 1, 100]])]).astype(F))
    v, f, q = surface_cases.CASES["far_origin"]
    ok = np.isfinite(v).all(axis=1)
    c = v[ok].mean(axis=0).astype(np.float64)
    C["far"] = (v, f, np.concatenate([q, (c + rng.normal(size=(30, 3)) * 30.0).astype(F), (c + np.array([[1e4, 0, 0], [0, -1e5, 0], [3e6, 3e6, 3e6]])).astype(F),
                                      np.zeros((1, 3), F)]))
    return {k: tuple(np.ascontiguousarray(a) for a in c) for k, c in C.items()}


CASES = _cases()
DEEP = ("deep_sphere", "deep_torus")


def _lattices():
    L = {}
    for mesh, (v, f), z in (("cube", (CUBE_V, CUBE_F), 0.45), ("tet", (TET_V, TET_F), 0.02)):
        L[f"{mesh}_1"] = (v, f, (F(0.3), F(0.3), F(z)), F(0.1), (1, 1, 1))
        for n in (63, 65, 257):
            L[f"{mesh}_{n}"] = (v, f, (F(-0.7), F(0.3), F(z)), F(0.01), (n, 1, 1))
        L[f"{mesh}_543"] = (v, f, (F(-0.13), F(0.21), F(z) - F(0.3)), F(0.3), (5, 4, 3))
    L["cube_tenths"] = (CUBE_V, CUBE_F, (F(-0.45),) * 3, F(0.1), (7, 6, 16))
    return L


LATTICES = _lattices()
NO_UNSTABLE = tuple(k for k in LATTICES if k.startswith("cube"))


def _compares():
    rng = np.random.default_rng(35)
    out = {}
    for n in (1, 63, 65, 257):
        a, b = rng.normal(size=n).astype(F), rng.normal(size=n).astype(F)
        a[::7], b[3::11], a[5::13], b[1::5], a[2::17] = np.inf, -np.inf, 0.0, -0.0, np.nan
        out[n] = (a, b)
    return out


COMPARES = _compares()

# the IoU case: the unit cube against itself moved 0.5 along x
IOU = SimpleNamespace(a=(CUBE_V, CUBE_F), b=((CUBE_V + np.array([0.5, 0, 0], F)).astype(F), CUBE_F), origin=(F(-0.45),) * 3, voxel=F(0.1), dims=(21, 16, 16),
                      counts=(1000, 1000, 500, 1500, 0))
# the remesh case: the unit cube on the lattice lattice_for chooses for voxel 0.07f, and on an explicit one
REMESH = SimpleNamespace(mesh=(CUBE_V, CUBE_F), voxel=F(0.07), explicit=((F(-0.31),) * 3, F(0.07), (24, 24, 24)))


@functools.lru_cache(maxsize=None)
def result(name):
    """surface_ref.point_mesh of a case (the brute force, no tree); do not modify."""
    if name.startswith("surface/"):
        return surface_cases.result(name[8:])
    if name.startswith("sdf/"):
        return sdf_cases.result(name[4:]).surface
    v, f, q = CASES[name]
    return surface_ref.point_mesh(q, v, f)


@functools.lru_cache(maxsize=None)
def signed(name):
    """volume_ref.signed of a case: the restated sign pass on the restated row; do not modify."""
    if name.startswith("sdf/"):
        return sdf_cases.result(name[4:])
    v, f, q = CASES[name]
    return ref.signed(q, v, f, result(name))


@functools.lru_cache(maxsize=None)
def lattice(name):
    """volume_ref.lattice of a lattice case; do not modify."""
    v, f, origin, voxel, dims = LATTICES[name]
    return ref.lattice(v, f, origin, voxel, dims)


def equal_result(got, want):
    return surface_cases.equal_result(got, want)


def compare_sdf(got_sdf, want):
    """sdf_cases.compare's rule for sign and sdf rows: exact on every row the restatement does not mark unstable, |sdf| exact everywhere."""
    got_sdf, s = np.asarray(got_sdf, F).reshape(-1), want.signed
    stable = ~s.unstable
    assert same(got_sdf[stable], s.sdf[stable]), np.nonzero(got_sdf != s.sdf)[0][:8]
    assert same(np.abs(got_sdf), np.abs(s.sdf))


# ---- the stand-alone build of csrc/volume_core.h, as a child process ----
def build_emulator(d, sanitize):
    """tests/volume_emulate.cpp built into `d` (a pathlib directory), under the sanitizers where `sanitize` is set; returns
    run(vertices, faces, queries, ...) -> SimpleNamespace(dist2, face, region, closest, bary, stats[, sdf, lattice_stats], counts), one
    run of the child."""
    import struct
    import subprocess

    import emulate_build
    exe = emulate_build.build("volume_emulate", d, sanitize=sanitize)

    def run(vertices, faces, queries, leaf=ref.LEAF, tables=None, lattice=None, pair=None, code=0, sizes=None):
        nv, nf, nq = len(vertices), len(faces), len(queries)
        ne = len(tables.edge_normal) if tables is not None else 0
        origin, voxel, dims = lattice if lattice is not None else ((0.0, 0.0, 0.0), 0.0, (0, 0, 0))
        a, b = pair if pair is not None else (np.zeros(0, F), np.zeros(0, F))
        head = list(sizes) if sizes else [nv, nf, ne, nq, leaf, dims[0], dims[1], dims[2], len(a)]
        job, out = str(d / "job.bin"), str(d / "out.bin")
        with open(job, "wb") as fp:
            fp.write(struct.pack("<12i", *head, 0, 0, 0) + struct.pack("<4f", *[float(x) for x in origin], float(voxel)))
            for arr, dtype in ((vertices, F), (faces, I), (queries, F)):
                fp.write(np.ascontiguousarray(arr, dtype).tobytes())
            if tables is not None:
                fp.write(np.ascontiguousarray(tables.face_edges, I).tobytes() + np.ascontiguousarray(tables.edge_normal, np.float64).tobytes() +
                         np.ascontiguousarray(tables.vertex_normal, np.float64).tobytes())
            else:
                fp.write(np.full((nf, 3), -1, I).tobytes() + np.zeros((nv, 3), np.float64).tobytes())
            fp.write(np.ascontiguousarray(a, F).tobytes() + np.ascontiguousarray(b, F).tobytes())
        done = subprocess.run([exe, job, out], timeout=300, stderr=subprocess.PIPE)
        assert done.returncode == code, done.stderr.decode()
        if code:
            return done.stderr.decode()
        n = int(np.prod(dims))
        layout = [("dist2", F, (nq,)), ("face", I, (nq,)), ("region", I, (nq,)), ("closest", F, (nq, 3)), ("bary", F, (nq, 2)), ("stats", np.int64, (ref.STAT_WORDS,))]
        if n:
            layout += [("sdf", F, (dims[2], dims[1], dims[0])), ("lattice_stats", np.int64, (ref.LATTICE_WORDS,))]
        layout += [("counts", np.int64, (ref.COUNT_WORDS,))]
        raw, got, at = open(out, "rb").read(), SimpleNamespace(), 0
        for key, dtype, shape in layout:
            k = int(np.prod(shape))
            setattr(got, key, np.frombuffer(raw, dtype, k, at).reshape(shape))
            at += k * np.dtype(dtype).itemsize
        assert at == len(raw)
        got.row = (got.dist2, got.face, got.region, got.closest, got.bary)
        return got

    return SimpleNamespace(run=run)


# ---- what the tests rest on, asserted on the CPU at import ----
def _conditions():
    for name in LATTICES:
        s = lattice(name).signed
        left = int(s.unstable.sum())
        assert left <= sdf_cases.UNSTABLE_CAP * len(s.sign) and (left == 0 or name not in NO_UNSTABLE), (name, left)
    # the IoU case: no lattice point within 0.01 of either surface; the restated counts
    a = ref.lattice(*IOU.a, IOU.origin, IOU.voxel, IOU.dims)
    b = ref.lattice(*IOU.b, IOU.origin, IOU.voxel, IOU.dims)
    assert min(np.abs(a.sdf).min(), np.abs(b.sdf).min()) > 0.01 and not a.signed.unstable.any() and not b.signed.unstable.any()
    assert tuple(ref.compare(a.sdf, b.sdf)[:5].tolist()) == IOU.counts
    origin, voxel, dims = ref.lattice_for(np.concatenate([IOU.a[0], IOU.b[0]]), IOU.voxel)          # the lattice volume_iou itself chooses: the same counts
    a, b = ref.lattice(*IOU.a, origin, voxel, dims), ref.lattice(*IOU.b, origin, voxel, dims)
    assert min(np.abs(a.sdf).min(), np.abs(b.sdf).min()) > 0.01 and tuple(ref.compare(a.sdf, b.sdf)[:5].tolist()) == IOU.counts
    # the remesh case: no lattice point has |sdf| < 10^-3, on either lattice
    for origin, voxel, dims in (ref.lattice_for(REMESH.mesh[0], REMESH.voxel), REMESH.explicit):
        r = ref.lattice(*REMESH.mesh, origin, voxel, dims)
        assert np.abs(r.sdf).min() >= 1e-3 and not r.signed.unstable.any() and (r.sdf < 0).any(), (origin, dims)


_conditions()
