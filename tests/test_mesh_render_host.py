"""No GPU: csrc/gp_mesh_render.h against the binding's table (a binding outside _lib.ABIS); the programs of csrc/mesh_render_core.h in
a stand-alone build (tests/mesh_render_emulate.cpp, under the sanitizers where the host compiler can link them) against the numpy
restatement tests/mesh_render_ref.py on every case, cull mode and output of tests/mesh_render_cases.py -- bit for bit; a face index
out of range under the sanitizers; the cases against what they are for and against facts that do not come from the restatement
(closed surfaces are covered an even number of times, culling the back faces changes no depth, the order of the faces changes
nothing, the sphere's depth is the analytic ray's); the refusals that need no device."""
import ctypes as C
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import abi_check
import emulate_build
import mesh_render_cases as cases
import mesh_render_ref as ref
import tsdf_cases
from gaussianprediction_amd import _lib, mesh_render as MR
from gaussianprediction_amd.tsdf_ops import Mesh, View

_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "gp_stream_t": _lib.Ptr}
_POINTEES = {"float", "int32_t", "uint8_t", "void"}
F = np.float32
I = np.int32


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the header, the table, the registry ----
def test_prototype_table_equals_the_header_and_stays_out_of_the_registry():
    before = len(_lib.ABIS)
    protos = abi_check.check_table(MR.ABI, 7, _SCALARS, _POINTEES)
    assert MR.ABI.prototypes is MR.PROTOTYPES and MR.ABI not in _lib.ABIS and len(_lib.ABIS) == before
    assert os.path.samefile(os.path.join(abi_check.ROOT, "include", MR.ABI.header), os.path.join(abi_check.ROOT, "gaussianprediction_amd", "csrc", "gp_mesh_render.h"))
    for name in ("gp_mesh_render_rasterize", "gp_mesh_render_resolve", "gp_mesh_render_interpolate", "gp_mesh_render_normals", "gp_mesh_render_shade"):
        assert protos[name][1][-1] == "gp_stream_t"              # the stream is the last parameter
    assert not os.path.exists(os.path.join(abi_check.ROOT, "include", "gp_mesh_render.h"))
    assert len([h for h in os.listdir(os.path.join(abi_check.ROOT, "include")) if h.endswith(".h")]) == 12      # include/ stays at its twelve


def test_symbols_and_constants():
    text = abi_check.header_text(MR.HEADER)
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_MESH_RENDER_[A-Z0-9_]+) +(\d+)", text)}
    assert defs["GP_MESH_RENDER_ABI_VERSION"] == MR.GP_MESH_RENDER_ABI_VERSION == MR.ABI.version == 1
    assert defs["GP_MESH_RENDER_NARROW_MAX"] == MR.NARROW_MAX == ref.NARROW_MAX == 64 and defs["GP_MESH_RENDER_SPLIT"] == MR.SPLIT == ref.SPLIT
    assert defs["GP_MESH_RENDER_MAX_SIZE"] == MR.MAX_SIZE == ref.MAX_SIZE == 16384 and defs["GP_MESH_RENDER_MAX_CHANNELS"] == MR.MAX_CHANNELS == ref.MAX_CHANNELS == 8
    assert defs["GP_MESH_RENDER_SUBPIXEL"] == MR.SUBPIXEL == ref.SUBPIXEL == 256 and defs["GP_MESH_RENDER_GUARD"] == MR.GUARD == ref.GUARD == 2 ** 23
    assert [defs["GP_MESH_RENDER_CULL_" + n.upper()] for n in ("none", "back", "front")] == [MR.CULL[n] for n in ("none", "back", "front")] == [0, 1, 2] and MR.CULL == ref.CULL
    names = ("STATUS", "DRAWN", "NEAR", "OUT_OF_RANGE", "DEGENERATE", "CULLED", "WIDE", "COUNT_WORDS")
    assert [defs["GP_MESH_RENDER_" + n] for n in names] == [MR.STATUS, MR.DRAWN, MR.NEAR, MR.OUT_OF_RANGE, MR.DEGENERATE, MR.CULLED, MR.WIDE, MR.COUNT_WORDS]
    assert [getattr(ref, n) for n in names] == [0, 1, 2, 3, 4, 5, 6, 8] == [getattr(MR, n) for n in names]
    assert MR.STAT_NAMES == tuple(n.lower() for n in names[:7])
    # every edge function stays exact: differences of snapped corners below 2^24, sample offsets below 2^23 + 2^22, two products
    assert 2 * (2 * MR.GUARD) * (MR.GUARD + MR.SUBPIXEL * MR.MAX_SIZE) < 2 ** 51
    abi_check.check_applied(MR.ABI)


# ---- the programs in a stand-alone build, under the sanitizers ----
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    d = tmp_path_factory.mktemp("mesh_render_emulate")
    exe = emulate_build.build("mesh_render_emulate", d, sanitize=True)

    def run(head, arrays, code=0):
        job, out = str(d / "job.bin"), str(d / "out.bin")
        with open(job, "wb") as fp:
            fp.write(head)
            for a in arrays:
                fp.write(np.ascontiguousarray(a).tobytes())
        done = subprocess.run([exe, job, out], timeout=300, stderr=subprocess.PIPE)
        assert done.returncode == code, done.stderr.decode()
        return done.stderr.decode() if code else open(out, "rb").read()

    return run


def job_head(nv, nf, H, W, cull, channels, backwards, z_near, tanfovx, tanfovy):
    return (struct.pack("<8i", nv, nf, H, W, cull, channels, int(backwards), 0)
            + struct.pack("<16f", z_near, tanfovx, tanfovy, cases.AMBIENT, *cases.SHADE_BACKGROUND, 0.0, *cases.BACKGROUND, 0.0, 0.0, 0.0, 0.0))


def emulated(emulator, c, cull="none", backwards=False, faces=None, pictures=True):
    """[counts, coverage, face, depth, valid, bary] (+ [interpolated, normals, nvalid, shaded]) of the stand-alone build."""
    faces = c.faces if faces is None else faces
    H, W, k = c.H, c.W, 4 if pictures else 0
    raw = emulator(job_head(len(c.vertices), len(faces), H, W, ref.CULL[cull], k, backwards, c.z_near, c.view.tanfovx, c.view.tanfovy),
                   [c.view.vm, c.vertices, faces, c.attributes if pictures else np.zeros(0, F)])
    shapes = [(I, (8,)), (I, (H, W)), (I, (H, W)), (F, (H, W)), (np.uint8, (H, W)), (F, (3, H, W))]
    if pictures:
        shapes += [(F, (4, H, W)), (F, (3, H, W)), (np.uint8, (H, W)), (F, (3, H, W))]
    out, at = [], 0
    for dtype, shape in shapes:
        n = int(np.prod(shape))
        out.append(np.frombuffer(raw, dtype, n, at).reshape(shape))
        at += n * np.dtype(dtype).itemsize
    assert at == len(raw)
    return out


@pytest.mark.parametrize("name, cull", cases.RUNS)
def test_the_emulated_programs_against_the_restatement(emulator, name, cull):
    c, want = cases.CASES[name], cases.result(name, cull)
    got = emulated(emulator, c, cull)
    print(name, cull, got[0].tolist())
    for k, (g, w) in enumerate(zip(got, cases.planes(want) + list(cases.pictures(name, cull)))):
        assert same(g, w), (name, cull, k)
    back = emulated(emulator, c, cull, backwards=True, pictures=False)          # the faces in descending order: equal bytes
    assert all(same(g, b) for g, b in zip(got, back))


def test_the_emulator_survives_and_reports_a_face_index_out_of_range(emulator):
    """Under the sanitizers every array has its exact size: an index dereferenced without its check ends the child."""
    c = cases.CASES["bad_index"]
    got = emulated(emulator, c)
    assert got[0].tolist() == [3, 2, 0, 0, 0, 0, 2, 0] and set(np.unique(got[2]).tolist()) <= {-1, 1, 3}       # faces 1 and 3 are one triangle, wound both ways
    assert got[1].max() == 2 and int(got[4].sum()) == int((got[2] >= 0).sum()) == int((got[1] == 2).sum()) > 0
    none = emulated(emulator, cases.CASES["no_vertices"])
    assert none[0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and not none[4].any()


def test_the_emulator_refuses_as_the_library_does(emulator):
    c = cases.CASES["diagonal"]
    arrays = [c.view.vm, c.vertices, c.faces, np.zeros(0, F)]
    for kw, word in ((dict(H=0), "H and W must be > 0"), (dict(W=16385), "<= 16384"), (dict(z_near=0.0), "z_near must be finite and > 0"), (dict(z_near=np.inf), "z_near"),
                     (dict(z_near=np.nan), "z_near"), (dict(cull=3), "cull must be"), (dict(tanfovx=np.inf), "tanfovx and tanfovy must be finite"), (dict(tanfovy=np.nan), "finite")):
        a = dict(nv=4, nf=2, H=48, W=64, cull=0, channels=0, backwards=0, z_near=0.01, tanfovx=0.5, tanfovy=0.375)
        a.update(kw)
        assert word in emulator(job_head(**a), arrays, code=3)


# ---- the cases reach what they are for ----
def test_the_small_cases_reach_what_they_are_for():
    R = cases.result
    # wide: one face, larger than the image, every pixel once, by the wide path
    w = R("wide")
    assert w.counts.tolist() == [0, 1, 0, 0, 0, 0, 1, 0] and (w.coverage == 1).all() and w.valid.all() and (w.face == 0).all()
    rec = w.rec
    assert (np.abs(rec.X) > 256 * 64).any() and (np.abs(rec.Y) > 256 * 48).any() and not rec.out_of_range.any()
    assert np.allclose(w.bary.sum(axis=0), 1, atol=1e-6) and (w.bary > 0).all() and (w.depth > 2).all() and (w.depth < 3).all()
    # diagonal: corners exactly on pixel centres; the quadrilateral's pixels once each; the boundary by ownership: the left and the
    # top edge belong to it, the right and the bottom edge do not
    d = R("diagonal")
    assert (d.rec.X % 256 == 0).all() and (d.rec.Y % 256 == 0).all() and d.rec.X.tolist() == [2560, 7680, 7680, 2560] and d.rec.Y.tolist() == [2560, 2560, 6400, 6400]
    ys, xs = np.nonzero(d.coverage)
    assert d.coverage.max() == 1 and int(d.coverage.sum()) == 20 * 15 and (xs.min(), xs.max() + 1, ys.min(), ys.max() + 1) in ((10, 30, 10, 25), (11, 31, 11, 26), (10, 30, 11, 26), (11, 31, 10, 25))
    assert set(np.unique(d.face).tolist()) == {-1, 0, 1} and (d.face[12, 12:29] >= 0).all()
    on_diagonal = [d.coverage[10 + 3 * k, 10 + 4 * k] for k in range(1, 5)]          # the shared edge passes through these centres exactly
    assert on_diagonal == [1, 1, 1, 1]
    # fan: the hub is a pixel centre shared by seven triangles
    f = R("fan")
    assert (f.rec.X[0], f.rec.Y[0]) == (40 * 256, 30 * 256) and f.coverage[30, 40] == 1 and f.coverage.max() == 1 and f.counts[ref.DRAWN] == 7
    assert len(np.unique(f.face[f.face >= 0])) == 7
    # slivers: between the samples; one snapped to nothing, one collinear
    s = R("slivers")
    assert s.counts.tolist() == [0, 2, 0, 0, 2, 0, 0, 0] and not s.coverage.any() and len({(x, y) for x, y in zip(s.rec.X[6:9], s.rec.Y[6:9])}) == 1
    # ties: face 0 and its copy 1: the smaller id; the coplanar pair overlaps
    t = R("ties")
    both = t.coverage == 2
    assert both.any() and set(np.unique(t.face).tolist()) == {-1, 0, 2, 3} and (t.face[:25][t.coverage[:25] > 0] == 0).all() and (t.coverage[:25][t.face[:25] == 0] == 2).all()
    overlap = both & (np.arange(48)[:, None] >= 25)
    assert overlap.any() and set(np.unique(t.face[overlap]).tolist()) <= {2, 3}
    equal_bits = [p for p in zip(*np.nonzero(overlap)) if _depth_of(cases.CASES["ties"], 2, p) == _depth_of(cases.CASES["ties"], 3, p)]
    assert equal_bits and all(t.face[p] == 2 for p in equal_bits)          # equal depth bits: the smaller id, whichever comes first
    # near: a corner at z_near exactly, a face behind the camera
    n = R("near")
    assert n.counts.tolist() == [0, 1, 2, 0, 0, 0, 1, 0] and n.rec.near.tolist() == [False, False, True, True, True, True, False, False, False]
    assert set(np.unique(n.face).tolist()) == {-1, 2}
    # guard: 40000 pixels are beyond 2^23 sub-pixels, 32767 are not
    g = R("guard")
    assert g.counts.tolist() == [0, 1, 0, 1, 0, 0, 1, 0] and g.rec.out_of_range.tolist() == [False, True, False, False, False, False] and g.rec.X[4] == 32767 * 256 <= ref.GUARD
    assert set(np.unique(g.face).tolist()) == {-1, 1} and g.face[:, 63].max() == 1          # clamped at the right border
    # threshold: boxes of 8 x 8 = NARROW_MAX and 13 x 5 = NARROW_MAX + 1 pixels
    h = R("threshold")
    assert h.counts.tolist() == [0, 2, 0, 0, 0, 0, 1, 0] and h.rec.X.tolist() == [2560, 4352, 2560, 7680, 10752, 7680] and h.rec.Y.tolist() == [1280, 1280, 3072, 7680, 7680, 8704]
    assert (h.face == 0).any() and (h.face == 1).any()
    # bad indices; nothing to draw
    assert R("bad_index").counts.tolist() == [3, 2, 0, 0, 0, 0, 2, 0] and R("bad_index").valid.any()
    for name in ("no_faces", "nothing", "no_vertices"):
        e = R(name)
        assert not e.valid.any() and (e.face == -1).all() and not e.depth.any() and not e.bary.any() and not e.coverage.any() and e.counts[1:].tolist() == [0] * 7
    r = cases.CASES["random"]
    assert (r.W, r.H, len(r.faces)) == (70, 50, 300) and r.culls == ("none", "back", "front")
    for cull in r.culls:
        k = R("random", cull).counts
        assert k[ref.WIDE] > 5 and k[ref.DRAWN] - k[ref.WIDE] > 100 and k[ref.NEAR] == 9 and k[ref.DEGENERATE] == 8 and k.sum() - k[ref.WIDE] == 300
    assert R("random", "back").counts[ref.CULLED] + R("random", "front").counts[ref.CULLED] == R("random").counts[ref.DRAWN]


def _depth_of(c, f, p):
    """The depth bits of face f alone at pixel p = (y, x), or None."""
    r = ref.rasterize(c.vertices, c.faces[f:f + 1], c.view, c.W, c.H, c.z_near)
    return r.depth[p].tobytes() if r.valid[p] else None


# ---- facts that do not come from the restatement ----
@pytest.mark.parametrize("name", cases.CLOSED)
def test_closed_surfaces(name):
    c = cases.CASES[name]
    none, back, front = (cases.result(name, cull) for cull in ("none", "back", "front"))
    values = set(np.unique(none.coverage).tolist())
    print(name, sorted(values), int(none.valid.sum()))
    assert all(v % 2 == 0 for v in values) and none.valid.any()                 # every ray that enters leaves
    if not name.startswith("torus"):
        assert values == {0, 2}
    assert same(back.depth, none.depth) and same(back.valid, none.valid)        # the nearest surface faces the camera
    assert same(front.valid, none.valid) and (front.depth[none.valid != 0] > none.depth[none.valid != 0]).all()
    assert same(back.coverage + front.coverage, none.coverage)
    # the order of the faces: any permutation gives the same depth, byte for byte
    order = np.random.default_rng(5).permutation(len(c.faces))
    mixed = ref.rasterize(c.vertices, c.faces[order], c.view, c.W, c.H, c.z_near)
    assert same(mixed.depth, none.depth) and same(mixed.coverage, none.coverage) and same(order[mixed.face[mixed.valid != 0]].astype(I), none.face[none.valid != 0])


def test_the_order_of_the_faces_on_the_emulator(emulator):
    c = cases.CASES["sphere_0"]
    order = np.random.default_rng(6).permutation(len(c.faces))
    got = emulated(emulator, c, faces=c.faces[order], pictures=False)
    want = cases.result("sphere_0")
    assert same(got[3], want.depth) and same(got[1], want.coverage) and same(got[4], want.valid)


def analytic_sphere(c):
    """(hit [H, W] bool, depth [H, W] float64, cosine [H, W] float64) of the rays of the case's pixels against tsdf_cases.SPHERE."""
    m = np.asarray(c.view.vm, np.float64).reshape(4, 4).T
    R, t = m[:3, :3], m[:3, 3]
    eye = -R.T @ t
    ys, xs = np.meshgrid(np.arange(c.H), np.arange(c.W), indexing="ij")
    d = np.stack([((2 * xs + 1) / c.W - 1) * c.view.tanfovx, ((2 * ys + 1) / c.H - 1) * c.view.tanfovy, np.ones_like(xs, dtype=np.float64)], axis=-1) @ R      # world; depth = t
    o = eye - np.asarray(tsdf_cases.SPHERE.c)
    a, b, k = (d * d).sum(-1), 2 * (d @ o), o @ o - tsdf_cases.SPHERE.r ** 2
    disc = b * b - 4 * a * k
    hit = disc >= 0
    depth = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0))) / (2 * a), np.nan)
    normal = (o + depth[..., None] * d) / tsdf_cases.SPHERE.r
    cosine = np.abs((normal * d).sum(-1)) / np.sqrt(a)
    return hit & (depth > 0), depth, cosine


@pytest.mark.parametrize("k", range(3))
def test_the_sphere_against_its_analytic_rays(k):
    c, r = cases.CASES[f"sphere_{k}"], cases.result(f"sphere_{k}")
    hit, depth, cosine = analytic_sphere(c)
    chosen = hit & (cosine >= 0.5)
    covered = r.valid != 0
    voxel = tsdf_cases.EXTRACT["33_sphere"][0].voxel
    error = np.abs(r.depth.astype(np.float64) - depth)[chosen]
    print(k, int(chosen.sum()), int(covered.sum()), int(hit.sum()), float(error.max()), 2 * np.sqrt(3) * voxel)
    assert chosen.sum() > 100 and covered[chosen].all()
    assert not (covered & ~hit).any()
    assert error.max() <= 2 * np.sqrt(3) * voxel


# ---- the refusals that need no device ----
def test_refusals_before_any_pointer_is_looked_at():
    l = MR.lib()

    def refused(rc, word):
        assert rc == 1 and word in l.gp_last_error(), (word, l.gp_last_error())

    def raster(nv=4, nf=2, H=48, W=64, tx=0.5, ty=0.375, z_near=0.01, cull=0, vertices=16, faces=16, vm=16, scratch=16, coverage=None, counts=16):
        return l.gp_mesh_render_rasterize(vertices, faces, nv, nf, vm, tx, ty, H, W, z_near, cull, scratch, coverage, counts, None)

    nan, inf = float("nan"), float("inf")
    sizes = ((dict(nv=2 ** 31), b"nv must be below 2^31"), (dict(nf=715827883), b"3*nf must be below 2^31"), (dict(nv=-1), b">= 0"), (dict(nf=-1), b">= 0"),
             (dict(H=0), b"H and W must be > 0"), (dict(W=-3), b"H and W must be > 0"), (dict(H=16385), b"<= 16384"), (dict(W=16385), b"<= 16384"))
    for kw, word in sizes:
        a = dict(nv=4, nf=2, H=48, W=64)
        a.update(kw)
        assert l.gp_mesh_render_scratch_bytes(a["nv"], a["nf"], a["H"], a["W"]) == -1 and word in l.gp_last_error()
        refused(raster(**kw), word)
        refused(l.gp_mesh_render_resolve(16, a["nv"], a["nf"], a["H"], a["W"], 16, 16, 16, 16, 16, None), word)
        refused(l.gp_mesh_render_interpolate(16, 3, 16, a["nv"], a["nf"], a["H"], a["W"], 16, 16, 16, 16, 16, 16, None), word)
        refused(l.gp_mesh_render_normals(16, 16, a["nv"], a["nf"], 16, 0.5, 0.5, a["H"], a["W"], 16, 16, 16, 16, 16, None), word)
    refused(l.gp_mesh_render_shade(16, 16, 16, 16, 0.5, 0.5, 0, 64, 0.3, 0, 0, 0, 16, None), b"H and W must be > 0")
    assert l.gp_mesh_render_scratch_bytes(0, 0, 1, 1) > 0 and l.gp_mesh_render_scratch_bytes(10 ** 6, 2 * 10 ** 6, 800, 800) >= 16 * 10 ** 6 + 8 * 640000 + 8 * 10 ** 6
    for kw, word in ((dict(scratch=None), b"null"), (dict(scratch=8), b"16-byte aligned"), (dict(counts=None), b"null"), (dict(vm=None), b"null"), (dict(vertices=None), b"null"),
                     (dict(faces=None), b"null"), (dict(tx=inf), b"tanfovx and tanfovy must be finite"), (dict(ty=nan), b"tanfovx and tanfovy must be finite"),
                     (dict(z_near=0.0), b"z_near must be finite and > 0"), (dict(z_near=-1.0), b"z_near"), (dict(z_near=nan), b"z_near"), (dict(z_near=inf), b"z_near"),
                     (dict(cull=3), b"cull must be"), (dict(cull=-1), b"cull must be")):
        refused(raster(**kw), word)
    for args, word in (((None, 4, 2, 48, 64, 16, 16, 16, 16, 16), b"null"), ((16, 4, 2, 48, 64, None, 16, 16, 16, 16), b"null"), ((16, 4, 2, 48, 64, 24, 16, 16, 16, 16), b"aligned"),
                       ((16, 4, 2, 48, 64, 16, None, 16, 16, 16), b"null"), ((16, 4, 2, 48, 64, 16, 16, None, 16, 16), b"null"), ((16, 4, 2, 48, 64, 16, 16, 16, None, 16), b"null"),
                       ((16, 4, 2, 48, 64, 16, 16, 16, 16, None), b"null")):
        refused(l.gp_mesh_render_resolve(*args, None), word)
    for args, word in (((16, 0, 16, 4, 2, 48, 64, 16, 16, 16, 16, 16, 16), b"C must be 1 .. 8"), ((16, 9, 16, 4, 2, 48, 64, 16, 16, 16, 16, 16, 16), b"C must be 1 .. 8"),
                       ((None, 3, 16, 4, 2, 48, 64, 16, 16, 16, 16, 16, 16), b"null"), ((16, 3, 16, 4, 2, 48, 64, None, 16, 16, 16, 16, 16), b"null"),
                       ((16, 3, 16, 4, 2, 48, 64, 8, 16, 16, 16, 16, 16), b"aligned"), ((16, 3, 16, 4, 2, 48, 64, 16, 16, 16, 16, None, 16), b"null"),
                       ((16, 3, 16, 4, 2, 48, 64, 16, 16, 16, 16, 16, None), b"null")):
        refused(l.gp_mesh_render_interpolate(*args, None), word)
    for args, word in (((16, 16, 4, 2, None, 0.5, 0.5, 48, 64, 16, 16, 16, 16, 16), b"null"), ((16, 16, 4, 2, 16, inf, 0.5, 48, 64, 16, 16, 16, 16, 16), b"finite"),
                       ((16, 16, 4, 2, 16, 0.5, 0.5, 48, 64, 16, 16, 16, None, 16), b"null")):
        refused(l.gp_mesh_render_normals(*args, None), word)
    for args, word in (((None, 16, 16, 16, 0.5, 0.5, 48, 64, 0.3, 0, 0, 0, 16), b"null"), ((16, 16, 16, 16, 0.5, nan, 48, 64, 0.3, 0, 0, 0, 16), b"finite"),
                       ((16, 16, 16, 16, 0.5, 0.5, 48, 64, nan, 0, 0, 0, 16), b"ambient must be finite"), ((16, 16, 16, 16, 0.5, 0.5, 48, 64, 0.3, 0, 0, 0, None), b"null")):
        refused(l.gp_mesh_render_shade(*args, None), word)


def test_the_python_surface_refuses_before_the_device(monkeypatch):
    monkeypatch.setattr(MR, "lib", lambda: pytest.fail("a launch was reached"))
    faces, vertices = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, 3)
    view = View(torch.eye(4), 0.5, 0.375)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MR.rasterize(Mesh(vertices, faces, None), view, size=(48, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MR.render_mesh(Mesh(vertices, faces, None), view, size=(48, 64))
    for call, word in ((lambda: MR.rasterize(Mesh(vertices, faces.long(), None), view, size=(48, 64)), "int32"),
                       (lambda: MR.rasterize(Mesh(vertices[0], faces, None), view, size=(48, 64)), r"\[Nv, 3\]"),
                       (lambda: MR.render_mesh(Mesh(vertices, faces, None), view, mode="wire"), "mode = 'wire'"),
                       (lambda: MR.render_mesh(Mesh(vertices, faces, None), view, near=1.0), "options of mode 'depth'"),
                       (lambda: MR.interpolate(None, vertices), "MeshRaster"), (lambda: MR.agreement(None, None), "MeshRaster")):
        with pytest.raises(RuntimeError, match=word):
            call()
    for call, word in ((lambda: MR.rasterize(Mesh(vertices, faces, None), view, z_near=0.0), "z_near must be finite and > 0"),
                       (lambda: MR.rasterize(Mesh(vertices, faces, None), view, z_near=float("nan")), "z_near"),
                       (lambda: MR.rasterize(Mesh(vertices, faces, None), view, cull="both"), "cull must be")):
        with pytest.raises(_lib.GpHipError, match=word):
            call()
    assert MR.check_size(48, 64) is None and MR.check_size(16384, 1) is None and "16384" in MR.check_size(16385, 1) and "> 0" in MR.check_size(0, 5)


def test_signatures_and_docstrings():
    from gaussianprediction_amd import eval_render as ER
    sig = inspect.signature(MR.rasterize)
    assert list(sig.parameters)[:5] == ["mesh", "view", "z_near", "cull", "counts"] and [p.default for p in sig.parameters.values()][2:5] == [0.01, "none", False]
    assert list(inspect.signature(MR.interpolate).parameters) == ["raster", "attributes", "background"] and inspect.signature(MR.interpolate).parameters["background"].default == 0
    assert list(inspect.signature(MR.normals).parameters)[:3] == ["raster", "mesh", "view"]
    sig = inspect.signature(MR.shade)
    assert list(sig.parameters)[:6] == ["color", "normals", "raster", "view", "ambient", "background"] and sig.parameters["ambient"].default == 0.3 and sig.parameters["background"].default == (0, 0, 0)
    sig = inspect.signature(MR.render_mesh)
    assert list(sig.parameters)[:4] == ["mesh", "view", "mode", "background"] and sig.parameters["mode"].default == "shaded" and MR.MODES == ("shaded", "color", "normals", "depth")
    assert list(inspect.signature(MR.agreement).parameters) == ["raster", "depth_result"]
    sig = inspect.signature(ER.render_mesh_views)
    names = list(sig.parameters)
    assert names[:7] == ["model_path", "name", "iteration", "views", "gaussians", "pipeline", "background"] and names[7:12] == ["meshes", "mode", "compare", "writer", "video"]
    assert [sig.parameters[k].default for k in names[7:12]] == [None, "shaded", False, None, False] and sig.parameters[names[-1]].kind is inspect.Parameter.VAR_KEYWORD
    assert open(ER.__file__).read().count("render_meshes(") == 1            # render_meshes itself is left alone
    assert "ONE read" in MR.MeshRaster.__doc__ and "Nothing is read" in MR.rasterize.__doc__ and "One read" in MR.agreement.__doc__
