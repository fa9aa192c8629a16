"""No GPU: csrc/gp_tsdf.h against the binding's table (a binding outside _lib.ABIS); the programs of csrc/tsdf_core.h in a stand-alone
build (tests/tsdf_emulate.cpp, under the sanitizers where the host compiler can link them) against the numpy restatement
tests/tsdf_ref.py on every case of tests/tsdf_cases.py -- bit for bit for tsdf, weight, color, counts, vertices, colors and faces; the
restatement against the facts of closed surfaces (a sphere, an ellipsoid-like surface, a torus) and against an analytic plane; the
header's sixteen rows against the rule; the mesh PLY files; the refusals that need no device."""
import ctypes as C
import inspect
import os
import re
import struct
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import abi_check
import emulate_build
import tsdf_cases as cases
import tsdf_ref as ref
from gaussianprediction_amd import _lib, io_formats, tsdf_ops as TO

_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "gp_stream_t": _lib.Ptr}
_POINTEES = {"float", "uint8_t", "int32_t", "void"}
F = np.float32


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the header, the table, the registry ----
def test_prototype_table_equals_the_header_and_stays_out_of_the_registry():
    before = len(_lib.ABIS)
    protos = abi_check.check_table(TO.ABI, 5, _SCALARS, _POINTEES, {"gp_tsdf_volume": TO.TsdfVolumeC, "gp_tsdf_view": TO.TsdfViewC})
    assert TO.ABI.prototypes is TO.PROTOTYPES and TO.ABI not in _lib.ABIS and len(_lib.ABIS) == before
    assert os.path.samefile(os.path.join(abi_check.ROOT, "include", TO.ABI.header),
                            os.path.join(abi_check.ROOT, "gaussianprediction_amd", "csrc", "gp_tsdf.h"))
    for name in ("gp_tsdf_integrate", "gp_tsdf_extract_count", "gp_tsdf_extract_fill"):
        assert protos[name][1][-1] == "gp_stream_t"              # the stream is the last parameter
    assert not os.path.exists(os.path.join(abi_check.ROOT, "include", "gp_tsdf.h"))
    assert len([h for h in os.listdir(os.path.join(abi_check.ROOT, "include")) if h.endswith(".h")]) == 12      # include/ stays at its twelve


def test_symbols_constants_and_the_structs():
    text = abi_check.header_text(TO.HEADER)
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_TSDF_[A-Z0-9_]+) +(\d+)", text)}
    assert defs["GP_TSDF_ABI_VERSION"] == TO.GP_TSDF_ABI_VERSION == TO.ABI.version == 1
    assert (defs["GP_TSDF_MAX_VIEWS"], defs["GP_TSDF_TILE"], defs["GP_TSDF_EDGES"]) == (TO.MAX_VIEWS, TO.TILE, TO.EDGES) == (16, 1024, 7)
    assert (ref.MAX_VIEWS, ref.TILE, len(ref.EDGE_BITS)) == (16, 1024, 7)
    abi_check.check_applied(TO.ABI)
    for cname, cls, size in (("gp_tsdf_volume", TO.TsdfVolumeC, 56), ("gp_tsdf_view", TO.TsdfViewC, 16)):
        fields = re.search(r"typedef struct %s \{(.*?)\}" % cname, text, flags=re.S).group(1)
        assert re.findall(r"(\w+)\s*[,;]", fields) == [n for n, _ in cls._fields_] and C.sizeof(cls) == size
    assert (TO.TsdfVolumeC.nx.offset, TO.TsdfVolumeC.origin_x.offset, TO.TsdfVolumeC.trunc.offset, TO.TsdfViewC.tanfovx.offset) == (24, 36, 52, 8)


def test_the_headers_sixteen_rows_are_the_rule():
    """tsdf_core.h packs the table into integers; tsdf_ref derives it from the rule the header states."""
    src = open(os.path.join(abi_check.ROOT, "gaussianprediction_amd", "csrc", "tsdf_core.h")).read()
    rows = [int(v, 16) for v in re.search(r"rows\[16\] = \{(.*?)\}", src, flags=re.S).group(1).replace("\n", " ").split(",")]
    assert [[(r >> 4 * s) & 15 for s in range(6)] for r in rows] == [[15 if e < 0 else e for e in row] for row in ref.case_table()]
    counts = int(re.search(r"ts_case_triangles\(int mask\) \{ return \((0x[0-9a-f]+)", src).group(1), 16)
    assert [(counts >> 2 * m) & 3 for m in range(16)] == [len(ref.case_triangles(m)) for m in range(16)]
    tets = [int(v, 16) for v in re.search(r"tets\[6\] = \{(.*?)\}", src).group(1).split(",")]
    assert [tuple((t >> 4 * v) & 7 for v in range(4)) for t in tets] == [cb for cb, _ in ref.tetrahedra()]
    odd = int(re.search(r"ts_tet_odd\(int q\) \{ return \(\((0x[0-9a-f]+)", src).group(1), 16)
    assert [bool(odd >> q & 1) for q in range(6)] == [o for _, o in ref.tetrahedra()]
    # the six tetrahedra tile the cell: each has volume 1/6 with the stated sign
    for cb, is_odd in ref.tetrahedra():
        p = np.array([[b & 1, b >> 1 & 1, b >> 2 & 1] for b in cb], np.float64)
        assert abs(np.linalg.det(p[1:] - p[0]) - (-1.0 if is_odd else 1.0)) < 1e-12


# ---- the programs in a stand-alone build, under the sanitizers ----
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    d = tmp_path_factory.mktemp("tsdf_emulate")
    exe = emulate_build.build("tsdf_emulate", d, sanitize=True)

    def run(head, arrays):
        job, out = str(d / "job.bin"), str(d / "out.bin")
        with open(job, "wb") as fp:
            fp.write(head)
            for a in arrays:
                if a is not None:
                    fp.write(np.ascontiguousarray(a).tobytes())
        subprocess.check_call([exe, job, out], timeout=300)
        return open(out, "rb").read()

    return run


def emulated_integrate(emulator, vol, depth, valid, image, views, z_min, view_weight, weight_max):
    V, H, W = depth.shape
    n = vol.nx * vol.ny * vol.nz
    has_color = vol.color is not None
    head = struct.pack("<iiiiiiiii8f", 0, vol.nx, vol.ny, vol.nz, int(has_color), V, H, W, int(valid is not None), *vol.origin, vol.voxel, vol.trunc,
                       z_min, view_weight, weight_max)
    flat = [np.concatenate([np.asarray(v.vm, F), np.array([v.tanfovx, v.tanfovy], F)]) for v in views]
    raw = emulator(head, [np.stack(flat), vol.tsdf, vol.weight, vol.color, depth, valid, image])
    assert len(raw) == 4 * n * (5 if has_color else 2)
    return np.frombuffer(raw, F, n), np.frombuffer(raw, F, n, 4 * n), np.frombuffer(raw, F, 3 * n, 8 * n).reshape(3, n) if has_color else None


def emulated_extract(emulator, vol, iso, min_weight):
    has_color = vol.color is not None
    raw = emulator(struct.pack("<iiiii6f", 1, vol.nx, vol.ny, vol.nz, int(has_color), *vol.origin, vol.voxel, iso, min_weight), [vol.tsdf, vol.weight, vol.color])
    counts = np.frombuffer(raw, np.int32, 2)
    nv, nf = int(counts[0]), int(counts[1])
    assert len(raw) == 8 + 12 * nv * (2 if has_color else 1) + 12 * nf
    vertices = np.frombuffer(raw, F, 3 * nv, 8).reshape(nv, 3)
    colors = np.frombuffer(raw, F, 3 * nv, 8 + 12 * nv).reshape(nv, 3) if has_color else None
    return counts, vertices, colors, np.frombuffer(raw, np.int32, 3 * nf, 8 + 12 * nv * (2 if has_color else 1)).reshape(nf, 3)


@pytest.mark.parametrize("name", list(cases.EXTRACT))
def test_the_emulated_extraction_against_the_restatement(emulator, name):
    vol, iso, min_weight = cases.EXTRACT[name]
    counts, vertices, colors, faces = emulated_extract(emulator, vol, iso, min_weight)
    w_counts, w_vertices, w_colors, w_faces = cases.extracted(name)
    assert same(counts, w_counts), (counts, w_counts)
    assert same(vertices, w_vertices) and same(faces, w_faces)
    assert (colors is None and w_colors is None) or same(colors, w_colors)


@pytest.mark.parametrize("name", list(cases.INTEGRATE))
def test_the_emulated_integration_against_the_restatement(emulator, name):
    c = cases.INTEGRATE[name]
    got = cases.integrate_in_groups(lambda vol, d, m, im, vs: emulated_integrate(emulator, vol, d, m, im, vs, c.z_min, c.view_weight, c.weight_max), c)
    want = cases.integrated(name)
    assert same(got[0], want[0]) and same(got[1], want[1])
    assert (got[2] is None and want[2] is None) or same(got[2], want[2])


def test_the_cases_reach_what_they_are_for():
    X = cases.extracted
    assert X("1x6x6_random")[0].tolist() == [0, 0] and X("13x11x7_empty")[0].tolist() == [0, 0]
    assert X("13x11x7_inside")[0].tolist() == [0, 0] and X("13x11x7_outside")[0].tolist() == [0, 0]
    assert X("2x2x2_random")[0][0] > 0 and X("5x4x3_plain")[2] is None
    assert X("13x11x7_random")[0][0] > 1024 and X("19x13x9_random")[0][1] > 3 * 1024            # the lists themselves cross tiles
    for name in ("13x11x7_random", "19x13x9_random", "19x13x9_hole"):
        vol, iso, mw = cases.EXTRACT[name]
        ids = np.flatnonzero(ref.marks(vol, iso, mw).reshape(-1))
        assert len(np.unique(ids // (7 * 1024))) == -(-vol.nx * vol.ny * vol.nz * 7 // (7 * 1024))      # every tile of points holds crossing edges
    # the hole: inactive cells, and edges whose ends differ in sign but lie in no active cell
    vol, iso, mw = cases.EXTRACT["19x13x9_hole"]
    usable, inside, active = ref.classify(vol, iso, mw)
    assert not usable[4, 6, 9] and not usable[2, 3, 4] and not usable[6, 9, 14] and active[:-1, :-1, :-1].mean() < 0.9 and not active[3:5, 4:8, 6:12].any()
    differ = inside[:, :, :-1] != inside[:, :, 1:]
    crossing = ref.marks(vol, iso, mw).reshape(9, 13, 19, 7)[:, :, :-1, 0]
    assert (differ & ~crossing).sum() > 20 and not (crossing & ~differ).any()
    full = ref.extract(SimpleNamespace(**{**vars(vol), "weight": np.ones_like(vol.weight), "tsdf": np.nan_to_num(vol.tsdf, nan=0.5, posinf=1, neginf=-1)}), iso, mw)
    assert X("19x13x9_hole")[0][1] < full[0][1]
    # samples equal to iso are not inside, and put vertices on grid points; the zero-area triangles are kept
    for name in ("5x4x3_equal_iso", "13x11x7_equal_iso"):
        vol, iso, mw = cases.EXTRACT[name]
        counts, vertices, _, faces = X(name)
        assert (vol.tsdf == F(iso)).sum() > 5 and counts[0] > 0
        grid = np.stack(ref.coords(vol), axis=1)
        on_grid = (vertices[:, None, :] == grid[None, vol.tsdf == F(iso)]).all(-1).any(-1)
        assert on_grid.sum() > 0
        tri = vertices[faces].astype(np.float64)
        area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
        print(name, "vertices on grid points", int(on_grid.sum()), "zero-area triangles", int((area == 0).sum()))
        assert (area == 0).sum() > 0
    # integrate
    c, (t, w, col) = cases.INTEGRATE["aligned_16x12_v1"], cases.integrated("aligned_16x12_v1")
    x, y, z = ref.coords(c.vol)
    assert (z.reshape(7, -1)[1] == F(c.z_min)).all() and (w.reshape(7, -1)[:2] == 0).all() and (w.reshape(7, -1)[2] > 0).any()       # at z_min: not seen
    with np.errstate(all="ignore"):
        half = (x / (z * F(0.5)) + F(1)) * F(8)                    # px + 0.5
    in_front = z > F(c.z_min)
    assert ((half == np.floor(half)) & (half > 0) & (half < 16) & in_front).sum() > 50          # exactly on a pixel boundary
    assert ((half < 0) & in_front).sum() > 0 and ((half >= 16) & in_front).sum() > 0             # outside the left and the right border
    plane4 = np.flatnonzero((z == 1) & (half >= 0) & (half < 16) & (np.abs(y) < 0.2))
    cols = np.floor(half[plane4]).astype(int)
    seen = w[plane4] > 0
    assert (z[plane4] == 1).all() and not seen[cols % 3 == 1].any() and seen[cols % 3 == 0].sum() > 3 and seen[cols % 3 == 2].sum() > 3      # one ulp under -trunc is skipped
    assert (t[plane4][seen & (cols % 3 == 0)] == -1).all()          # s == -trunc exactly is taken, as -1
    assert (w == 0).sum() > 100 and (w == 1).sum() > 100 and t.max() == 1.0 and t.min() == -1.0
    c, (t, w, col) = cases.INTEGRATE["round_16x12_v16_cap"], cases.integrated("round_16x12_v16_cap")
    assert w.max() == F(2.5) and (w == F(2.5)).sum() > 100 and 0 < (w == 1).sum()               # the cap, reached inside the batch
    uncapped = ref.integrate(c.vol, c.depth, c.valid, c.image, c.views, c.z_min, c.view_weight, 64.0)
    assert uncapped[1].max() >= 6 and not same(uncapped[0], t)                                   # the cap changes the running mean
    m = np.asarray(c.views[1].vm, F)
    pz = m[2] * x + m[6] * y + m[10] * z + m[14]
    assert (pz < 0).sum() > 200 and (pz > 0).sum() > 200                                         # a camera inside the volume
    assert cases.integrated("plain_16x12_v3")[2] is None and len(cases.INTEGRATE["round_40x30_v17"].views) == 17
    started = cases.INTEGRATE["started_40x30_v3"]
    after = cases.integrated("started_40x30_v3")[1]
    assert (started.vol.weight > 0).all() and (after[after != started.vol.weight] <= 4).all() and (after == 4).sum() > 50      # every seen point is under the cap
    for name, c in cases.INTEGRATE.items():
        t, w, col = cases.integrated(name)
        changed = w != c.vol.weight
        assert 0.1 < changed.mean() and (~changed).sum() > 0, name
        assert np.isfinite(t).all() and (np.abs(t[changed]) <= 1).all()
        if name.startswith("round") or name.startswith("plain"):       # from an empty volume: the clamp at 1 and the band below it
            assert (np.abs(t[changed]) < 1).sum() > 50 and (t[changed] == 1).sum() > 5, name
        bad = ~np.isfinite(c.depth) | (c.depth <= 0)
        assert bad.sum() >= 5, name


# ---- the restatement against independent facts ----
def check_closed_surface(vertices, faces, euler):
    facts = ref.mesh_facts(vertices, faces)
    print(facts)
    assert facts["edge_uses"] == {2}                 # every undirected edge lies in exactly two triangles
    assert facts["directed_max"] == 1 and 2 * facts["E"] == 3 * facts["F"]      # every directed edge occurs exactly once
    assert facts["euler"] == euler and facts["unreferenced"] == 0 and facts["volume"] > 0
    return facts


def test_the_restatement_on_a_sphere():
    vol, iso, mw = cases.EXTRACT["33_sphere"]
    s = cases.SPHERE
    x, y, z = (a.astype(np.float64) for a in ref.coords(vol))
    exact = cases.sphere_sdf(x, y, z)
    assert (vol.tsdf != F(iso)).all() and (vol.weight >= mw).all() and np.isfinite(vol.tsdf).all()         # no sample on iso, all usable
    boundary = (np.arange(vol.nx * vol.ny * vol.nz).reshape(33, 33, 33)[1:-1, 1:-1, 1:-1]).reshape(-1)
    outer = np.setdiff1d(np.arange(33 ** 3), boundary)
    assert (exact[outer] > 2 * vol.voxel).all() and (exact < 0).sum() > 1000                             # strictly inside the grid
    counts, vertices, colors, faces = cases.extracted("33_sphere")
    facts = check_closed_surface(vertices, faces, 2)
    assert counts.tolist() == [facts["V"], facts["F"]]
    dist = np.abs(np.linalg.norm(vertices.astype(np.float64) - np.array(s.c), axis=1) - s.r)
    print("sphere: largest | |v - c| - r | in voxels", dist.max() / vol.voxel)
    assert dist.max() <= np.sqrt(3) * vol.voxel      # a vertex lies on a lattice edge no longer than sqrt(3) voxel whose ends straddle the surface of a 1-Lipschitz function
    assert abs(facts["volume"] - 4 / 3 * np.pi * s.r ** 3) < 0.02 * facts["volume"]
    assert colors.min() >= 0 and colors.max() <= 1 and np.abs(colors - (vertices + 1.6) / 3.2).max() < 1e-5          # colour = position, interpolated alike


@pytest.mark.parametrize("name, euler", [("33_ellipsoid", 2), ("33_torus", 0)])
def test_the_restatement_on_an_ellipsoid_and_a_torus(name, euler):
    vol, iso, mw = cases.EXTRACT[name]
    assert (vol.tsdf != F(iso)).all() and (vol.tsdf.reshape(33, 33, 33)[[0, -1]] > 0).all() and (vol.tsdf.reshape(33, 33, 33)[:, [0, -1]] > 0).all() \
        and (vol.tsdf.reshape(33, 33, 33)[:, :, [0, -1]] > 0).all()
    counts, vertices, colors, faces = cases.extracted(name)
    check_closed_surface(vertices, faces, euler)
    if name == "33_torus":
        t = cases.TORUS
        v = vertices.astype(np.float64) - np.array(t.c)
        dist = np.abs(np.sqrt((np.sqrt(v[:, 0] ** 2 + v[:, 1] ** 2) - t.R) ** 2 + v[:, 2] ** 2) - t.r)
        assert dist.max() <= np.sqrt(3) * vol.voxel
    open_facts = ref.mesh_facts(*[cases.extracted("13x11x7_open_sphere")[k] for k in (1, 3)])
    assert open_facts["edge_uses"] == {1, 2} and open_facts["directed_max"] == 1           # a surface that leaves the grid has a border, wound alike


def test_integrate_and_extract_an_analytic_plane():
    d, trunc, voxel = float(F(1.53)), 0.25, 0.0625       # (between two planes of the grid: no sample is 0)
    vol = ref.volume(9, 9, 17, (-0.25, -0.25, 1.0), voxel, trunc)
    front = cases.plain_view(0.0, 0.5, 0.5)
    H = W = 32
    depth = np.full((1, H, W), d, F)
    image = np.full((1, 3, H, W), 0.5, F)
    t, w, col = ref.integrate(vol, depth, None, image, [front])
    x, y, z = ref.coords(vol)
    assert (w == 1).sum() > 0 and (z[w == 0] > d + trunc).all() and (z[w == 1] <= d + trunc).all()      # every point projects inside the image
    assert same(t[w == 1], np.minimum(F(1), (F(d) - z[w == 1]) / F(trunc))) and same(col[:, w == 1], np.full((3, int((w == 1).sum())), 0.5, F))
    # a second view from the side: the camera at (3, 0, 1.5) looking along -x sees the plane x = 0.25 + ... as depth 2.875 everywhere
    side = cases.look_at((3.0, 0.0, 1.5), (0.0, 0.0, 1.5), 0.5, 0.5)
    one = SimpleNamespace(**{**vars(vol), "tsdf": t, "weight": w, "color": col})
    t2, w2, col2 = ref.integrate(one, np.full((1, H, W), 2.875, F), None, np.full((1, 3, H, W), 1.0, F), [side], view_weight=3.0)
    m = np.asarray(side.vm, F)
    pz = ref.fma32(m[2], x, ref.fma32(m[6], y, ref.fma32(m[10], z, m[14])))
    ts = np.minimum(F(1), (F(2.875) - pz) / F(trunc))
    both = (w == 1) & (w2 == 4)
    assert both.sum() > 100 and same(t2[both], ((t[both] * F(1) + ts[both] * F(3)) / F(4))) and same(col2[0][both], np.full(int(both.sum()), (F(0.5) + F(3)) / F(4), F))
    only_side = (w == 0) & (w2 == 3)
    assert only_side.sum() > 0 and same(t2[only_side], ((F(0) * F(0) + ts[only_side] * F(3)) / F(3)))
    # the front view alone extracts as a flat sheet at z = d
    counts, vertices, colors, faces = ref.extract(one, 0.0, 1.0)
    assert counts[0] > 100 and counts[1] > 100
    err = float(np.abs(vertices[:, 2].astype(np.float64) - d).max())
    print("the plane's sheet: largest |z - d|", err)
    # t0 and t1 (|t| <= 1/4) carry two roundings each, a = -t0 / (t1 - t0) with t1 - t0 = -1/4 three more: below 16 x 2^-24, times the
    # voxel 1/16; the final fmaf rounds once at a value below 2: 2^-24
    assert err <= 2 * 2.0 ** -24
    tri = vertices[faces].astype(np.float64)
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (normal[:, 2] < 0).all()                  # towards larger tsdf: towards the camera


# ---- mesh PLY files ----
def test_mesh_ply_round_trip(tmp_path):
    counts, vertices, colors, faces = cases.extracted("5x4x3_random")
    path = str(tmp_path / "deep" / "mesh.ply")
    io_formats.save_mesh_ply(path, vertices, faces, colors)
    raw = open(path, "rb").read()
    nv, nf = len(vertices), len(faces)
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n"
              "property uchar green\nproperty uchar blue\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n" % (nv, nf)).encode()
    assert raw.startswith(header) and len(raw) == len(header) + 15 * nv + 13 * nf
    v, f, c = io_formats.read_mesh_ply(path)
    assert same(v, vertices) and same(f, faces) and same(c, io_formats.color_to_uint8(colors)) and c.dtype == np.uint8
    io_formats.save_mesh_ply(path, torch.from_numpy(vertices), torch.from_numpy(faces), torch.from_numpy(colors))      # tensors pass alike
    assert open(path, "rb").read() == raw
    io_formats.save_mesh_ply(path, vertices, faces)
    v, f, c = io_formats.read_mesh_ply(path)
    assert same(v, vertices) and same(f, faces) and c is None
    io_formats.save_mesh_ply(path, np.zeros((0, 3), F), np.zeros((0, 3), np.int32))
    v, f, c = io_formats.read_mesh_ply(path)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    with pytest.raises(ValueError, match="outside"):
        io_formats.save_mesh_ply(path, vertices, faces + nv)
    with pytest.raises(ValueError, match="colours"):
        io_formats.save_mesh_ply(path, vertices, faces, colors[:-1])
    for bad in (raw[:-1], raw + b"\0", b"plx" + raw[3:], raw.replace(b"list uchar int", b"list uchar uint")):
        (tmp_path / "bad.ply").write_bytes(bad)
        with pytest.raises(ValueError):
            io_formats.read_mesh_ply(str(tmp_path / "bad.ply"))


# ---- the refusals that need no device ----
def test_refusals_before_any_pointer_is_looked_at():
    l = TO.lib()
    nan, inf = float("nan"), float("inf")

    def volume(**kw):
        a = dict(tsdf=8, weight=8, color=None, nx=5, ny=4, nz=3, origin_x=0.0, origin_y=0.0, origin_z=0.0, voxel=0.1, trunc=0.4)
        a.update(kw)
        return TO.TsdfVolumeC(*[a[n] for n, _ in TO.TsdfVolumeC._fields_])

    def refused(rc, word):
        assert rc == 1 and word in l.gp_last_error(), (word, l.gp_last_error())

    volumes = ((dict(nx=0), b"nx, ny and nz"), (dict(nz=-1), b"nx, ny and nz"), (dict(nx=1024, ny=1024, nz=293), b"7*nx*ny*nz"), (dict(nx=2 ** 30, ny=2 ** 30, nz=2 ** 30), b"7*nx*ny*nz"),
               (dict(voxel=0.0), b"> 0"), (dict(trunc=-1.0), b"> 0"), (dict(voxel=nan), b"finite"), (dict(trunc=inf), b"finite"), (dict(origin_y=inf), b"finite"),
               (dict(tsdf=None), b"null"), (dict(weight=None), b"null"))
    views = (TO.TsdfViewC * 2)(TO.TsdfViewC(8, 0.5, 0.5), TO.TsdfViewC(8, 0.5, 0.5))
    defaults = dict(vol=volume(), depth=8, valid=None, image=None, views=views, V=2, H=12, W=16, z_min=1e-3, view_weight=1.0, weight_max=64.0)

    def integrate(**kw):
        a = dict(defaults)
        a.update(kw)
        return l.gp_tsdf_integrate(None if a["vol"] is None else C.byref(a["vol"]), a["depth"], a["valid"], a["image"], a["views"], a["V"], a["H"], a["W"], a["z_min"],
                                   a["view_weight"], a["weight_max"], None)

    for kw, word in volumes:
        refused(integrate(vol=volume(**kw)), word)
        refused(l.gp_tsdf_extract_count(C.byref(volume(**kw)), 0.0, 1.0, 8, 8, None), word)
        refused(l.gp_tsdf_extract_fill(C.byref(volume(**kw)), 0.0, 8, 8, None, 8, None), word)
    for kw, word in ((dict(vol=None), b"null"), (dict(V=0), b"V must be"), (dict(V=17), b"V must be"), (dict(H=0), b"H and W"), (dict(W=-2), b"H and W"),
                     (dict(H=2 ** 16, W=2 ** 15), b"H*W"), (dict(z_min=0.0), b"finite and > 0"), (dict(z_min=nan), b"finite and > 0"), (dict(view_weight=-1.0), b"finite and > 0"),
                     (dict(weight_max=inf), b"finite and > 0"), (dict(depth=None), b"null"), (dict(views=None), b"null"),
                     (dict(views=(TO.TsdfViewC * 2)(TO.TsdfViewC(8, 0.5, 0.5), TO.TsdfViewC(None, 0.5, 0.5))), b"null"),
                     (dict(views=(TO.TsdfViewC * 2)(TO.TsdfViewC(8, 0.5, nan), TO.TsdfViewC(8, 0.5, 0.5))), b"finite"),
                     (dict(image=8), b"go together"), (dict(vol=volume(color=8)), b"go together")):
        refused(integrate(**kw), word)
    vol = volume()
    for args, word in (((None, 0.0, 1.0, 8, 8), b"null"), ((C.byref(vol), nan, 1.0, 8, 8), b"iso"), ((C.byref(vol), inf, 1.0, 8, 8), b"iso"), ((C.byref(vol), 0.0, nan, 8, 8), b"NaN"),
                       ((C.byref(vol), 0.0, 1.0, None, 8), b"null"), ((C.byref(vol), 0.0, 1.0, 8, None), b"null"), ((C.byref(vol), 0.0, 1.0, 10, 8), b"aligned")):
        refused(l.gp_tsdf_extract_count(*args, None), word)
    for args, word in (((None, 0.0, 8, 8, None, 8), b"null"), ((C.byref(vol), nan, 8, 8, None, 8), b"iso"), ((C.byref(vol), 0.0, None, 8, None, 8), b"null"),
                       ((C.byref(vol), 0.0, 8, None, None, 8), b"null"), ((C.byref(vol), 0.0, 8, 8, None, None), b"null"), ((C.byref(vol), 0.0, 8, 8, 8, 8), b"go together"),
                       ((C.byref(volume(color=8)), 0.0, 8, 8, None, 8), b"go together"), ((C.byref(vol), 0.0, 6, 8, None, 8), b"aligned")):
        refused(l.gp_tsdf_extract_fill(*args, None), word)
    for dims, word in (((0, 4, 3), b"nx, ny and nz"), ((1024, 1024, 293), b"7*nx*ny*nz")):
        assert l.gp_tsdf_extract_scratch_bytes(*dims) == -1 and word in l.gp_last_error() and TO.check_dims(*dims).encode() in l.gp_last_error()
    up = lambda v: (v + 255) // 256 * 256             # noqa: E731
    assert l.gp_tsdf_extract_scratch_bytes(5, 4, 3) == 3 * up(60) + 2 * up(240) + 2 * up(4)
    assert l.gp_tsdf_extract_scratch_bytes(19, 13, 9) == 3 * up(2223) + 2 * up(4 * 2223) + 2 * up(12)
    assert TO.check_dims(1024, 1024, 292) is None and l.gp_tsdf_extract_scratch_bytes(1024, 1024, 292) > 11 * 1024 * 1024 * 292


def test_the_python_surface_refuses_before_the_device(monkeypatch):
    monkeypatch.setattr(TO, "lib", lambda: pytest.fail("a launch was reached"))
    for call, word in ((lambda: TO.TsdfVolume((0, 0, 0), 0.1, (0, 4, 4)), "nx, ny and nz"), (lambda: TO.TsdfVolume((0, 0, 0), 0.1, (1024, 1024, 293)), "7\\*nx"),
                       (lambda: TO.TsdfVolume((0, 0, 0), 0.0, (4, 4, 4)), "> 0"), (lambda: TO.TsdfVolume((0, 0, float("inf")), 0.1, (4, 4, 4)), "finite"),
                       (lambda: TO.TsdfVolume((0, 0, 0), 0.1, (4, 4, 4), trunc=-1.0), "> 0")):
        with pytest.raises(_lib.GpHipError, match=word):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TO.TsdfVolume((0, 0, 0), 0.1, (4, 4, 4), device="cpu")
    with pytest.raises(RuntimeError, match="three numbers"):
        TO.TsdfVolume((0, 0), 0.1, (4, 4, 4))
    cam = SimpleNamespace(world_view_transform=torch.eye(4), time=np.array([0.0], F))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TO.fuse([cam], None, None, 1)
    with pytest.raises(_lib.GpHipError, match="V must be"):
        TO.fuse([], None, None, 1)
    assert TO.Mesh._fields == ("vertices", "faces", "colors") and TO.View._fields == ("world_view", "tanfovx", "tanfovy")
    assert TO.check_dims(2, 2, 2) is None and TO.check_grid((0, 0, 0), 0.1, 0.4) is None


def test_signatures_and_docstrings():
    from gaussianprediction_amd import eval_render as ER
    assert list(inspect.signature(TO.TsdfVolume.__init__).parameters) == ["self", "origin", "voxel_size", "dims", "trunc", "color", "device"]
    assert list(inspect.signature(TO.TsdfVolume.integrate).parameters) == ["self", "depth", "valid", "views", "image", "weight", "weight_max", "z_min"]
    d = {k: p.default for k, p in inspect.signature(TO.TsdfVolume.integrate).parameters.items() if p.default is not inspect.Parameter.empty}
    assert d == dict(image=None, weight=1.0, weight_max=64.0, z_min=1e-3)
    assert {k: p.default for k, p in inspect.signature(TO.TsdfVolume.extract).parameters.items() if k != "self"} == dict(iso=0.0, min_weight=1.0)
    sig = inspect.signature(TO.fuse)
    assert list(sig.parameters)[:10] == ["views", "gaussians", "pipeline", "iteration", "time", "bounds", "voxel_size", "resolution", "alpha_min", "trunc"]
    assert (sig.parameters["resolution"].default, sig.parameters["alpha_min"].default, sig.parameters["time"].default) == (256, 0.5, None)
    sig = inspect.signature(ER.render_meshes)
    assert list(sig.parameters)[:9] == ["model_path", "name", "iteration", "views", "gaussians", "pipeline", "background", "times", "resolution"]
    assert sig.parameters["times"].default is None and sig.parameters["resolution"].default == 256
    assert "only read" in " ".join(TO.TsdfVolume.extract.__doc__.split()) and "meshes/%05d.ply" in ER.render_meshes.__doc__
    assert inspect.getsource(ER).count("render_meshes(") == 1            # opt-in: no other loop calls it
    assert list(inspect.signature(io_formats.save_mesh_ply).parameters) == ["path", "vertices", "faces", "colors"]
