"""No GPU: csrc/gp_depth.h against the binding's table (a binding outside _lib.ABIS); the programs of csrc/depth_core.h in a stand-alone
build (tests/depth_emulate.cpp, under the sanitizers where the host compiler can link them) against the numpy restatement
tests/depth_ref.py on every case of tests/depth_cases.py -- bit for bit for resolve, valid, the derived range, the LUT rows, normals and
nvalid, points, colours, index and count, and the metric counts; the float64 columns without a logf within 1e-12 relative; the two log
columns within max(8 x |float32 restatement - float64 restatement|, 1e-9); the restatement against an analytic plane; the PFM files;
the refusals that need no device."""
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
import depth_cases as cases
import depth_ref as ref
import emulate_build
import flow_ref
from gaussianprediction_amd import _lib, depth_ops as DO

_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "gp_stream_t": _lib.Ptr}
_POINTEES = {"float", "uint8_t", "int32_t", "double", "void"}
F64_BAR = 1e-12              # relative: at most 3072 non-negative terms at 2^-53 each, about 3.4e-13, a division and a square root
F = np.float32


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_row(got, want32, want64, where):
    """One row of the table under the rules of the module's docstring; prints the distances of the log columns."""
    if np.isnan(want32).all():
        assert np.isnan(got).all(), where
        return
    assert got[0] == want32[0] and got[11] == 0.0, (where, got[0], want32[0])
    plain = list(cases.PLAIN_COLUMNS)
    assert (np.abs(got[plain] - want32[plain]) <= F64_BAR * np.abs(want32[plain])).all(), (where, got[plain], want32[plain])
    logs, bar = list(cases.LOG_COLUMNS), cases.log_bar(want32, want64)
    dist = np.abs(got[logs] - want32[logs])
    print(where, "log columns: distance", dist, "bar", bar)
    assert (dist <= bar).all(), (where, dist, bar)


# ---- the header, the table, the registry ----
def test_prototype_table_equals_the_header_and_stays_out_of_the_registry():
    before = len(_lib.ABIS)
    protos = abi_check.check_table(DO.ABI, 9, _SCALARS, _POINTEES, {"gp_depth_view": DO.DepthViewC})
    assert DO.ABI.prototypes is DO.PROTOTYPES and DO.ABI not in _lib.ABIS and len(_lib.ABIS) == before
    assert os.path.samefile(os.path.join(abi_check.ROOT, "include", DO.ABI.header),
                            os.path.join(abi_check.ROOT, "gaussianprediction_amd", "csrc", "gp_depth.h"))
    for name in ("gp_depth_resolve", "gp_depth_colorize", "gp_depth_normals", "gp_depth_normals_image", "gp_depth_unproject", "gp_depth_metrics"):
        assert protos[name][1][-1] == "gp_stream_t"              # the stream is the last parameter
    assert not os.path.exists(os.path.join(abi_check.ROOT, "include", "gp_depth.h"))


def test_symbols_constants_and_the_struct():
    text = abi_check.header_text(DO.HEADER)
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_DEPTH_[A-Z0-9_]+) +(\d+)", text)}
    assert defs["GP_DEPTH_ABI_VERSION"] == DO.GP_DEPTH_ABI_VERSION == DO.ABI.version == 1
    assert (defs["GP_DEPTH_TILE"], defs["GP_DEPTH_SUMS"], defs["GP_DEPTH_COLUMNS"], defs["GP_DEPTH_LUT"]) == (DO.TILE, DO.SUMS, DO.COLUMNS, DO.LUT) == (1024, 12, 12, 256)
    assert (ref.TILE, ref.SUMS, ref.COLUMNS, ref.LUT) == (DO.TILE, DO.SUMS, DO.COLUMNS, DO.LUT) and len(DO.METRIC_NAMES) == DO.COLUMNS
    assert DO.METRIC_NAMES[9] == "scale" and DO.METRIC_NAMES[0] == "count" and DO.MODES == {"depth": 0, "disparity": 1}
    abi_check.check_applied(DO.ABI)
    fields = re.search(r"typedef struct gp_depth_view \{(.*?)\}", text, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*[,;]", fields) == ["cam2world", "tanfovx", "tanfovy", "W", "H"]
    assert [n for n, _ in DO.DepthViewC._fields_] == ["cam2world", "tanfovx", "tanfovy", "W", "H"] and C.sizeof(DO.DepthViewC) == 24
    assert (DO.DepthViewC.tanfovx.offset, DO.DepthViewC.W.offset) == (8, 16)


# ---- the programs in a stand-alone build, under the sanitizers ----
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    d = tmp_path_factory.mktemp("depth_emulate")
    exe = emulate_build.build("depth_emulate", d, sanitize=True)

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


def emulated_metrics(emulator, pred, gt, mask, scale, gt_min, gt_max):
    B, H, W = pred.shape
    raw = emulator(struct.pack("<iiiiiiff", 4, B, H, W, int(mask is not None), int(scale is not None), gt_min, gt_max),
                   [pred, gt, mask, None if scale is None else np.asarray(scale, F)])
    return np.frombuffer(raw, np.float64).reshape(B, 12)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_emulated_programs_against_the_restatement(emulator, name):
    c, want = cases.CASES[name], cases.reference(name)
    H, W, plane, v = c.H, c.W, c.H * c.W, c.view
    raw = emulator(struct.pack("<iiif", 0, H, W, c.alpha_min), [c.accum, c.alpha])
    assert len(raw) == 5 * plane
    assert same(np.frombuffer(raw, F, plane).reshape(H, W), want.resolve[0]) and same(np.frombuffer(raw, np.uint8, plane, 4 * plane).reshape(H, W), want.resolve[1])
    for (mname, mode, lo, hi) in cases.COLOUR_MODES:
        for masked in (False, True):
            raw = emulator(struct.pack("<iiiiifffff", 1, H, W, int(masked), mode, lo, hi, *cases.BG), [c.depth, cases.lut(), c.valid if masked else None])
            out, rng, _ = want.colour[(mname, masked)]
            assert same(np.frombuffer(raw, F, 2), rng), (mname, masked, np.frombuffer(raw, F, 2), rng)            # the range, bit for bit
            assert same(np.frombuffer(raw, F, 3 * plane, 8).reshape(3, H, W), out), (mname, masked)                # the LUT rows (every row differs)
    for masked in (False, True):
        raw = emulator(struct.pack("<iiiifffff", 2, H, W, int(masked), v.tanfovx, v.tanfovy, *cases.BG), [c.depth, c.valid if masked else None])
        n, nvalid = want.normals[masked]
        assert same(np.frombuffer(raw, F, 3 * plane).reshape(3, H, W), n) and same(np.frombuffer(raw, np.uint8, plane, 12 * plane).reshape(H, W), nvalid), masked
        if masked:
            assert same(np.frombuffer(raw, F, 3 * plane, 13 * plane).reshape(3, H, W), want.picture)
        for with_image in (False, True):
            raw = emulator(struct.pack("<iiiiiff", 3, H, W, int(masked), int(with_image), v.tanfovx, v.tanfovy),
                           [v.c2w, c.depth, c.valid if masked else None, c.image if with_image else None])
            points, colors, index, count = want.unproject[masked]
            assert struct.unpack("<i", raw[:4])[0] == count
            got = np.frombuffer(raw, F, 3 * plane, 4).reshape(plane, 3)
            assert same(got[:count], points) and (got[count:] == -7).all(), (masked, with_image)
            off = 4 + 12 * plane
            if with_image:
                got = np.frombuffer(raw, F, 3 * plane, off).reshape(plane, 3)
                assert same(got[:count], colors) and (got[count:] == -7).all()
                off += 12 * plane
            got = np.frombuffer(raw, np.int32, plane, off)
            assert same(got[:count], index) and (got[count:] == -7).all() and len(raw) == off + 4 * plane
    for (masked, scaled), row in want.metrics.items():
        got = emulated_metrics(emulator, c.pred[None], c.gt[None], c.mask[None] if masked else None, [c.scale] if scaled else None, c.gt_min, c.gt_max)[0]
        check_row(got, row, want.metrics64[(masked, scaled)], (name, masked, scaled))


def test_the_cases_reach_what_they_are_for(emulator):
    c, want = cases.CASES["37x53_random"], cases.reference("37x53_random")
    depth, valid = want.resolve
    #                       x/0  below  at  0  NaN  inf  -inf  negative  0/0  overflow  tiny  plain
    assert valid[0, :12].tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1] and (depth[valid == 0] == 0).all() and np.isfinite(depth).all()
    assert float(c.alpha[0, 1]) < 1e-3 <= float(c.alpha[0, 2]) and c.alpha[0, 2] == F(1e-3) and depth[0, 2] == 3.0
    # colour: the derived ranges are the extremes of the coloured values, a pixel on hi has t = 1 and takes row 255, one on lo row 0
    for mname, mode in (("depth", 0), ("disparity", 1)):
        out, rng, rows = want.colour[(mname, True)]
        v, take = ref.value(c.depth, c.valid, mode)
        assert rng[0] == v[take].min() < rng[1] == v[take].max() and rows[take & (v == rng[1])].tolist() == [255] and rows[take & (v == rng[0])].tolist() == [0]
        assert (rows[~take] == -1).all() and len(np.unique(rows)) > 100 and 0 < take.sum() < take.size
    assert want.colour[("depth", True)][2][1, :8].tolist() == [-1, -1, -1, -1, 0, 255, -1, want.colour[("depth", True)][2][1, 7]]   # 0, NaN, inf, < 0: background
    assert want.colour[("disparity", True)][2][1, 4:6].tolist() == [255, 0]
    extremes = cases.reference("37x53_extremes").colour
    assert extremes[("disparity", False)][2][1, 4] == -1 and extremes[("disparity", False)][1][0] == F(1) / F(3e38) > 0      # 1 / 1e-45 is infinite, 1 / 3e38 a denormal
    assert extremes[("depth", False)][1].tolist() == [float(F(1e-45)), float(F(3e38))]
    assert same(want.colour[("swapped_is_derived", True)][1], want.colour[("depth", True)][1]) and same(want.colour[("equal_is_derived", False)][1], want.colour[("disparity", False)][1])
    given = want.colour[("depth_given", False)]
    assert given[1].tolist() == [2.5, 3.25] and given[2][1, 7] == 0 and given[2].max() == 255 and (given[2] == 0).sum() > 1     # v == lo: t = 0; beyond hi: row 255
    assert (given[0][:, given[2] == -1] == np.array(cases.BG, F)[:, None]).all()
    const = cases.reference("37x53_constant").colour[("depth", False)]
    assert const[1].tolist() == [2.5, 2.5] and (const[2] == 0).all()                           # lo == hi: t = 0
    nothing = cases.reference("37x53_none")
    assert nothing.colour[("depth", True)][1].tolist() == [0.0, 1.0] and (nothing.colour[("depth", True)][2] == -1).all()
    assert nothing.unproject[True][3] == 0 and not nothing.normals[True][1].any() and nothing.unproject[False][3] == 37 * 53
    # normals: only the centre of 3 x 5 can have four neighbours; the checkerboard has none; the special depths break their neighbours
    small = cases.reference("3x5").normals[False][1]
    assert small.sum() <= 1 and not small[[0, 2]].any() and not small[:, [0, 4]].any()
    assert not cases.reference("37x53_checker").normals[True][1].any() and cases.reference("37x53_checker").unproject[True][3] == 37 * 53 // 2
    n, nvalid = cases.reference("37x53_all").normals[True]
    assert 0.8 < nvalid.mean() < 1.0 and np.abs(np.sqrt((n.astype(np.float64) ** 2).sum(0))[nvalid != 0] - 1).max() < 1e-6
    a = cases.CASES["37x53_all"]
    ys, xs = np.meshgrid(np.arange(a.H), np.arange(a.W), indexing="ij")
    with np.errstate(all="ignore"):
        toward = sum(n[k].astype(np.float64) * p for k, p in enumerate(ref.point(a.view, xs, ys, a.depth)))
    assert (toward[nvalid != 0] <= 0).all() and (toward[nvalid != 0] < -0.1).mean() > 0.9              # every normal faces the camera
    # the compaction: a run across the tile boundary, an empty tile between full ones
    s = cases.reference("37x53_straddle").unproject[True]
    assert s[2].tolist() == list(range(1024 - 37, 1024 + 29)) and s[3] == 66
    g = cases.reference("240x320_tile_gap").unproject[True]
    assert g[3] == 240 * 320 - 1024 and g[2][1023] == 1023 and g[2][1024] == 2048
    assert (cases.CASES["520x512_random"].H * cases.CASES["520x512_random"].W + 1023) // 1024 == 260
    # metrics: what counts, and the exact thresholds
    plain, masked = want.metrics[(False, False)], want.metrics[(True, False)]
    with np.errstate(all="ignore"):
        counts = np.isfinite(c.pred) & np.isfinite(c.gt) & (c.pred > 0) & (c.gt > 0) & (c.gt >= F(c.gt_min)) & (c.gt <= F(c.gt_max))
    assert plain[0] == counts.sum() < c.H * c.W and masked[0] == (counts & (c.mask != 0)).sum() < plain[0]
    assert counts[2, :9].tolist() == [True, True, True, True, False, False, False, False, False]       # the bounds count, 0, NaN, inf, beyond, negative do not
    assert 0 < plain[5] < plain[6] <= plain[7] < 1 and plain[1] > 0 and plain[3] > 0 and plain[11] == 0
    two = np.array([[2.5, 2.0, 2.4]], F)[None], np.array([[2.0, 2.5, 2.0]], F)[None]
    assert ref.metrics(*two)[0][5:8].tolist() == [1 / 3, 1.0, 1.0]                              # d/g and g/d of exactly 1.25 are not below it
    e = (c.pred.astype(np.float64) - c.gt)[counts]
    assert abs(plain[3] - np.sqrt((e * e).mean())) <= 1e-6 * plain[3] and abs(plain[1] - (np.abs(e) / c.gt[counts]).mean()) <= 1e-6 * plain[1]
    # a batch's rows are the single images' rows, whatever else is in the batch
    a, b = cases.CASES["37x53_random"], cases.CASES["37x53_all"]
    pred, gt, mask = np.stack([a.pred, b.pred, a.gt]), np.stack([a.gt, b.gt, a.pred]), np.stack([a.mask, np.zeros_like(b.mask), b.mask])
    table = emulated_metrics(emulator, pred, gt, mask, None, a.gt_min, a.gt_max)
    wanted = ref.metrics(pred, gt, mask, None, a.gt_min, a.gt_max)
    assert np.isnan(table[1]).all() and np.isnan(wanted[1]).all()
    for k in (0, 2):
        single = emulated_metrics(emulator, pred[k:k + 1], gt[k:k + 1], mask[k:k + 1], None, a.gt_min, a.gt_max)
        assert same(single[0], table[k])
    check_row(table[0], want.metrics[(True, False)], want.metrics64[(True, False)], "batch row 0")


# ---- the restatement against analytic truth ----
def test_the_restatement_on_an_analytic_plane():
    H, W = 240, 320
    v = cases.view(True, W, H, 0.5, 0.5)
    assert abs(v.tanfovx - 0.5) < 1e-15 and abs(v.tanfovy - 0.5) < 1e-15
    a, b, c0 = 0.2, -0.15, 3.0                                       # the plane z = c0 + a X + b Y in camera space
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rx, ry = ((2 * xs + 1) / W - 1) * 0.5, ((2 * ys + 1) / H - 1) * 0.5          # X = rx z, Y = ry z
    z64 = c0 / (1 - a * rx - b * ry)
    depth = z64.astype(F)
    assert 2.4 < z64.min() and z64.max() < 3.8
    n, nvalid = ref.normals(depth, None, v)
    truth = np.array([a, b, -1.0]) / np.sqrt(a * a + b * b + 1)     # faces the camera: n . P < 0
    inner = nvalid[1:-1, 1:-1]
    assert inner.all() and nvalid.sum() == (H - 2) * (W - 2)
    err = float(np.abs(n[:, 1:-1, 1:-1].astype(np.float64) - truth[:, None, None]).max())
    print("normals of the plane against the analytic normal:", err)
    assert err <= 1e-4              # depth rounding 2^-24 * 3 over twice the pixel pitch 0.0094 gives about 1e-5
    points, _, index, count = ref.unproject(depth, None, None, v)
    assert count == H * W and same(index, np.arange(H * W, dtype=np.int32))
    px, py, front = flow_ref.pixel(v, points)
    back = flow_ref.fma32(v.vm[2], points[:, 0], flow_ref.fma32(v.vm[6], points[:, 1], flow_ref.fma32(v.vm[10], points[:, 2], v.vm[14])))
    e_px = float(max(np.abs(px.astype(np.float64) - xs.reshape(-1)).max(), np.abs(py.astype(np.float64) - ys.reshape(-1)).max()))
    e_z = float((np.abs(back.astype(np.float64) - depth.reshape(-1)) / depth.reshape(-1)).max())
    print("unprojected points back through the projection: pixel", e_px, "relative depth", e_z)
    assert front.all() and e_px <= 1e-3 and e_z <= 1e-5              # a handful of float32 operations scaled by W


# ---- PFM files ----
def test_pfm_files(tmp_path):
    depth = np.arange(6, dtype=F).reshape(2, 3) + F(0.5)             # W = 3, H = 2: the top row 0.5 1.5 2.5, the bottom row 3.5 4.5 5.5
    path = tmp_path / "a.pfm"
    DO.write_pfm(path, torch.from_numpy(depth))
    want = b"Pf\n3 2\n-1.0\n" + struct.pack("<6f", 3.5, 4.5, 5.5, 0.5, 1.5, 2.5)
    assert open(path, "rb").read() == want
    back = DO.read_pfm(path)
    assert back.dtype == torch.float32 and back.shape == (2, 3) and same(back.numpy(), depth)
    c = cases.CASES["37x53_random"]
    DO.write_pfm(str(tmp_path / "b.pfm"), c.depth)                   # NaN, infinities and -0.0 survive
    assert same(DO.read_pfm(str(tmp_path / "b.pfm")).numpy(), c.depth)
    (tmp_path / "big.pfm").write_bytes(b"Pf\n3 2\n1.0\n" + struct.pack(">6f", 3.5, 4.5, 5.5, 0.5, 1.5, 2.5))
    assert same(DO.read_pfm(tmp_path / "big.pfm").numpy(), depth)    # a positive scale: big-endian
    for bad in (b"PF" + want[2:], want[:-1], want + b"\0", b"Pf\n3 2\n", b"Pf\n0 2\n-1.0\n", b"Pf\n3 2\n0.0\n" + want[12:], b"Pf\n3 -2\n-1.0\n" + want[12:]):
        (tmp_path / "bad.pfm").write_bytes(bad)
        with pytest.raises(RuntimeError, match="read_pfm"):
            DO.read_pfm(tmp_path / "bad.pfm")
    with pytest.raises(RuntimeError, match=r"\[H, W\]"):
        DO.write_pfm(tmp_path / "c.pfm", np.zeros((3, 2, 2), F))


# ---- the refusals that need no device ----
def test_refusals_before_any_pointer_is_looked_at():
    l = DO.lib()
    view = DO.DepthViewC(8, 0.5, 0.5, 17, 13)

    def refused(rc, word):
        assert rc == 1 and word in l.gp_last_error(), (word, l.gp_last_error())

    planes = ((dict(H=0), b"H and W"), (dict(W=-3), b"H and W"), (dict(H=2 ** 16, W=2 ** 15), b"H*W"))
    nulls = lambda *names: tuple((dict([(n, None)]), b"null") for n in names)            # noqa: E731

    def sweep(call, defaults, table):
        for kw, word in table:
            a = dict(defaults, H=13, W=17)
            a.update(kw)
            refused(call(a), word)
            if kw in [p[0] for p in planes]:
                assert DO.check_plane(a["H"], a["W"]).encode() in l.gp_last_error()

    nan = float("nan")
    sweep(lambda a: l.gp_depth_resolve(a["accum"], a["alpha"], a["alpha_min"], a["depth"], a["valid"], a["H"], a["W"], None),
          dict(accum=8, alpha=8, alpha_min=1e-3, depth=8, valid=8), planes + nulls("accum", "alpha", "depth", "valid") + ((dict(alpha_min=nan), b"NaN"),))
    sweep(lambda a: l.gp_depth_colorize(a["depth"], a["valid"], a["mode"], a["lo"], a["hi"], a["lut"], 0.0, 0.0, 0.0, a["range"], a["out"], a["H"], a["W"], None),
          dict(depth=8, valid=None, mode=1, lo=0.0, hi=0.0, lut=8, range=8, out=8),
          planes + nulls("depth", "lut", "range", "out") + ((dict(lo=nan), b"NaN"), (dict(hi=nan), b"NaN"), (dict(mode=2), b"mode"), (dict(mode=-1), b"mode")))
    views = ((dict(view=None), b"null"), (dict(view=DO.DepthViewC(8, 0.5, 0.5, 16, 13)), b"view's W and H"), (dict(view=DO.DepthViewC(8, 0.5, 0.5, 17, 12)), b"view's W and H"),
             (dict(view=DO.DepthViewC(8, nan, 0.5, 17, 13)), b"NaN"), (dict(view=DO.DepthViewC(8, 0.5, nan, 17, 13)), b"NaN"))
    ref_of = lambda v: None if v is None else C.byref(v)                                  # noqa: E731
    sweep(lambda a: l.gp_depth_normals(a["depth"], a["valid"], ref_of(a["view"]), a["normals"], a["nvalid"], a["H"], a["W"], None),
          dict(depth=8, valid=None, view=view, normals=8, nvalid=8), planes + views + nulls("depth", "normals", "nvalid"))
    sweep(lambda a: l.gp_depth_normals_image(a["normals"], a["nvalid"], 0.0, 0.0, 0.0, a["out"], a["H"], a["W"], None),
          dict(normals=8, nvalid=8, out=8), planes + nulls("normals", "nvalid", "out"))
    sweep(lambda a: l.gp_depth_unproject(a["depth"], a["valid"], a["image"], ref_of(a["view"]), a["points"], a["colors"], a["index"], a["count"], a["scratch"],
                                         a["H"], a["W"], None),
          dict(depth=8, valid=None, image=None, view=view, points=8, colors=None, index=None, count=8, scratch=8),
          planes + views + nulls("depth", "points", "count", "scratch") + ((dict(view=DO.DepthViewC(0, 0.5, 0.5, 17, 13)), b"null"), (dict(image=8), b"go together"),
                                                                            (dict(colors=8), b"go together"), (dict(scratch=10), b"aligned")))
    for kw, _ in planes:
        a = dict(H=13, W=17)
        a.update(kw)
        assert l.gp_depth_unproject_scratch_bytes(a["H"], a["W"]) == -1 and DO.check_plane(a["H"], a["W"]).encode() in l.gp_last_error()
    assert l.gp_depth_unproject_scratch_bytes(13, 17) == 4 and l.gp_depth_unproject_scratch_bytes(1025, 1) == 8 and l.gp_depth_unproject_scratch_bytes(520, 512) == 260 * 4
    batches = planes + ((dict(B=0), b"B must be > 0"), (dict(B=65536), b"at most 65535"))
    for kw, word in batches + nulls("pred", "gt", "scratch", "table") + ((dict(scratch=12), b"aligned"), (dict(gt_min=nan), b"NaN"), (dict(gt_max=nan), b"NaN")):
        a = dict(pred=8, gt=8, mask=None, scale=None, gt_min=0.0, gt_max=float("inf"), B=2, H=13, W=17, scratch=8, table=8)
        a.update(kw)
        refused(l.gp_depth_metrics(a["pred"], a["gt"], a["mask"], a["scale"], a["gt_min"], a["gt_max"], a["B"], a["H"], a["W"], a["scratch"], a["table"], None), word)
        if kw in [p[0] for p in batches]:
            assert DO.check_batch(a["B"], a["H"], a["W"]).encode() in l.gp_last_error()
            assert l.gp_depth_metrics_scratch_bytes(a["B"], a["H"], a["W"]) == -1 and word in l.gp_last_error()
    assert l.gp_depth_metrics_scratch_bytes(2, 13, 17) == 2 * 1 * 12 * 8 and l.gp_depth_metrics_scratch_bytes(3, 37, 53) == 3 * 2 * 12 * 8
    assert DO.check_batch(65535, 1, 1) is None and DO.check_plane(13, 17) is None


def test_the_python_surface_refuses_before_the_device(monkeypatch):
    monkeypatch.setattr(DO, "lib", lambda: pytest.fail("a launch was reached"))
    cpu = "no CPU fallback"
    plane, image = torch.zeros(13, 17), torch.zeros(3, 13, 17)
    cam = cases.view(True, 17, 13).cam
    dummy = DO.DepthView(torch.zeros(4, 4), 0.5, 0.5, 17, 13, None)
    with pytest.raises(RuntimeError, match=cpu):
        DO.view_constants(cam)
    with pytest.raises(RuntimeError, match=r"\[4, 4\]"):
        DO.view_constants(SimpleNamespace(world_view_transform=torch.zeros(3, 4), image_width=17, image_height=13, FoVx=0.9, FoVy=0.7))
    for call, word in ((lambda: DO.resolve(plane, plane), cpu), (lambda: DO.resolve(image, plane), r"\[H, W\]"), (lambda: DO.resolve(plane.double(), plane), "float32"),
                       (lambda: DO.colorize(plane), cpu), (lambda: DO.colorize(image), r"\[H, W\]"), (lambda: DO.colorize(plane.half()), "float32"),
                       (lambda: DO.normals(plane, None, dummy), cpu), (lambda: DO.normals(image, None, dummy), r"\[H, W\]"),
                       (lambda: DO.normals_image(image, plane.bool()), cpu), (lambda: DO.normals_image(plane, plane.bool()), r"\[3, H, W\]"),
                       (lambda: DO.unproject(plane, None, dummy), cpu), (lambda: DO.unproject(plane.long(), None, dummy), "float32"),
                       (lambda: DO.depth_metrics(plane, plane), cpu), (lambda: DO.depth_metrics(plane[None], plane[None]), cpu),
                       (lambda: DO.depth_metrics(torch.zeros(2), plane), r"\[B, H, W\]"), (lambda: DO.depth_metrics(plane, plane.double()), "float32")):
        with pytest.raises(RuntimeError, match=word):
            call()
    g = SimpleNamespace(get_xyz=torch.zeros(4, 3), forward=lambda *a: pytest.fail("the model was evaluated"))
    with pytest.raises(RuntimeError, match=cpu):
        DO.render_depth(cam, g, None, 1)
    with pytest.raises(RuntimeError, match=cpu):
        DO.render_depth({"cam": cam}, g, None, 1, time=0.5)             # (a view dict is unwrapped)
    assert DO.check_plane(0, 5) == "H and W must be > 0" and DO.check_batch(0, 5, 5) == "B must be > 0" and DO.check_plane(2 ** 16, 2 ** 15) == "H*W must be below 2^31"
    assert DO.DepthResult._fields == ("depth", "alpha", "valid")


def test_render_depths_signature_and_docstrings():
    from gaussianprediction_amd import eval_render as ER
    sig = inspect.signature(ER.render_depths)
    assert list(sig.parameters) == ["model_path", "name", "iteration", "views", "gaussians", "pipeline", "background", "mode", "near", "far", "alpha_min",
                                    "normals", "save_pfm", "save_ply", "writer", "video"]
    d = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert d == dict(mode="disparity", near=None, far=None, alpha_min=1e-3, normals=False, save_pfm=False, save_ply=False, writer=None, video=False)
    assert list(inspect.signature(DO.render_depth).parameters) == ["view", "gaussians", "pipeline", "iteration", "time", "alpha_min"]
    assert list(inspect.signature(DO.colorize).parameters) == ["depth", "valid", "mode", "near", "far", "lut", "background", "return_range"]
    assert list(inspect.signature(DO.unproject).parameters) == ["depth", "valid", "view", "image", "return_index"]
    assert list(inspect.signature(DO.depth_metrics).parameters) == ["pred", "gt", "mask", "align", "gt_min", "gt_max"]
    assert "only host read" in " ".join(DO.unproject.__doc__.split()) and "ONE render()" in DO.render_depth.__doc__
    assert "fixed" in ER.render_depths.__doc__ and "near" in ER.render_depths.__doc__
    src = inspect.getsource(ER)
    assert src.count("render_depths(") == 1                             # opt-in: no other loop calls it
