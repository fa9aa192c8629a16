"""No GPU: csrc/gp_flow.h against the binding's table (a binding outside _lib.ABIS); the programs of csrc/flow_core.h in a stand-alone
build (tests/flow_emulate.cpp, under the sanitizers where the host compiler can link them) against the numpy restatement
tests/flow_ref.py on every case of tests/flow_cases.py -- bit for bit for project, resolve, warp, the counts and the maximum
magnitude, within the bars below for the colours and the float64 columns; the restatement's warp against torch's grid_sample and its
colours against the same formula in float64; the .flo files; the refusals that need no device."""
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
import flow_cases as cases
import flow_ref as ref
from gaussianprediction_amd import _lib, flow_ops as FO

_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "gp_stream_t": _lib.Ptr}
_POINTEES = {"float", "uint8_t", "double", "void"}
COLOUR_BAR = 1e-5            # atan2f is not correctly rounded on either side; the map is continuous in fk, so a floor that flips does not jump
F64_BAR = 1e-12              # relative: at most 3072 non-negative terms at 2^-53 each, about 3.4e-13


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def close64(got, want):
    """The float64 columns within F64_BAR relative; NaN where NaN and an infinity (3e38's magnitude) where there is one."""
    fin = np.isfinite(want)
    return same(got[~fin], want[~fin]) and bool((np.abs(got[fin] - want[fin]) <= F64_BAR * np.abs(want[fin])).all())


# ---- the header, the table, the registry ----
def test_prototype_table_equals_the_header_and_stays_out_of_the_registry():
    before = len(_lib.ABIS)
    protos = abi_check.check_table(FO.ABI, 7, _SCALARS, _POINTEES, {"gp_flow_view": FO.FlowViewC})
    assert FO.ABI.prototypes is FO.PROTOTYPES and FO.ABI not in _lib.ABIS and len(_lib.ABIS) == before
    assert os.path.samefile(os.path.join(abi_check.ROOT, "include", FO.ABI.header),
                            os.path.join(abi_check.ROOT, "gaussianprediction_amd", "csrc", "gp_flow.h"))
    for name in ("gp_flow_project", "gp_flow_resolve", "gp_flow_colorize", "gp_flow_metrics", "gp_flow_warp"):
        assert protos[name][1][-1] == "gp_stream_t"              # the stream is the last parameter
    assert not os.path.exists(os.path.join(abi_check.ROOT, "include", "gp_flow.h"))


def test_symbols_constants_and_the_struct():
    text = abi_check.header_text(FO.HEADER)
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_FLOW_[A-Z0-9_]+) +(\d+)", text)}
    assert defs["GP_FLOW_ABI_VERSION"] == FO.GP_FLOW_ABI_VERSION == FO.ABI.version == 1
    assert (defs["GP_FLOW_TILE"], defs["GP_FLOW_SUMS"], defs["GP_FLOW_COLUMNS"], defs["GP_FLOW_WHEEL"]) == (FO.TILE, FO.SUMS, FO.COLUMNS, FO.WHEEL)
    assert (ref.TILE, ref.SUMS, ref.COLUMNS, ref.WHEEL) == (FO.TILE, FO.SUMS, FO.COLUMNS, FO.WHEEL) and len(FO.METRIC_NAMES) == FO.COLUMNS
    abi_check.check_applied(FO.ABI)
    fields = re.search(r"typedef struct gp_flow_view \{(.*?)\}", text, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*[,;]", fields) == ["viewmatrix", "projmatrix", "W", "H"]
    assert [n for n, _ in FO.FlowViewC._fields_] == ["viewmatrix", "projmatrix", "W", "H"] and C.sizeof(FO.FlowViewC) == 24


# ---- the restatement's own pieces ----
def test_fma32_is_the_correctly_rounded_one():
    from fractions import Fraction
    rng = np.random.default_rng(1)
    a, b = rng.normal(size=4000).astype(np.float32), rng.normal(size=4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(np.float32)          # cancellation: the low bits of the product decide
    c[::2] = rng.normal(size=2000).astype(np.float32)
    got = ref.fma32(a, b, c)

    def exact(x, y, z):
        v = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo = np.float32(float(v))                                                     # (float(Fraction) rounds once, to 53 bits: a start)
        best = min((np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))),
                   key=lambda f: (abs(Fraction(float(f)) - v), int(np.float32(f).view(np.uint32)) & 1))
        return np.float32(best)

    assert all(got[i].tobytes() == exact(a[i], b[i], c[i]).tobytes() for i in range(0, 4000, 7))
    assert float(ref.fma32(np.float32(2.0 ** -30), np.float32(2.0 ** -30), np.float32(1.0))) == 1.0
    # a sum that float64 rounds to the tie of two float32 values, and float32 must then round up
    x = ref.fma32(np.float32(2.0 ** -12), np.float32(2.0 ** -12 + 2.0 ** -35), np.float32(1.0))          # 1 + 2^-24 + 2^-47: above the tie
    assert float(x) == 1.0 + 2.0 ** -23


def test_the_wheel_and_the_colours_against_float64():
    w = ref.wheel_bytes()
    assert w.shape == (55, 3) and w.min() == 0 and w.max() == 255
    assert w[0].tolist() == [255, 0, 0] and w[15].tolist() == [255, 255, 0] and w[21].tolist() == [0, 255, 0] and w[25].tolist() == [0, 255, 255]
    assert w[36].tolist() == [0, 0, 255] and w[49].tolist() == [255, 0, 255] and w[54].tolist() == [255, 0, 255 - 255 * 5 // 6]
    assert w[1].tolist() == [255, 17, 0] and w[35].tolist() == [0, 255 - 255 * 10 // 11, 255]
    rng = np.random.default_rng(2)
    flow = rng.normal(0, 2.0, (2, 25, 40)).astype(np.float32)
    a, _ = ref.colorize(flow, None, 3.0)
    b, _ = ref.colorize(flow, None, 3.0, dtype=np.float64)
    err = float(np.abs(a.astype(np.float64) - b).max())
    print("colour, float32 against float64:", err)
    assert a.dtype == np.float32 and b.dtype == np.float64 and err <= COLOUR_BAR
    assert 0.0 <= a.min() and a.max() <= 1.0
    zero, _ = ref.colorize(np.zeros((2, 2, 2), np.float32), None, 3.0)
    assert (zero == 1.0).all()                                                          # no motion is white
    # beyond the scale the colour is the wheel's, dimmed by 0.75: along +x the angle is that of row 0 after half a turn
    for vec in ((6.0, 0.0), (0.0, -6.0), (-4.5, 0.0)):
        f = np.array(vec, dtype=np.float32).reshape(2, 1, 1)
        far, _ = ref.colorize(f, None, 3.0)
        near, _ = ref.colorize(f / np.float32(np.hypot(*vec)) * np.float32(3.0), None, 3.0)   # the same direction at rad = 1: the pure wheel colour
        assert np.abs(far - np.float32(0.75) * near).max() <= 1e-6, vec
    left, _ = ref.colorize(np.array([-3.0, 0.0], np.float32).reshape(2, 1, 1), None, 3.0)     # atan2(-0, 3) = 0: fk = 27, between rows 27 and 28
    assert np.abs(left[:, 0, 0] - ref.wheel()[27]).max() <= 1e-6
    # the scale found on the way: the largest finite magnitude of the coloured pixels
    c = cases.FIELDS["17x13"]
    assert ref.max_magnitude(c.flow, c.valid) == np.float32(np.sqrt(np.float32(100.0 * 100.0 + 100.0 * 100.0)))
    assert ref.max_magnitude(c.flow) == ref.max_magnitude(c.flow, c.valid)                    # (3e38's magnitude is not finite)
    assert ref.max_magnitude(cases.FIELDS["all_zero_flow_17x13"].flow) == 0 and ref.max_magnitude(c.flow, np.zeros_like(c.valid)) == 0


def test_warp_against_grid_sample():
    c = cases.FIELDS["17x13"]
    flow = np.where(np.isfinite(c.flow), c.flow, np.float32(0.0))
    flow[np.abs(flow) > 1e3] = 0.0
    assert (c.H, c.W) == (13, 17) and np.abs(flow).max() == 100.0
    ours = ref.warp(c.image, flow)
    ys, xs = np.meshgrid(np.arange(c.H, dtype=np.float64), np.arange(c.W, dtype=np.float64), indexing="ij")
    grid = np.stack([2 * (xs + flow[0]) / (c.W - 1) - 1, 2 * (ys + flow[1]) / (c.H - 1) - 1], axis=-1)
    want = torch.nn.functional.grid_sample(torch.from_numpy(c.image)[None], torch.from_numpy(grid.astype(np.float32))[None], mode="bilinear",
                                           padding_mode="zeros", align_corners=True)[0].numpy()
    err = float(np.abs(ours - want).max())
    print("warp against grid_sample:", err)
    assert err <= 1e-5                                   # (grid_sample's normalised coordinates)
    assert (ours[:, 2, 2] == 0).all() and same(ours[:, 0, 0], c.image[:, 0, 0])          # out of the image; a zero flow copies
    x, y = 7 + int(flow[0, 4, 7]), 4 + int(flow[1, 4, 7])
    if 0 <= x < c.W and 0 <= y < c.H:
        assert same(ours[:, 4, 7], c.image[:, y, x])                                      # a position exactly on a pixel copies it


# ---- the programs in a stand-alone build, under the sanitizers ----
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    d = tmp_path_factory.mktemp("flow_emulate")
    exe = emulate_build.build("flow_emulate", d, sanitize=True)

    def run(head, arrays):
        job, out = str(d / "job.bin"), str(d / "out.bin")
        with open(job, "wb") as fp:
            fp.write(head)
            for a in arrays:
                if a is not None:
                    fp.write(np.ascontiguousarray(a).tobytes())
        subprocess.check_call([exe, job, out], timeout=120)
        return open(out, "rb").read()

    return run


@pytest.mark.parametrize("name", list(cases.PROJECT))
def test_emulated_projection_against_the_restatement(emulator, name):
    v0, v1, xyz0, xyz1 = cases.PROJECT[name]
    raw = emulator(struct.pack("<iiiiiq", 0, v0.W, v0.H, v1.W, v1.H, len(xyz0)), [v0.vm, v0.pm, v1.vm, v1.pm, xyz0, xyz1])
    got = np.frombuffer(raw, np.float32).reshape(-1, 3)
    assert same(got, cases.reference_project(name))


def test_the_projection_cases_reach_what_they_are_for():
    want = {n: cases.reference_project(n) for n in cases.PROJECT}
    for n, rows in want.items():
        assert set(np.unique(rows[:, 2])) <= {0.0, 1.0} and (rows[rows[:, 2] == 0] == 0).all(), n
    plain, rotated = want["N257_plain_17x13"], want["N257_rotated_64x48"]
    for rows in (plain, rotated):
        assert (rows[[3, 4, 7, 8, 9, 10], 2] == 0).all() and rows[:, 2].sum() > 200 and np.abs(rows[:, :2]).max() > 0.5
    assert (plain[[5, 6], 2] == 0).all()                                    # a depth of exactly 0.2 does not pass
    v0, _, xyz0, _ = cases.PROJECT["N257_plain_17x13"]
    assert float(xyz0[5, 2]) == float(np.float32(0.2)) and ref.pixel(v0, xyz0)[2][[11, 12]].all()
    z = want["zero_denominator"]
    assert z[:, 2].tolist() == [0, 1, 0, 0, 1, 0]                           # an infinite or NaN pixel at either end is no flow (w = 0 is finite)
    s = want["two_views_static_scene"]
    assert s[:, 2].sum() > 100 and np.median(np.hypot(s[:, 0], s[:, 1])) > 1.0   # the camera's motion alone moves the pixels


@pytest.mark.parametrize("name", list(cases.FIELDS))
def test_emulated_fields_against_the_restatement(emulator, name):
    c, want = cases.FIELDS[name], cases.reference_fields(name)
    plane = c.H * c.W
    raw = emulator(struct.pack("<iiif", 1, c.H, c.W, c.alpha_min), [c.composite])
    flow, alpha = np.frombuffer(raw, np.float32, 2 * plane).reshape(2, c.H, c.W), np.frombuffer(raw, np.float32, plane, 8 * plane).reshape(c.H, c.W)
    valid = np.frombuffer(raw, np.uint8, plane, 12 * plane).reshape(c.H, c.W)
    assert len(raw) == 13 * plane and same(flow, want.resolve[0]) and same(alpha, want.resolve[1]) and same(valid, want.resolve[2])
    for mode, max_flow, bg in cases.COLOUR_MODES:
        for masked in (False, True):
            raw = emulator(struct.pack("<iiiiffff", 2, c.H, c.W, int(masked), max_flow, *bg), [c.flow, c.valid if masked else None])
            scale, image = np.frombuffer(raw, np.float32, 1), np.frombuffer(raw, np.float32, 3 * plane, 4).reshape(3, c.H, c.W)
            want_image, want_scale = want.colour[(mode, masked)]
            assert scale[0].tobytes() == np.float32(want_scale).tobytes(), (mode, masked)
            err = float(np.abs(image - want_image).max())
            print(name, mode, masked, "colour error", err)
            assert err <= COLOUR_BAR and image.min() >= 0.0 and image.max() <= 1.0
            take = ref.coloured(c.flow, c.valid if masked else None)
            assert same(image[:, ~take], np.broadcast_to(np.array(bg, np.float32)[:, None], (3, int((~take).sum()))))
    for masked in (False, True):
        raw = emulator(struct.pack("<iiiii", 3, 1, c.H, c.W, int(masked)), [c.flow, c.gt, c.mask if masked else None])
        row = np.frombuffer(raw, np.float64).reshape(8)
        assert same(row[:1], want.metrics[masked][:1]) and close64(row, want.metrics[masked]), (masked, row, want.metrics[masked])
    for image, wanted in ((c.image, want.warp), (c.flow, want.warp_flow)):
        raw = emulator(struct.pack("<iiii", 4, image.shape[0], c.H, c.W), [image, c.flow])
        assert same(np.frombuffer(raw, np.float32).reshape(image.shape), wanted)


def test_the_field_cases_reach_what_they_are_for(emulator):
    c, want = cases.FIELDS["64x48"], cases.reference_fields("64x48")
    flow, alpha, valid = want.resolve
    assert valid[0, :3].tolist() == [0, 0, 1] and not valid[1, :6].any() and 0.9 < valid.mean() < 1.0
    assert (flow[:, valid == 0] == 0).all() and np.isfinite(flow).all() and np.isnan(alpha[1, 5])
    plain, masked = want.metrics[False], want.metrics[True]
    finite = np.isfinite(c.flow).all(axis=0) & np.isfinite(c.gt).all(axis=0)
    assert plain[0] == finite.sum() < c.H * c.W and masked[0] == (finite & (c.mask != 0)).sum() < plain[0]
    assert 1.0 > plain[2] > plain[3] > plain[4] > 0 and plain[3] >= plain[5] > 0 and plain[7] == 0
    with np.errstate(invalid="ignore"):
        e = np.sqrt(((c.flow.astype(np.float64) - c.gt) ** 2).sum(axis=0))[finite]
    assert abs(plain[1] - e.mean()) <= 1e-6 * e.mean() and abs(plain[3] - (e > 3).mean()) <= 2 / e.size
    nothing = cases.reference_fields("nothing_valid_17x13")
    assert np.isnan(nothing.metrics[True]).all() and not np.isnan(nothing.metrics[False]).any()
    assert (nothing.colour[("given", True)][0] == np.array([0.25, 0.5, 1.0], np.float32)[:, None, None]).all()
    # a batch's rows are the single images' rows, whatever else is in the batch
    a, b = cases.FIELDS["17x13"], cases.FIELDS["all_zero_flow_17x13"]
    raw = emulator(struct.pack("<iiiii", 3, 3, 13, 17, 1), [np.stack([a.flow, b.flow, a.flow]), np.stack([a.gt, b.gt, b.gt]), np.stack([a.mask, b.mask, b.mask])])
    table = np.frombuffer(raw, np.float64).reshape(3, 8)
    assert same(table, ref.metrics(np.stack([a.flow, b.flow, a.flow]), np.stack([a.gt, b.gt, b.gt]), np.stack([a.mask, b.mask, b.mask])))
    assert same(table[0], cases.reference_fields("17x13").metrics[True]) and same(table[1], cases.reference_fields("all_zero_flow_17x13").metrics[True])
    # more than 256 tiles: the finalising workgroup's lanes take more than one slot each
    rng = np.random.default_rng(5)
    flow, gt = rng.normal(0, 3, (1, 2, 520, 512)).astype(np.float32), rng.normal(0, 3, (1, 2, 520, 512)).astype(np.float32)
    raw = emulator(struct.pack("<iiiii", 3, 1, 520, 512, 0), [flow, gt])
    row, wanted = np.frombuffer(raw, np.float64), ref.metrics(flow, gt)[0]
    assert row[0] == 520 * 512 == wanted[0] and close64(row, wanted)


# ---- .flo files ----
def test_flo_files(tmp_path):
    flow = np.arange(12, dtype=np.float32).reshape(2, 2, 3) + np.float32(0.5)          # u = 0.5 .. 5.5, v = 6.5 .. 11.5; W = 3, H = 2
    path = tmp_path / "a.flo"
    FO.write_flo(path, torch.from_numpy(flow))
    want = b"PIEH" + struct.pack("<ii", 3, 2) + struct.pack("<12f", 0.5, 6.5, 1.5, 7.5, 2.5, 8.5, 3.5, 9.5, 4.5, 10.5, 5.5, 11.5)
    assert open(path, "rb").read() == want
    back = FO.read_flo(path)
    assert back.dtype == torch.float32 and back.shape == (2, 2, 3) and same(back.numpy(), flow)
    c = cases.FIELDS["17x13"]
    FO.write_flo(str(tmp_path / "b.flo"), c.flow)                                       # NaN, infinities and -0.0 survive
    assert same(FO.read_flo(str(tmp_path / "b.flo")).numpy(), c.flow)
    for bad in (b"PIEG" + want[4:], want[:-1], want + b"\0", want[:8], b"PIEH" + struct.pack("<ii", 0, 2)):
        (tmp_path / "bad.flo").write_bytes(bad)
        with pytest.raises(RuntimeError, match="read_flo"):
            FO.read_flo(tmp_path / "bad.flo")
    with pytest.raises(RuntimeError, match=r"\[2, H, W\]"):
        FO.write_flo(tmp_path / "c.flo", np.zeros((3, 2, 2), np.float32))


# ---- the refusals that need no device ----
def test_refusals_before_any_pointer_is_looked_at():
    l = FO.lib()
    view = FO.FlowViewC(8, 8, 17, 13)

    def refused(rc, word):
        assert rc == 1 and word in l.gp_last_error(), (word, l.gp_last_error())

    def project(v0=view, v1=view, xyz0=8, xyz1=8, N=5, out=8):
        return l.gp_flow_project(None if v0 is None else C.byref(v0), None if v1 is None else C.byref(v1), xyz0, xyz1, N, out, None)

    for kw, word in ((dict(N=-1), b"N must be"), (dict(N=2 ** 31), b"N must be"), (dict(v0=None), b"null"), (dict(v1=None), b"null"), (dict(xyz0=None), b"null"),
                     (dict(xyz1=None), b"null"), (dict(out=None), b"null"), (dict(v0=FO.FlowViewC(8, 8, 0, 13)), b"H and W"),
                     (dict(v1=FO.FlowViewC(8, 8, 17, -1)), b"H and W"), (dict(v0=FO.FlowViewC(0, 8, 17, 13)), b"null"), (dict(v1=FO.FlowViewC(8, 0, 17, 13)), b"null")):
        refused(project(**kw), word)
        if b"N must" in word:
            assert FO.check_points(kw["N"]).encode() in l.gp_last_error()
    assert project(N=0, xyz0=None, xyz1=None, out=None) == 0 and FO.check_points(0) is None and FO.check_points(2 ** 31 - 1) is None
    planes = ((dict(H=0), b"H and W"), (dict(W=-3), b"H and W"), (dict(H=2 ** 16, W=2 ** 15), b"H*W"))
    for kw, word in planes + ((dict(comp=None), b"null"), (dict(flow=None), b"null"), (dict(alpha=None), b"null"), (dict(valid=None), b"null"),
                              (dict(alpha_min=float("nan")), b"NaN")):
        a = dict(comp=8, alpha_min=1e-3, flow=8, alpha=8, valid=8, H=13, W=17)
        a.update(kw)
        refused(l.gp_flow_resolve(a["comp"], a["alpha_min"], a["flow"], a["alpha"], a["valid"], a["H"], a["W"], None), word)
        if kw in [p[0] for p in planes]:
            assert FO.check_plane(a["H"], a["W"]).encode() in l.gp_last_error()
    for kw, word in planes + ((dict(flow=None), b"null"), (dict(scale=None), b"null"), (dict(out=None), b"null"), (dict(max_flow=float("nan")), b"NaN")):
        a = dict(flow=8, valid=None, max_flow=0.0, scale=8, out=8, H=13, W=17)
        a.update(kw)
        refused(l.gp_flow_colorize(a["flow"], a["valid"], a["max_flow"], 0.0, 0.0, 0.0, a["scale"], a["out"], a["H"], a["W"], None), word)
    batches = planes + ((dict(B=0), b"B must be > 0"), (dict(B=65536), b"at most 65535"))
    for kw, word in batches + ((dict(flow=None), b"null"), (dict(gt=None), b"null"), (dict(scratch=None), b"null"), (dict(table=None), b"null"),
                               (dict(scratch=12), b"aligned")):
        a = dict(flow=8, gt=8, mask=None, B=2, H=13, W=17, scratch=8, table=8)
        a.update(kw)
        refused(l.gp_flow_metrics(a["flow"], a["gt"], a["mask"], a["B"], a["H"], a["W"], a["scratch"], a["table"], None), word)
        if kw in [p[0] for p in batches]:
            assert FO.check_batch(a["B"], a["H"], a["W"]).encode() in l.gp_last_error()
            assert l.gp_flow_metrics_scratch_bytes(a["B"], a["H"], a["W"]) == -1 and word in l.gp_last_error()
    assert l.gp_flow_metrics_scratch_bytes(2, 13, 17) == 2 * 1 * 7 * 8 and l.gp_flow_metrics_scratch_bytes(3, 48, 64) == 3 * 3 * 7 * 8
    assert l.gp_flow_metrics_scratch_bytes(1, 1025, 1) == 2 * 7 * 8 and FO.check_batch(65535, 1, 1) is None
    warps = planes + ((dict(Cn=0), b"C must be > 0"), (dict(Cn=3, H=2 ** 15, W=2 ** 15), b"C*H*W"))
    for kw, word in warps + ((dict(image=None), b"null"), (dict(flow=None), b"null"), (dict(out=None), b"null")):
        a = dict(image=8, flow=8, out=8, Cn=3, H=13, W=17)
        a.update(kw)
        refused(l.gp_flow_warp(a["image"], a["flow"], a["out"], a["Cn"], a["H"], a["W"], None), word)
        if kw in [p[0] for p in warps]:
            assert FO.check_warp(a["Cn"], a["H"], a["W"]).encode() in l.gp_last_error()
    assert FO.check_plane(13, 17) is None and FO.check_warp(1, 2 ** 15, 2 ** 15) is None and FO.check_warp(2, 2 ** 15, 2 ** 15) is not None


def test_the_python_surface_refuses_before_the_device(monkeypatch):
    monkeypatch.setattr(FO, "lib", lambda: pytest.fail("a launch was reached"))
    cpu = "no CPU fallback"
    flow, image = torch.zeros(2, 13, 17), torch.zeros(3, 13, 17)
    cam = cases.view(True, 17, 13).cam
    with pytest.raises(RuntimeError, match=cpu):
        FO.view_constants(cam)
    with pytest.raises(RuntimeError, match=r"\[4, 4\]"):
        FO.view_constants(SimpleNamespace(world_view_transform=torch.zeros(3, 4), full_proj_transform=torch.zeros(4, 4), image_width=17, image_height=13))
    for call, word in ((lambda: FO.screen_flow(torch.zeros(5, 3), torch.zeros(5, 3), cam), cpu), (lambda: FO.screen_flow(torch.zeros(5, 2), torch.zeros(5, 3), cam), r"\[N, 3\]"),
                       (lambda: FO.screen_flow(torch.zeros(5, 3, dtype=torch.float64), torch.zeros(5, 3), cam), "float32"),
                       (lambda: FO.resolve(image), cpu), (lambda: FO.resolve(flow), r"\[3, H, W\]"), (lambda: FO.resolve(image.double()), "float32"),
                       (lambda: FO.colorize(flow), cpu), (lambda: FO.colorize(image), r"\[2, H, W\]"), (lambda: FO.colorize(flow.half()), "float32"),
                       (lambda: FO.flow_metrics(flow, flow), cpu), (lambda: FO.flow_metrics(flow[None], flow[None]), cpu), (lambda: FO.flow_metrics(image, image), r"\[B, 2, H, W\]"),
                       (lambda: FO.flow_metrics(torch.zeros(2), flow), r"\[B, 2, H, W\]"),
                       (lambda: FO.warp(image, flow), cpu), (lambda: FO.warp(image[0], flow), r"\[C, H, W\]"), (lambda: FO.warp(image, flow[:1]), r"\[2, H, W\]"),
                       (lambda: FO.warp(image.long(), flow), "float32")):
        with pytest.raises(RuntimeError, match=word):
            call()
    g = SimpleNamespace(forward=lambda *a: pytest.fail("the model was evaluated"))
    with pytest.raises(RuntimeError, match=cpu):
        FO.render_flow(cam, g, None, 1, 0.0, 0.5)
    with pytest.raises(RuntimeError, match=cpu):
        FO.render_flow({"cam": cam}, g, None, 1, 0.0, 0.5)              # (an optical-flow dataset's view dict is unwrapped)
    assert FO.check_plane(0, 5) == "H and W must be > 0" and FO.check_batch(0, 5, 5) == "B must be > 0" and FO.check_warp(0, 5, 5) == "C must be > 0"
    assert FO.FlowResult._fields == ("flow", "alpha", "valid")


def test_render_flows_signature_and_docstrings():
    from gaussianprediction_amd import eval_render as ER
    sig = inspect.signature(ER.render_flows)
    assert list(sig.parameters) == ["model_path", "name", "iteration", "views", "gaussians", "pipeline", "background", "dt", "max_flow", "alpha_min",
                                    "save_flo", "writer", "video"]
    d = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert d == dict(dt=None, max_flow=None, alpha_min=1e-3, save_flo=False, writer=None, video=False)
    assert list(inspect.signature(FO.render_flow).parameters) == ["view", "gaussians", "pipeline", "iteration", "time0", "time1", "view1", "alpha_min"]
    assert list(inspect.signature(FO.colorize).parameters)[:4] == ["flow", "valid", "max_flow", "background"]
    assert "UNPINNED" in FO.__doc__ and "three deformation passes" in FO.render_flow.__doc__ and "occlusion" in FO.__doc__
    src = inspect.getsource(ER)
    assert src.count("render_flows(") == 1                              # opt-in: no other loop calls it
