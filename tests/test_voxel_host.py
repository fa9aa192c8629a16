"""No GPU: include/gp_voxel.h against the binding's table; gp_voxel_downsample_host -- the programs of csrc/voxel_core.h on the CPU --
against the numpy restatement tests/voxel_ref.py; the same programs in a stand-alone build (tests/voxel_emulate.cpp, under the
sanitizers where the host compiler can link them); the refusals that need no device; the loop's voxel sizes; the PLY writer.  Every
comparison is bit-exact."""
import ctypes as C
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import abi_check
import emulate_build
import voxel_ref as ref
from gaussianprediction_amd import _lib, io_formats, voxel_ops as V

_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "gp_stream_t": _lib.Ptr}
_POINTEES = {"void", "double", "int32_t", "int64_t"}


def same(a, b):
    """Bit-equal arrays (or both None): the bytes, so that -0.0 and 0.0 differ and a NaN equals itself."""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_pass(got, points, voxel_size, colors, normals):
    want = ref.down_sample(points, voxel_size, colors, normals)
    assert len(got) == 4 and got[0].shape == want[0].shape, (got[0].shape, want[0].shape)
    assert same(got[3], want[3])
    for g, w in zip(got[:3], want[:3]):
        assert same(g, w)
    return want


def test_prototype_table_equals_the_header():
    protos = abi_check.check_table(V.ABI, 5, _SCALARS, _POINTEES)
    assert V.ABI.prototypes is V.PROTOTYPES and V.ABI.header == "gp_voxel.h"
    for name in ("gp_voxel_bounds", "gp_voxel_downsample"):
        assert protos[name][1][-1] == "gp_stream_t"              # the stream is the last parameter
    assert "gp_stream_t" not in protos["gp_voxel_downsample_host"][1]


def test_symbols_and_constants():
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_VOXEL_[A-Z0-9_]+) (\d+)\b", abi_check.header_text("gp_voxel.h"))}
    assert defs["GP_VOXEL_ABI_VERSION"] == V.GP_VOXEL_ABI_VERSION == V.ABI.version == 1
    abi_check.check_applied(V.ABI)
    assert defs["GP_VOXEL_RECORD_DOUBLES"] == V.RECORD_DOUBLES == 8


def test_the_restatement_sums_in_ascending_input_row():
    """np.add.at against the explicit loop, and the order against a sort of tuples."""
    pts, col, nrm = ref.surface(700, 3, "xyz+colors+normals")
    got = ref.down_sample(pts, 0.1, col, nrm)
    index = np.floor((pts - (pts.min(axis=0) - 0.1 / 2)) / 0.1).astype(np.int32)
    cells = sorted(set(map(tuple, index)))
    assert [tuple(r) for r in got[3]] == cells and 1 < len(cells) < 700
    for a, g in zip((pts, col, nrm), got[:3]):
        want = np.empty_like(g)
        for v, cell in enumerate(cells):
            s, k = np.zeros(3), 0
            for i in range(len(pts)):
                if tuple(index[i]) == cell:
                    s, k = s + a[i], k + 1
            want[v] = s / float(k)
        assert same(g, want)


@pytest.mark.parametrize("attrs", ref.ATTRS)
@pytest.mark.parametrize("n", ref.SIZES)
def test_host_pass_equals_the_restatement(n, attrs):
    pts, col, nrm, vs = ref.size_case(n, attrs)
    want = check_pass(V.host_pass(pts, vs, col, nrm, return_index=True), pts, vs, col, nrm)
    assert n < 1000 or 1 < len(want[0]) < n


@pytest.mark.parametrize("name", list(ref.special_cases()))
def test_host_pass_on_boundaries_and_degenerate_clouds(name):
    pts, col, nrm, vs = ref.special_cases()[name]
    want = check_pass(V.host_pass(pts, vs, col, nrm, return_index=True), pts, vs, col, nrm)
    m, top = len(want[0]), want[3].max(axis=0)
    if name in ("boundary", "negative_boundary"):
        q = (pts - (pts.min(axis=0) - vs / 2)) / vs
        assert (q == np.floor(q)).all(axis=1).sum() > 400              # points exactly on voxel boundaries ...
        assert len(np.unique(pts, axis=0)) < len(pts)                  # ... duplicated points ...
        assert name == "boundary" or (pts < 0).any()                   # ... negative coordinates
    assert {"one_voxel": m == 1 and len(pts) == 5000, "own_voxel": m == len(pts), "wide_x": top[0] > 65535 and 255 < top[1] < 65536,
            "wide_xyz": (top > 65535).all(), "wide_far": (top > 2 ** 22).all()}.get(name, True)


def test_host_loop_takes_the_eleven_passes():
    pts = ref.loop_cloud()
    want_cloud, want_passes = ref.until(pts, max_points=500)
    assert [c for _, c in want_passes] == ref.LOOP_COUNTS and len(want_cloud[0]) == 451
    cloud, passes = V._loop(V.host_pass, (pts, None, None), 500, 0.02, 0.01)
    assert passes == want_passes and same(cloud[0], want_cloud[0]) and cloud[1] is None and cloud[2] is None


def test_voxel_sizes_accumulate_as_the_script_does():
    want, v = [], 0.02
    for _ in range(11):
        want.append(v)
        v += 0.01
    assert want[4] == 0.060000000000000005 != 0.06
    assert [s for s, _ in V._loop(V.host_pass, (ref.loop_cloud(), None, None), 500, 0.02, 0.01)[1]] == want[:11]


def test_empty_cloud_and_refusals_of_the_host_entry():
    out = V.host_pass(np.empty((0, 3)), 0.02, np.empty((0, 3)), None, return_index=True)
    assert out[0].shape == (0, 3) and out[1].shape == (0, 3) and out[2] is None and out[3].shape == (0, 3)
    pts = ref.surface(50, 1)[0]
    for vs in (0.0, -0.02, float("nan")):
        with pytest.raises(_lib.GpHipError, match="voxel_size <= 0"):
            V.host_pass(pts, vs)
        with pytest.raises(ValueError):
            ref.down_sample(pts, vs)
    far = np.array([[0.0, 0.0, 0.0], [1.0, 3.0e6, 0.0]])               # 3e6 / 1e-3 = 3e9 cells: beyond int32
    with pytest.raises(_lib.GpHipError, match="voxel_size is too small"):
        V.host_pass(far, 1e-3)
    with pytest.raises(ValueError, match="too small"):
        ref.down_sample(far, 1e-3)
    assert len(V.host_pass(far, 2e-3)[0]) == 2                          # ... and 1.5e9 is not
    for bad in (float("nan"), float("inf"), -float("inf")):
        p = pts.copy()
        p[17, 1] = bad
        with pytest.raises(_lib.GpHipError, match="not finite"):
            V.host_pass(p, 0.02)
    l = V.lib()
    assert l.gp_voxel_scratch_bytes(-1) == -1 and l.gp_voxel_scratch_bytes(2 ** 31 - 1) == -1 and b"2^31" in l.gp_last_error()
    assert l.gp_voxel_scratch_bytes(2 ** 31 - 2) > 0 and l.gp_voxel_scratch_bytes(0) >= 0 and l.gp_voxel_scratch_bytes(1000) % 256 == 0
    m = C.c_int64(-1)
    assert l.gp_voxel_downsample_host(2 ** 31 - 1, 8, None, None, 0.02, 8, None, None, 8, C.byref(m)) == 1 and b"2^31" in l.gp_last_error()
    assert l.gp_voxel_downsample_host(3, 8, 8, None, 0.02, 8, None, None, 8, C.byref(m)) == 1 and b"come together" in l.gp_last_error()


def test_device_entries_refuse_before_they_look_at_a_pointer():
    l = V.lib()
    assert l.gp_voxel_bounds(0, 8, 8, 8, None) == 1 and b"2^31" in l.gp_last_error()
    assert l.gp_voxel_bounds(2 ** 31 - 1, 8, 8, 8, None) == 1
    assert l.gp_voxel_bounds(5, None, 8, 8, None) == 1 and b"null" in l.gp_last_error()
    rec = np.array([0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0])

    def call(n=5, pts=8, col=None, nrm=None, vs=0.02, bounds=rec, out_p=8, out_c=None, out_n=None, out_i=8, m=8, scr=8):
        return l.gp_voxel_downsample(n, pts, col, nrm, vs, None if bounds is None else bounds.ctypes.data, out_p, out_c, out_n, out_i, m, scr, None)

    flagged, wide, upside = rec.copy(), rec.copy(), rec.copy()
    flagged[6], wide[3], upside[0] = 1.0, 1.0e9, 2.0
    for kw, word in ((dict(vs=0.0), b"voxel_size <= 0"), (dict(vs=-1.0), b"voxel_size <= 0"), (dict(n=-1), b"2^31"), (dict(n=2 ** 31 - 1), b"2^31"),
                     (dict(m=None), b"null"), (dict(pts=None), b"null"), (dict(bounds=None), b"null"), (dict(out_i=None), b"null"), (dict(scr=None), b"null"),
                     (dict(col=8), b"come together"), (dict(out_n=8), b"come together"), (dict(bounds=flagged), b"not finite"),
                     (dict(bounds=wide), b"voxel_size is too small"), (dict(bounds=upside), b"bounds are not")):
        assert call(**kw) == 1 and word in l.gp_last_error(), kw          # (nothing was launched: the pointers are not even memory)


def test_checked_before_the_device_and_before_any_launch(monkeypatch, tmp_path):
    monkeypatch.setattr(V, "lib", lambda: pytest.fail("a launch was reached"))
    pts = torch.zeros(8, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.voxel_down_sample(pts, 0.02)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.downsample_until(pts)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.downsample_ply(tmp_path / "never-read.ply", tmp_path / "never-written.ply", device="cpu")
    with pytest.raises(RuntimeError, match="must be a tensor"):
        V.voxel_down_sample(np.zeros((8, 3)), 0.02)


def test_ply_round_trip_and_colour_bytes(tmp_path):
    rng = np.random.default_rng(4)
    pts, nrm = rng.normal(size=(257, 3)), rng.normal(size=(257, 3))
    col = rng.uniform(-0.2, 1.2, (257, 3))
    col[:6] = [[0.0, 1.0, 0.5], [127.5 / 255, 128.5 / 255, 0.4999 / 255], [-1.0, 2.0, 1e-9], [1 / 255, 254 / 255, 254.5 / 255], [0.5 / 255, 1.5 / 255, 2.5 / 255],
               [0.999, 0.001, 0.25]]
    want_bytes = np.round(np.clip(col, 0, 1) * 255).astype(np.uint8)
    assert same(io_formats.color_to_uint8(col), want_bytes) and want_bytes.min() == 0 and want_bytes.max() == 255
    for name, c, n in (("full", col, nrm), ("xyz", None, None), ("colors", col, None), ("normals", None, nrm)):
        path = tmp_path / f"{name}.ply"
        io_formats.save_point_cloud_ply(path, pts, c, n)
        v = io_formats.read_ply_vertices(path)
        want_names = ["x", "y", "z"] + (["nx", "ny", "nz"] if n is not None else []) + (["red", "green", "blue"] if c is not None else [])
        assert list(v.dtype.names) == want_names and len(v) == 257
        assert all(v.dtype[k] == np.dtype("<f8") for k in want_names[:-3 if c is not None else None])
        assert open(path, "rb").read().startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 257\nproperty double x\n")
        got = V.read_point_cloud_ply(path)
        assert same(got[0], pts) and same(got[2], n)
        if c is None:
            assert got[1] is None
        else:
            assert v.dtype["red"] == np.dtype("u1") and same(np.stack([v["red"], v["green"], v["blue"]], axis=1), want_bytes)
            assert same(got[1], want_bytes.astype(np.float64) / 255.0)
    # the reference's reader: vertices['x'] .. ['red'] / 255.0 .. ['nx']
    v = io_formats.read_ply_vertices(tmp_path / "full.ply")
    assert same(np.vstack([v["x"], v["y"], v["z"]]).T, pts) and same(np.vstack([v["nx"], v["ny"], v["nz"]]).T, nrm)
    with pytest.raises(ValueError, match="are"):
        io_formats.save_point_cloud_ply(tmp_path / "bad.ply", pts, col[:5], None)


# ---- the programs in a stand-alone build, under the sanitizers ----
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    """run(points, voxel_size, colors, normals) -> (points, colors, normals, index), or the refusal's code as an int."""
    d = tmp_path_factory.mktemp("voxel_emulate")
    exe = emulate_build.build("voxel_emulate", d, sanitize=True)

    def run(points, voxel_size, colors=None, normals=None):
        n = len(points)
        job, out = str(d / "job.bin"), str(d / "out.bin")
        with open(job, "wb") as fp:
            fp.write(struct.pack("<qiid", n, int(colors is not None), int(normals is not None), voxel_size))
            for a in (points, colors, normals):
                if a is not None:
                    fp.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        subprocess.check_call([exe, job, out], timeout=120)
        raw = open(out, "rb").read()
        rc, m = struct.unpack("<iq", raw[:12])
        if rc:
            return rc
        got, off = [], 12
        for a in (points, colors, normals):
            got.append(None if a is None else np.frombuffer(raw, np.float64, m * 3, off).reshape(m, 3))
            off += 0 if a is None else m * 24
        return tuple(got) + (np.frombuffer(raw, np.int32, m * 3, off).reshape(m, 3),)

    return run


def test_emulated_programs_against_the_restatement(emulator):
    for n in ref.SIZES[:-2]:
        for attrs in ref.ATTRS:
            pts, col, nrm, vs = ref.size_case(n, attrs)
            check_pass(emulator(pts, vs, col, nrm), pts, vs, col, nrm)
    for name, (pts, col, nrm, vs) in ref.special_cases().items():
        check_pass(emulator(pts, vs, col, nrm), pts, vs, col, nrm)
    pts = ref.surface(50, 1)[0]
    bad = pts.copy()
    bad[3, 2] = float("nan")
    assert emulator(pts, 0.0) == 1 and emulator(bad, 0.02) == 3 and emulator(np.array([[0.0, 0.0, 0.0], [1.0, 3.0e6, 0.0]]), 1e-3) == 4
    assert emulator(np.empty((0, 3)), 0.02)[3].shape == (0, 3)
