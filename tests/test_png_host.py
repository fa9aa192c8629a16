"""No GPU: include/gp_png.h against the binding's table; the refusals that need no device; the PNG encoder's workgroup programs
(csrc/png_core.h) run lane by lane on the CPU (tests/png_emulate.cpp) with Pillow's and zlib's decoders as the oracle; video_schedule
against its formula; slerp / interpolation_pose against the reference's own results (tests/golden/pose_interpolation.npz)."""
import ctypes as C
import os
import re
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import abi_check
import png_cases as P
from gaussianprediction_amd import _lib, eval_render as ER, png_ops as PNG

HERE = os.path.dirname(os.path.abspath(__file__))

# ---- one signature per entry point, two statements of it: include/gp_png.h and png_ops.PROTOTYPES ----
_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "gp_stream_t": _lib.Ptr}
_POINTEES = {"void", "uint8_t", "uint32_t"}


def test_prototype_table_equals_the_header():
    protos = abi_check.check_table(PNG.ABI, 4, _SCALARS, _POINTEES)
    assert PNG.ABI.prototypes is PNG.PROTOTYPES and PNG.ABI.header == "gp_png.h"
    assert protos["gp_png_encode"][1][-1] == "gp_stream_t"         # the stream is the last parameter


def test_symbols_and_constants():
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_PNG_[A-Z0-9_]+) (\d+)u?\b", abi_check.header_text("gp_png.h"))}
    assert defs["GP_PNG_ABI_VERSION"] == PNG.GP_PNG_ABI_VERSION == PNG.ABI.version == 1
    abi_check.check_applied(PNG.ABI)
    assert (defs["GP_PNG_BAND_BYTES"], defs["GP_PNG_MAX_BATCH"], defs["GP_PNG_SRC_F32"], defs["GP_PNG_SRC_U8"], defs["GP_PNG_FILTER_NONE"]) == \
        (PNG.BAND_BYTES, PNG.MAX_BATCH, PNG.SRC_F32, PNG.SRC_U8, PNG.FILTER_NONE)
    assert PNG.BAND_BYTES >= 8192 and PNG.BAND_BYTES % 256 == 0


def _worst_case(H, W):
    S = H * (3 * W + 1)
    nb = -(-S // PNG.BAND_BYTES)
    return S + nb * (5 + 12) + 2 + 9 + 33 + 12


def test_bound_is_the_stored_worst_case_and_refuses_outside_the_limits():
    for H, W in ((1, 1), (37, 45), (163, 178), (1014, 1352), (1, 5000), (5000, 1)):
        b = PNG.bound(H, W)
        assert b % 8 == 0 and _worst_case(H, W) <= b < _worst_case(H, W) + 8, (H, W, b)
    assert 2 ** 31 - 2 ** 21 < PNG.bound(46300, 15433) < 2 ** 31            # the largest files: their length still fits an int32
    q = PNG.lib().gp_png_bound
    for bad, word in (((0, 4), b"H = 0"), ((4, 0), b"W = 0"), ((-1, 4), b"H = -1"), ((46340, 15446), b"2^31"), ((46341, 15447), b"2^31"), ((1, 715827883), b"2^31")):
        assert q(*bad) == -1 and word in PNG.lib().gp_last_error(), bad
        with pytest.raises(ValueError, match="png_ops.bound"):
            PNG.bound(*bad)
    s = PNG.lib().gp_png_scratch_bytes
    assert s(1, 163, 178) > 0 and s(32, 1014, 1352) < 1 << 29
    for bad, word in (((0, 4, 4), b"B = 0"), ((65536, 4, 4), b"B = 65536"), ((1, 0, 4), b"H = 0")):
        assert s(*bad) == -1 and word in PNG.lib().gp_last_error(), bad


def test_refusals_need_no_gpu():
    l = PNG.lib()
    big = PNG.bound(4, 4)
    for args, word in (((0, 4, 4, None, 0, 0, None, big, None, None, None), b"B = 0"), ((1, 4, 0, None, 0, 0, None, big, None, None, None), b"W = 0"),
                       ((1, 4, 4, None, 2, 0, None, big, None, None, None), b"src_kind = 2"), ((1, 4, 4, None, 0, 2, None, big, None, None, None), b"flag"),
                       ((1, 4, 4, None, 0, 0, None, big - 8, None, None, None), b"out_stride"), ((1, 4, 4, None, 0, 0, None, big, None, None, None), b"null")):
        assert l.gp_png_encode(*args) == 1 and word in l.gp_last_error(), args       # the C entry refuses before it looks at a pointer
    x = torch.zeros(3, 8, 8)
    for call in (lambda: PNG.encode(x), lambda: PNG.encode([x, x]), lambda: PNG.encode_to_bytes(x[None]), lambda: PNG.encode(x.to(torch.uint8))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    w = PNG.PngWriter()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        w.submit(x, "never-written.png")
    w.close()
    assert not [t for t in threading.enumerate() if t.name.startswith("PngWriter")]
    with pytest.raises(RuntimeError, match="closed"):
        w.submit(x, "never-written.png")


def test_shape_and_dtype_are_checked_before_the_device_and_any_launch(monkeypatch):
    monkeypatch.setattr(PNG, "lib", lambda: pytest.fail("a launch was reached"))
    for bad in (torch.zeros(8, 8), torch.zeros(1, 4, 8, 8), torch.zeros(3, 8, 8, dtype=torch.int32), torch.zeros(2, 2, 3, 8, 8),
                [torch.zeros(3, 8, 8), torch.zeros(3, 8, 9)], [torch.zeros(3, 8, 8), torch.zeros(3, 8, 8, dtype=torch.uint8)]):
        with pytest.raises(RuntimeError, match="images must be"):
            PNG.encode(bad)


# ---- the workgroup programs on the CPU ----
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return P.build_emulator(tmp_path_factory.mktemp("png_emulate"))


CASES = {name: (imgs, fnone) for name, imgs, fnone in P.cases(PNG.BAND_BYTES)}


@pytest.mark.parametrize("name", list(CASES))
def test_emulated_encoder_against_the_decoders(emulator, name):
    """Every case of the GPU test, through the same workgroup programs: Pillow and zlib decode the file to the quantised input, every
    CRC holds, the filter types are the header's rule, and the sizes meet the GPU test's conditions."""
    imgs, fnone = CASES[name]
    for img in imgs:
        want = P.quantise(img)
        _, H, W = want.shape
        data = emulator(img, fnone)
        assert len(data) <= PNG.bound(H, W)
        stream, payload, nidat = P.check_file(data, want, fnone)
        assert nidat == -(-len(stream) // PNG.BAND_BYTES)
        if not fnone:
            types = np.frombuffer(stream, dtype=np.uint8).reshape(H, 3 * W + 1)[:, 0]
            assert np.array_equal(types, P.best_filters(want))
        ratio = payload / P.rle_reference_bytes(stream, PNG.BAND_BYTES)
        print(f"{name}: {H}x{W} file {len(data)} B, IDAT payload {payload} B, {ratio:.4f} of zlib's Z_RLE over the same bands")
        if name.startswith(("disc", "ramp-300")):
            assert ratio <= 1.10
        if name.startswith("constant"):
            assert len(data) < H * 3 * W / 20
        if name == "zero-crc-slice":               # the crafted bytes sit on one lane's slice of the chunk kernel: its slice CRC is 0
            T = len(data) - 33 - 8 - 12            # type + data of the one IDAT chunk
            per = -(-T // 256)
            assert nidat == 1 and per == 4 and data[37 + 5 * per:37 + 6 * per] == P.ZERO_CRC


def test_the_cases_are_what_they_claim():
    band = PNG.BAND_BYTES
    img, k = P.fibonacci(band)
    assert k >= 18 and img.dtype == np.uint8
    first = np.concatenate([np.concatenate([[0], row]) for row in img.transpose(1, 2, 0).reshape(img.shape[1], -1)])[:band]
    counts = np.bincount(first, minlength=256)[1:k + 1]
    fib = [1, 1]
    while len(fib) < k:
        fib.append(fib[-1] + fib[-2])
    assert sorted(counts.tolist()) == fib and not (first[1:] == first[:-1]).any()
    H, W = P.one_band_plus_one(band)
    assert H * (3 * W + 1) == band + 1
    cut, lo, hi = P.run_across_cut(band, bounds=True)
    flat = np.concatenate([np.concatenate([[0], row]) for row in cut.transpose(1, 2, 0).reshape(cut.shape[1], -1)])
    assert lo < band - 2 and hi > band + 2 and (flat[lo:hi] == 77).all() and flat[lo - 1] != 77 and flat[hi] != 77
    assert len(np.unique(P.ramp(300, 400))) == 256
    x = P.edge_floats((3, 37, 45), 1)
    assert np.isnan(x).sum() == 1 and (x < 0).any() and (x[np.isfinite(x)] > 1).any()
    # the quantisation in numpy is the header's: one multiply, one add, floor, clamp, on float32
    assert P.quantise(np.array([0.3, -1.0, 2.0, np.nan, 1.0, -0.0, np.inf, 0.0019], dtype=np.float32)).tolist() == [77, 0, 255, 0, 255, 0, 255, 0]


# ---- the video schedule and the pose interpolation ----
@pytest.mark.parametrize("n,interpolation,step", [(1, 5, 1), (2, 5, 1), (7, 3, 2), (8, 3, 2)])
def test_video_schedule_against_the_formula(n, interpolation, step):
    frames = ER.video_schedule(n, interpolation, step)
    assert len(frames) == interpolation * ((n - 1) // step) + 1
    assert sorted(f[0] for f in frames) == list(range(len(frames)))            # unique, contiguous from 0
    assert frames[0][:3] == (0, 0, 0)
    want = [(0, 0, 0)]
    for idx in range(1, n):
        if idx % step == 0:
            want += [(frame + (idx // step - 1) * interpolation, idx - step, idx) for frame in range(1, interpolation + 1)]
    assert [f[:3] for f in frames] == want
    assert all(f[3] == frame / interpolation for f, frame in zip(frames[1:], list(range(1, interpolation + 1)) * n))
    with pytest.raises(ValueError):
        ER.video_schedule(0, 5, 1)


GOLD = np.load(os.path.join(HERE, "golden", "pose_interpolation.npz"))


def test_slerp_equals_the_reference():
    pairs, ratios, want, dots = GOLD["pairs"], GOLD["ratios"], GOLD["slerp"], GOLD["dots"]
    assert pairs.shape == (8, 2, 4) and len(ratios) == 4
    assert (np.abs(dots) > 0.9995).any() and ((dots < 0) & (np.abs(dots) <= 0.9995)).any()
    for i, (q0, q1) in enumerate(pairs):
        for j, t in enumerate(ratios):
            got = ER.slerp(float(t), q0, q1)
            assert got.dtype == np.float64 and np.abs(got - want[i, j]).max() <= 1e-12, (i, j)
            assert np.abs(ER.slerp(float(t), torch.from_numpy(q0), torch.from_numpy(q1)) - want[i, j]).max() <= 1e-12


def test_interpolation_pose_equals_the_reference():
    from pytorch3d.transforms import quaternion_to_matrix
    pairs, ratios, want, canonical = GOLD["pairs"], GOLD["ratios"], GOLD["slerp"], GOLD["canonical"]
    assert canonical.sum() >= 4
    rng = np.random.default_rng(4)
    for i in np.nonzero(canonical)[0]:
        R0, R1 = (quaternion_to_matrix(torch.from_numpy(q)).numpy() for q in pairs[i])
        prev, view = SimpleNamespace(R=R0, T=rng.normal(size=3)), SimpleNamespace(R=R1, T=rng.normal(size=3))
        for j, t in enumerate(ratios):
            new_t, new_R = ER.interpolation_pose(view, prev, float(t))
            assert np.abs(new_R - quaternion_to_matrix(torch.from_numpy(want[i, j])).numpy()).max() <= 1e-12, (i, j)
            assert np.array_equal(new_t, prev.T + (view.T - prev.T) * float(t))
