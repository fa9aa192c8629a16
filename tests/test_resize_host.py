"""No GPU: include/gp_resize.h against the binding's table; gp_resize_coeffs against the numpy restatement tests/resize_ref.py; that
restatement against Pillow itself; the kernels' programs (csrc/resize_core.h) run lane by lane on the CPU (tests/resize_emulate.cpp,
under the sanitizers where the host compiler can link them) against Pillow; the refusals that need no device.  Every comparison is
bit-exact."""
import ctypes as C
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import abi_check
import emulate_build
import resize_ref as ref
from gaussianprediction_amd import _lib, resize_ops as R

_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "gp_stream_t": _lib.Ptr}
_POINTEES = {"void", "uint8_t", "int32_t"}


def test_prototype_table_equals_the_header():
    protos = abi_check.check_table(R.ABI, 6, _SCALARS, _POINTEES)
    assert R.ABI.prototypes is R.PROTOTYPES and R.ABI.header == "gp_resize.h"
    assert protos["gp_resize_u8"][1][-1] == "gp_stream_t"          # the stream is the last parameter


def test_symbols_and_constants():
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_RESIZE_[A-Z0-9_]+) (\d+)\b", abi_check.header_text("gp_resize.h"))}
    assert defs["GP_RESIZE_ABI_VERSION"] == R.GP_RESIZE_ABI_VERSION == R.ABI.version == 1
    abi_check.check_applied(R.ABI)
    assert {k: defs["GP_RESIZE_" + k.upper()] for k in R.FILTERS} == R.FILTERS == ref.FILTERS
    from PIL import Image
    assert {k: int(getattr(Image.Resampling, k.upper())) for k in R.FILTERS} == R.FILTERS
    assert (defs["GP_RESIZE_DST_U8"], defs["GP_RESIZE_DST_F32"]) == (R.DST_U8, R.DST_F32) == (0, 1)
    assert [defs["GP_RESIZE_PATH_" + k] for k in ("COPY", "FUSED", "TWO_LAUNCH", "HORIZONTAL", "VERTICAL")] == \
        [R.PATH_COPY, R.PATH_FUSED, R.PATH_TWO_LAUNCH, R.PATH_HORIZONTAL, R.PATH_VERTICAL] == list(range(5))
    assert (defs["GP_RESIZE_TILE_W"], defs["GP_RESIZE_TILE_H"]) == (R.TILE_W, R.TILE_H)


PAIRS = [(i, o) for i in range(1, 41) for o in range(1, 41)] + [(1352, 676), (1014, 507), (135, 67), (600, 9), (9, 600)]


@pytest.mark.parametrize("name", list(ref.FILTERS))
def test_coefficients_equal_the_restatement(name):
    l, f = R.lib(), R.FILTERS[name]
    for n_in, n_out in PAIRS:
        want_b, want_k = ref.coeffs(n_in, n_out, name)
        assert l.gp_resize_ksize(n_in, n_out, f) == ref.ksize(n_in, n_out, name) == want_k.shape[1]
        got_b, got_k = R.coeffs(n_in, n_out, name)
        assert np.array_equal(got_b, want_b) and np.array_equal(got_k, want_k), (name, n_in, n_out)
        assert np.abs(want_k).max() < 1 << 23
    assert np.array_equal(R.coeffs(135, 67, f)[1], R.coeffs(135, 67, name.upper())[1])          # a name in any case, or Pillow's constant


# source W x H; the targets of one source: 1 x 1, small, vertical only, horizontal only, pure upscale, the reference's int(x * 0.5)
SOURCES = [(1, 1), (5, 7), (16, 16), (37, 23), (135, 101), (64, 200)]


def _targets(W, H):
    return [(1, 1), (2, 3), (W, max(1, H // 2)), (max(1, W // 3), H), (2 * W + 1, 2 * H + 3), (max(1, int(W * 0.5)), max(1, int(H * 0.5)))]


def _grid():
    seed = 0
    for name in ref.FILTERS:
        for Cn in (1, 3, 4):
            for W, H in SOURCES:
                for size in _targets(W, H):
                    seed += 1
                    yield name, Cn, W, H, size, seed


@pytest.mark.parametrize("name", list(ref.FILTERS))
def test_the_restatement_equals_pillow(name):
    """All 540 cases over the five runs: five filters, L / RGB / RGBA (alpha from {0, 1, 77, 200, 255}), six sources, six targets."""
    n = 0
    for flt, Cn, W, H, size, seed in _grid():
        if flt != name:
            continue
        img = ref.noise(Cn, H, W, seed)
        assert Cn != 4 or set(np.unique(img[3])) <= set(ref.ALPHAS)
        assert np.array_equal(ref.resize(img, size, name), ref.pillow(img, size, name)), (name, Cn, W, H, size)
        n += 1
    assert n == 108


def test_default_filter_and_copy_are_pillows():
    from PIL import Image
    img = ref.noise(4, 9, 11, 5)
    im = Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0)), "RGBA")
    assert np.array_equal(np.array(im.resize((5, 4))), np.array(im.resize((5, 4), Image.Resampling.BICUBIC)))      # no filter argument: bicubic
    assert np.array_equal(np.array(im.resize((11, 9))), np.array(im))                        # equal sizes: untouched, no alpha round trip
    assert not np.array_equal(ref.unpremultiply(ref.premultiply(img)), img)                  # ... which would have changed it


# ---- the kernels' programs on the CPU ----
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    """run(batch uint8 [B, C, H, W], size, name, alpha, dtype, src_gap, guard) -> (path, [B, C, Ho, Wo] numpy)."""
    d = tmp_path_factory.mktemp("resize_emulate")
    exe = emulate_build.build("resize_emulate", d, sanitize=True)

    def run(batch, size, name="bicubic", alpha=None, dtype=np.uint8, src_gap=0, guard=8):
        B, Cn, H, W = batch.shape
        Wo, Ho = size
        alpha = Cn == 4 if alpha is None else alpha
        job, out = str(d / "job.bin"), str(d / "out.bin")
        with open(job, "wb") as fp:
            fp.write(struct.pack("<11i", B, Cn, H, W, Ho, Wo, R.FILTERS[name], int(alpha), 0 if dtype == np.uint8 else 1, src_gap, guard))
            fp.write(np.ascontiguousarray(batch).tobytes())
        subprocess.check_call([exe, job, out], timeout=120)
        raw = open(out, "rb").read()
        (path,) = struct.unpack("<i", raw[:4])
        n = Cn * Ho * Wo
        slots = np.frombuffer(raw[4:], dtype=dtype).reshape(B, n + guard)
        assert (slots[:, n:].view(np.uint8) == 0xA5).all()              # the guard behind every slot
        return path, slots[:, :n].reshape(B, Cn, Ho, Wo)

    return run


@pytest.mark.parametrize("name", list(ref.FILTERS))
def test_emulated_kernels_against_pillow(emulator, name):
    """The 540-case grid again, through the programs the kernels run."""
    paths = set()
    for flt, Cn, W, H, size, seed in _grid():
        if flt != name:
            continue
        img = ref.noise(Cn, H, W, seed)
        path, got = emulator(img[None], size, name)
        assert path == R.path((W, H), size, name)
        assert np.array_equal(got[0], ref.pillow(img, size, name)), (name, Cn, W, H, size)
        paths.add(path)
    assert paths >= {R.PATH_COPY, R.PATH_FUSED, R.PATH_HORIZONTAL, R.PATH_VERTICAL}


# W x H -> W x H: the fused tile's edges from a source 2.3 times larger, the two-launch path, the reference's own rounding
EDGES = [((int(2.3 * w), int(2.3 * h)), (w, h)) for w, h in ((R.TILE_W - 1, R.TILE_H + 1), (R.TILE_W, R.TILE_H), (R.TILE_W + 1, R.TILE_H - 1),
                                                             (2 * R.TILE_W + 1, 2 * R.TILE_H + 1))]
LONG = [((600, 64), (9, 8)), ((64, 600), (8, 9))]


@pytest.mark.parametrize("Cn", [1, 3, 4])
def test_emulated_tile_edges_two_launch_path_batches_and_float(emulator, Cn):
    for k, (src, size) in enumerate(EDGES + LONG + [((135, 101), (67, 50)), ((16, 16), (33, 35))]):
        batch = np.stack([ref.noise(Cn, src[1], src[0], 100 * Cn + 10 * k + b) for b in range(2)])
        want = np.stack([ref.pillow(im, size) for im in batch])
        path, got = emulator(batch, size, src_gap=37)
        assert path == (R.PATH_TWO_LAUNCH if (src, size) in LONG else R.PATH_FUSED), (src, size)
        assert np.array_equal(got, want), (Cn, src, size)
        _, as_float = emulator(batch, size, dtype=np.float32, src_gap=5)
        unit = (torch.from_numpy(want).to(torch.float32) / 255.0).numpy()
        assert np.array_equal(as_float.view(np.uint32), unit.view(np.uint32)), (Cn, src, size)
    if Cn == 4:                                                          # alpha=False: four independent planes
        img = ref.noise(4, 23, 37, 9)
        _, got = emulator(img[None], (15, 11), alpha=False)
        assert np.array_equal(got[0], np.concatenate([ref.pillow(img[c:c + 1], (15, 11)) for c in range(4)]))


def test_the_path_boundary_is_the_window_byte_count():
    l = R.lib()
    assert R.path((1352, 1014), (676, 507)) == R.PATH_FUSED                                   # the workload: 9 taps an axis
    for name in ref.FILTERS:                                                                  # fused while the count fits, whatever the ratio
        seen = [R.path((4000, 4000), (o, o), name) for o in (2000, 400, 100, 40, 10)]
        assert seen == sorted(seen, key=lambda p: p == R.PATH_TWO_LAUNCH) and seen[0] == R.PATH_FUSED and seen[-1] == R.PATH_TWO_LAUNCH, (name, seen)
    assert l.gp_resize_scratch_bytes(2, 3, 64, 600, 8, 9, R.BICUBIC) == -(-2 * 3 * 64 * 9 // 256) * 256
    assert l.gp_resize_scratch_bytes(2, 3, 1014, 1352, 507, 676, R.BICUBIC) == 0


def test_c_entries_refuse_before_they_look_at_a_pointer():
    l = R.lib()
    assert l.gp_resize_ksize(1352, 676, R.BICUBIC) == 9 and l.gp_resize_ksize(16, 33, R.LANCZOS) == 7
    for bad, word in (((0, 4, R.BICUBIC), b"in = 0"), ((4, 0, R.BICUBIC), b"out = 0"), ((4, -1, R.BOX), b"out = -1"), ((4, 4, 0), b"filter = 0"),
                      ((4, 4, 6), b"filter = 6")):
        assert l.gp_resize_ksize(*bad) == -1 and word in l.gp_last_error(), bad
        assert l.gp_resize_coeffs(*bad, 8, 8) == 1 and word in l.gp_last_error(), bad
    assert l.gp_resize_coeffs(4, 2, R.BICUBIC, None, 8) == 1 and b"null" in l.gp_last_error()
    assert l.gp_resize_coeffs(4, 2, R.BICUBIC, 8, None) == 1 and b"null" in l.gp_last_error()
    for bad, word in (((0, 3, 4, 4, 2, 2, 3), b"B = 0"), ((1, 2, 4, 4, 2, 2, 3), b"C = 2"), ((1, 5, 4, 4, 2, 2, 3), b"C = 5"), ((1, 3, 0, 4, 2, 2, 3), b">= 1"),
                      ((1, 3, 4, 4, 2, 0, 3), b">= 1"), ((1, 3, 4, 4, 2, 2, 9), b"filter = 9"), ((1, 3, 4, 65536, 2, 2, 3), b"<= 65535"),
                      ((21846, 3, 4, 4, 2, 2, 3), b"B * C")):
        assert l.gp_resize_scratch_bytes(*bad) == -1 and word in l.gp_last_error(), bad
    assert l.gp_resize_path(0, 4, 2, 2, 3) == -1 and l.gp_resize_path(4, 4, 2, 2, 7) == -1 and b"filter = 7" in l.gp_last_error()

    def call(B=1, Cn=3, H=4, W=4, Ho=2, Wo=2, f=R.BICUBIC, src=1, sstride=48, xb=8, xk=8, xt=9, yb=8, yk=8, yt=9, alpha=0, kind=0, dst=4, dstride=12, scr=None):
        return l.gp_resize_u8(B, Cn, H, W, Ho, Wo, f, src, sstride, xb, xk, xt, yb, yk, yt, alpha, kind, dst, dstride, scr, None)

    for kw, word in ((dict(B=0), b"B = 0"), (dict(Cn=2), b"C = 2"), (dict(Cn=5), b"C = 5"), (dict(H=0), b">= 1"), (dict(Wo=0), b">= 1"), (dict(f=0), b"filter = 0"),
                     (dict(alpha=1), b"alpha_mode needs C = 4"), (dict(alpha=2), b"alpha_mode = 2"), (dict(kind=2), b"dst_kind = 2"),
                     (dict(sstride=47), b"src_stride"), (dict(dstride=11), b"dst_stride"), (dict(kind=1, dstride=47), b"dst_stride"),
                     (dict(kind=1, dstride=50), b"multiple of 4"), (dict(kind=1, dstride=48, dst=2), b"float32 dst"), (dict(xt=4), b"xtaps = 4"),
                     (dict(yt=5), b"ytaps = 5"), (dict(src=None), b"null"), (dict(dst=None), b"null"), (dict(xb=None), b"null"), (dict(yk=None), b"null"),
                     (dict(xk=6), b"4-byte"), (dict(H=600, W=64, Ho=9, Wo=8, sstride=3 * 600 * 64, dstride=3 * 72, xt=33, yt=269), b"null scratch")):
        assert call(**kw) == 1 and word in l.gp_last_error(), kw          # (nothing was launched: the pointers are not even memory)


def test_checked_before_the_device_and_before_any_launch(monkeypatch, tmp_path):
    from gaussianprediction_amd import jpeg_decode, png_decode
    monkeypatch.setattr(R, "lib", lambda: pytest.fail("a launch was reached"))
    img = torch.zeros(3, 8, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.resize(img, (4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        png_decode.decode([b""], device="cpu", resize=(4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        jpeg_decode.decode_files([tmp_path / "never-read.jpg"], device="cpu", resize=lambda w, h: (w // 2, h // 2))
    with pytest.raises(RuntimeError, match="not one of"):
        R.filter_id("nearest")
    with pytest.raises(RuntimeError, match="not one of"):
        R.filter_id(0)
    with pytest.raises(RuntimeError, match="not one of"):
        png_decode.decode([b""], device="cuda:0", resize=(4, 4), resample="cubic")
    assert R.filter_id("BICUBIC") == R.filter_id(3) == R.BICUBIC
    assert R.target_size(lambda w, h: (int(w * 0.5), int(h * 0.5)), 135, 101) == (67, 50) and R.target_size((3, 2), 9, 9) == (3, 2)
    with pytest.raises(ValueError, match=r"tiny\.png: 1 x 7 -> 0 x 3: a target size of 0"):
        R.target_size(lambda w, h: (int(w * 0.5), int(h * 0.5)), 1, 7, "tiny.png")
