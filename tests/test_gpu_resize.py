"""Image resizing on the device (include/gp_resize.h, resize_ops): byte for byte what Pillow's Image.resize returns -- the smallest
cases, the fused path's tile edges, an upscale, the reference's own rounding, the two-launch path, all five filters, L / RGB / RGBA,
batches with a free batch stride, both destination kinds, the workload's shape; the decoders' resize= against Pillow-open followed by
Pillow-resize; and evaluate_dirs(resize=True) equal, number for number, to scoring files that Pillow resized on the host.  Sizes are
W x H.  A test that ends in a device error is the last one of this module to launch anything."""
import contextlib
import os

import numpy as np
import pytest
import torch

import resize_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_DEVICE_ERROR = []


@pytest.fixture(autouse=True)
def _nothing_is_launched_after_a_device_error():
    if _DEVICE_ERROR:
        pytest.fail(f"not run: an earlier test of this module ended in a device error ({_DEVICE_ERROR[0]})")
    yield


@contextlib.contextmanager
def device_work():
    """Everything that launches runs inside: the device has finished when the block ends, and an error that is not a failed
    comparison keeps the rest of the module from launching."""
    try:
        yield
        torch.cuda.synchronize()
    except AssertionError:
        raise
    except Exception as e:
        _DEVICE_ERROR.append(f"{type(e).__name__}: {e}")
        raise


@pytest.fixture(scope="module")
def R():
    from gaussianprediction_amd import resize_ops
    return resize_ops


def _edges(R):
    sizes = [(R.TILE_W - 1, R.TILE_H - 1), (R.TILE_W, R.TILE_H), (R.TILE_W + 1, R.TILE_H + 1), (2 * R.TILE_W + 1, 2 * R.TILE_H + 1),
             (R.TILE_W - 1, R.TILE_H + 1), (R.TILE_W + 1, R.TILE_H - 1)]
    return [((int(2.3 * w), int(2.3 * h)), (w, h)) for w, h in sizes]


SMALL = [((1, 1), (1, 1)), ((1, 1), (3, 2)), ((5, 7), (2, 3)), ((5, 7), (5, 3)), ((5, 7), (2, 7))]
LONG = [((600, 64), (9, 8)), ((64, 600), (8, 9))]
OTHER = [((16, 16), (33, 35)), ((135, 101), (67, 50))] + LONG


def _strided(batch, gap):
    """[B, C, H, W] uint8 numpy -> the same images on the device, `gap` bytes between one image and the next."""
    B, n = batch.shape[0], batch[0].size
    buf = torch.full((B, n + gap), 0x5A, dtype=torch.uint8, device=DEV)
    buf[:, :n] = torch.from_numpy(batch.reshape(B, n)).to(DEV)
    x = buf[:, :n].view(batch.shape)
    assert gap == 0 or not x.is_contiguous()
    return x


def _check(R, src, size, name, Cn, seed, every_form):
    """B = 3 with a free batch stride as uint8; B = 1 as float32; with every_form also B = 1 as uint8, B = 3 as float32 into `out=`."""
    (W, H) = src
    batch = np.stack([ref.noise(Cn, H, W, seed + b) for b in range(3)])
    want = np.stack([ref.pillow(im, size, name) for im in batch])
    unit = torch.from_numpy(want).to(torch.float32) / 255.0
    x = _strided(batch, 13)
    got = R.resize(x, size, name)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), (src, size, name, Cn)
    one = R.resize(x[1], size, R.FILTERS[name], dtype=torch.float32)                     # [C, H, W] in, Pillow's constant
    assert one.dtype == torch.float32 and torch.equal(one.cpu(), unit[1]), (src, size, name, Cn)
    if every_form:
        assert np.array_equal(R.resize(x[2:], size, name).cpu().numpy(), want[2:])
        slots = torch.full((3, want[0].size + 5), -1.0, dtype=torch.float32, device=DEV)
        out = slots[:, :want[0].size].view(want.shape)
        assert R.resize(x, size, name, dtype=torch.float32, out=out) is out
        assert torch.equal(out.cpu(), unit) and bool((slots[:, want[0].size:] == -1.0).all()), (src, size, name, Cn)
    return R.path(src, size, name)


@pytest.mark.parametrize("name", list(ref.FILTERS))
def test_smallest_and_tile_edge_cases_equal_pillow(R, name):
    paths = set()
    with device_work():
        for k, (src, size) in enumerate(SMALL + _edges(R)):
            for Cn in (1, 3, 4):
                paths.add(_check(R, src, size, name, Cn, 1000 * k + 10 * Cn, every_form=name == "bicubic"))
    assert paths == {R.PATH_COPY, R.PATH_FUSED, R.PATH_HORIZONTAL, R.PATH_VERTICAL}


def test_upscale_reference_rounding_and_the_two_launch_path(R):
    paths = []
    with device_work():
        for k, (src, size) in enumerate(OTHER):
            for Cn in (1, 3, 4):
                paths.append(_check(R, src, size, "bicubic", Cn, 50000 + 1000 * k + 10 * Cn, every_form=True))
    assert paths == [R.PATH_FUSED] * 6 + [R.PATH_TWO_LAUNCH] * 6
    seen = {R.path(src, size) for src, size in SMALL + _edges(R) + OTHER}
    assert seen == {R.PATH_COPY, R.PATH_FUSED, R.PATH_TWO_LAUNCH, R.PATH_HORIZONTAL, R.PATH_VERTICAL}       # every path was entered


def test_alpha_off_contiguous_input_and_two_calls(R):
    img = ref.noise(4, 23, 37, 7)
    with device_work():
        x = torch.from_numpy(img).to(DEV)
        plain = R.resize(x, (15, 11), alpha=False)
        assert np.array_equal(plain.cpu().numpy(), np.concatenate([ref.pillow(img[c:c + 1], (15, 11)) for c in range(4)]))
        a, b = R.resize(x, (15, 11)), R.resize(x, (15, 11))
        assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), ref.pillow(img, (15, 11)))
        flipped = x.flip(2)                                                              # not contiguous inside an image: copied first
        assert np.array_equal(R.resize(flipped, (15, 11)).cpu().numpy(), ref.pillow(np.ascontiguousarray(img[:, :, ::-1]), (15, 11)))


def test_arguments_are_refused_by_name(R):
    x = torch.zeros(3, 8, 8, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="torch.float32"):
        R.resize(x.float(), (4, 4))
    with pytest.raises(RuntimeError, match="torch.float16"):
        R.resize(x, (4, 4), dtype=torch.float16)
    with pytest.raises(RuntimeError, match="C = 1, 3 or 4"):
        R.resize(x[:2], (4, 4))
    with pytest.raises(RuntimeError, match="alpha needs four planes"):
        R.resize(x, (4, 4), alpha=True)
    with pytest.raises(ValueError, match="a target size of 0"):
        R.resize(x, (0, 4))
    with pytest.raises(RuntimeError, match="out must be"):
        R.resize(x, (4, 4), out=torch.empty(3, 4, 5, dtype=torch.uint8, device=DEV))


def test_the_workloads_shape(R):
    batch = np.stack([ref.noise(3, 1014, 1352, 90 + b) for b in range(2)])
    want = np.stack([ref.pillow(im, (676, 507)) for im in batch])
    assert R.path((1352, 1014), (676, 507)) == R.PATH_FUSED
    with device_work():
        got = R.resize(torch.from_numpy(batch).to(DEV), (676, 507))
        assert np.array_equal(got.cpu().numpy(), want)


def _half(w, h):
    return int(w * 0.5), int(h * 0.5)


def _pillow_file(path, size):
    """Pillow-open followed by Pillow-resize, planar."""
    from PIL import Image
    im = Image.open(path)
    arr = np.array(im.resize(size(*im.size) if callable(size) else size))
    return arr[None] if arr.ndim == 2 else np.ascontiguousarray(arr.transpose(2, 0, 1))


def test_the_decoders_resize_equals_pillow_open_and_resize(R, tmp_path):
    from PIL import Image
    from gaussianprediction_amd import jpeg_decode, png_decode
    pngs = []
    for k, (Cn, W, H) in enumerate([(3, 37, 23), (3, 37, 23), (1, 20, 31), (4, 19, 17), (3, 70, 41)]):
        img = ref.noise(Cn, H, W, 300 + k)
        path = str(tmp_path / f"{k}.png")
        Image.fromarray(img[0] if Cn == 1 else np.ascontiguousarray(img.transpose(1, 2, 0))).save(path)
        pngs.append(path)
    jpgs = []
    for k, (W, H) in enumerate([(48, 40), (48, 40), (35, 29)]):
        img = np.clip(np.add.outer(np.arange(H) * 3, np.arange(W) * 2)[None] + ref.noise(3, H, W, 400 + k) // 8, 0, 255).astype(np.uint8)
        path = str(tmp_path / f"{k}.jpg")
        Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0))).save(path, quality=92, subsampling=2 if k % 2 else 0)
        jpgs.append(path)
    with device_work():
        for size in (_half, (10, 9)):
            got = png_decode.decode_files(pngs, device=DEV, resize=size)
            three = png_decode.decode_files(pngs, device=DEV, resize=size, channels=3, dtype=torch.float32)
            for path, g, t in zip(pngs, got, three):
                want = _pillow_file(path, size)
                assert g.dtype == torch.uint8 and np.array_equal(g.cpu().numpy(), want), (path, size)
                assert torch.equal(t.cpu(), torch.from_numpy(want[:3]).to(torch.float32) / 255.0), (path, size)     # [:3] follows .resize
            assert three[3].shape[0] == 3 and got[3].shape[0] == 4                          # the RGBA file: its alpha plane was resized with it
            for sync in (False, True):
                got = jpeg_decode.decode_files(jpgs, device=DEV, resize=size, sync=sync)
                for path, g in zip(jpgs, got):
                    assert np.array_equal(g.cpu().numpy(), _pillow_file(path, size)), (path, size)
        lanczos = png_decode.decode_files(pngs[:1], device=DEV, resize=(11, 7), resample="lanczos")[0]
        assert np.array_equal(lanczos.cpu().numpy(), ref.pillow(_pillow_file(pngs[0], (37, 23)), (11, 7), "lanczos"))
        # a background composites the RESIZED RGBA image, by the reader's formula in float64
        bg = torch.tensor([1.0, 0.5, 0.0], device=DEV)
        (comp,) = png_decode.decode_files(pngs[3:4], device=DEV, resize=_half, background=bg)
        small = _pillow_file(pngs[3], _half).astype(np.float64) / 255.0
        arr = small[:3] * small[3:4] + bg.cpu().numpy().astype(np.float64).reshape(3, 1, 1) * (1 - small[3:4])
        want = np.array(arr * 255.0, dtype=np.byte).view(np.uint8)
        assert np.array_equal(comp.cpu().numpy(), want)
        (comp32,) = png_decode.decode_files(pngs[3:4], device=DEV, resize=_half, background=bg, dtype=torch.float32)
        assert torch.equal(comp32.cpu(), torch.from_numpy(want).to(torch.float32) / 255.0)
    with pytest.raises(ValueError, match=r"0\.png: 37 x 23 -> 1 x 0: a target size of 0"):
        png_decode.decode_files(pngs, device=DEV, resize=lambda w, h: (w // 30, h // 30))


def test_decode_avi_with_resize_equals_pillow_frame_by_frame(R, tmp_path):
    import io
    from PIL import Image
    from gaussianprediction_amd import jpeg_decode, jpeg_ops
    from jpeg_ref import riff_walk
    yy, xx = np.mgrid[:80, :96]
    frames = np.stack([np.stack([(xx * (s + 1) + yy) % 256, (yy * 2 + xx * s) % 256, (xx + yy) % 256]) for s in range(3)]).astype(np.uint8)
    path = tmp_path / "v.avi"
    with device_work():
        vw = jpeg_ops.VideoWriter(path, 24)
        vw.submit(torch.from_numpy(frames).to(DEV))
        vw.close()
        got = jpeg_decode.decode_avi(path, device=DEV, resize=_half, frames=[2, 0], dtype=torch.float32)
    files = [f for _, f in riff_walk(path.read_bytes())["frames"]]
    want = np.stack([np.array(Image.open(io.BytesIO(bytes(files[k]))).resize((48, 40))).transpose(2, 0, 1) for k in (2, 0)])
    assert got.shape == (2, 3, 40, 48) and torch.equal(got.cpu(), torch.from_numpy(want).to(torch.float32) / 255.0)


@pytest.fixture(scope="module")
def render_dirs(tmp_path_factory):
    """<full>/m/{renders,gt}: 3 PNG pairs (one of them RGBA renders); <half>/m/...: the same files resized by Pillow and saved."""
    from PIL import Image
    full, half = tmp_path_factory.mktemp("full"), tmp_path_factory.mktemp("half")
    W, H = 341, 333                                                                      # -> 170 x 166: MS-SSIM needs more than 160
    yy, xx = np.mgrid[:H, :W]
    for i in range(3):
        base = np.stack([(xx * (i + 2) + yy) % 256, (yy * 2 + xx * i) % 256, (xx + yy * (i + 1)) % 256]).astype(np.uint8)
        for sub, seed in (("renders", 500 + i), ("gt", 600 + i)):
            img = (base // 2 + ref.noise(3, H, W, seed) // 3).astype(np.uint8)
            if sub == "renders" and i == 1:
                img = np.concatenate([img, ref.noise(4, H, W, seed)[3:]])                 # an RGBA render: [:3] follows the resize
            for root in (full, half):
                os.makedirs(root / "m" / sub, exist_ok=True)
            im = Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0)))
            im.save(full / "m" / sub / f"{i:05d}.png")
            im.resize(_half(W, H)).save(half / "m" / sub / f"{i:05d}.png")
    return str(full), str(half)


@pytest.mark.parametrize("how", ["default", "device_png", "device_decode"])
def test_evaluate_dirs_with_resize_equals_scoring_files_pillow_resized(render_dirs, how):
    from gaussianprediction_amd import metrics
    full, half = render_dirs
    kw = {} if how == "default" else {how: True}
    with device_work():
        want = metrics.evaluate_dirs(half, device=DEV, write=False, **kw)
        got = metrics.evaluate_dirs(full, device=DEV, write=False, resize=True, resize_ratio=0.5, **kw)
        ignored = metrics.evaluate_dirs(half, device=DEV, write=False, resize=False, resize_ratio=0.25, **kw)
        full_size = metrics.evaluate_dirs(full, device=DEV, write=False, **kw)
    assert got == want and ignored == want                                               # number for number
    assert set(got["m"]["summary"]) == {"SSIM", "PSNR", "MS-SSIM", "D-SSIM"} and all(np.isfinite(v) for v in got["m"]["summary"].values())
    assert got != full_size                                                              # ... and not the full-size numbers
    with pytest.raises(ValueError, match=r"00000\.png: 341 x 333 -> 0 x 0: a target size of 0"):
        metrics.evaluate_dirs(full, device=DEV, write=False, resize=True, resize_ratio=0.001, **kw)
