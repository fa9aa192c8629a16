"""JPEG decoding on the device (include/gp_jpeg_decode.h, jpeg_decode): every case of tests/jpeg_decode_cases.py -- the ones
tests/test_jpeg_decode_host.py has put through the same workgroup programs on the CPU, the malformed ones under the sanitizers --
through the kernels.  The device's bytes equal the emulator's and Pillow's, float32 output is bit-equal to metrics._load_rgb's tensor,
two calls are bit-identical, an image of a batch equals its B = 1 call, the guard behind every output slot is untouched, every
malformed file is refused with its status between two good images, jpeg_ops.encode -> jpeg_decode.decode equals Pillow's decoding of
the same bytes, decode_avi equals Pillow frame by frame, and evaluate_dirs(device_decode=True) equals the default path key for key
and float for float."""
import json

import numpy as np
import pytest
import torch

import jpeg_cases as J
import jpeg_decode_cases as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 16


@pytest.fixture(scope="module")
def JD():
    from gaussianprediction_amd import jpeg_decode
    return jpeg_decode


@pytest.fixture(scope="module")
def own():
    """own(img, "420" / "444", quality or (luminance, chrominance), key) -> the file jpeg_ops writes on the device."""
    from gaussianprediction_amd import jpeg_ops
    done = {}

    def write(img, sub, q, key):
        if key not in done:
            kw = dict(quality=q) if isinstance(q, int) else dict(qtables=q)
            (done[key],) = jpeg_ops.encode_to_bytes(torch.from_numpy(np.ascontiguousarray(img)).to(DEV), subsampling=sub, **kw)
        return done[key]

    return write


@pytest.fixture(scope="module")
def well(own):
    return D.wellformed(own)


@pytest.fixture(scope="module")
def emulate(tmp_path_factory):
    """emulate(items) -> (images [3, H, W] numpy, status): csrc/jpeg_decode_core.h on the CPU (tests/jpeg_decode_emulate.cpp, built plain)."""
    run = D.build_emulator(tmp_path_factory.mktemp("jpeg_decode_emulate"), sanitize=False)
    return lambda items: run(items, guard=0)


def _once(JD, files, **kw):
    """One pass with guards: (images as numpy, status); the guard elements behind every slot are checked here."""
    items = [JD.parse(f, f"<{k}>") for k, f in enumerate(files)]
    images, status, slots = JD.decode_once(items, device=DEV, guard=GUARD, **kw)
    for dst in slots:
        raw = dst.cpu().numpy()
        assert (raw[:, -GUARD:].view(np.uint8) == 0xA5).all()
    return [im.cpu().numpy() for im in images], status


KINDS = {"textured": "-textured-", "rows-and-wrap": ("-rows-", "-wrap-"), "narrow": "-narrow-", "noise-and-saturated": ("-noise-", "-saturated-"),
         "constant": "-constant-", "lanes": "-lanes-", "zrl": "-zrl-", "optimize-and-appn": ("-optimize-", "-com-appn-")}


@pytest.mark.parametrize("kind", list(KINDS))
def test_device_equals_the_emulator_and_pillow(JD, well, emulate, kind, tmp_path):
    from gaussianprediction_amd import metrics as M
    keys = KINDS[kind] if isinstance(KINDS[kind], tuple) else (KINDS[kind],)
    cases = [c for c in well if any(k in c.name for k in keys)]
    assert cases
    files = [c.file for c in cases]
    images = JD.decode(files, device=DEV)
    again = JD.decode(files, device=DEV)
    floats = JD.decode(files, device=DEV, dtype=torch.float32)
    guarded, status = _once(JD, files)
    emulated, est = emulate([JD.parse(f) for f in files])
    assert status == est == [0] * len(files)
    for k, c in enumerate(cases):
        got = images[k].cpu().numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, emulated[k]), c.name                  # the same program on the CPU
        assert np.array_equal(got, D.pillow_pixels(c.file).transpose(2, 0, 1)), c.name              # Pillow's decoder
        assert torch.equal(images[k], again[k]) and np.array_equal(guarded[k], got), c.name         # two calls: the same bits
    for k in range(0, len(cases), 5):                                                              # float32; an image of the batch is its B = 1 call
        path = tmp_path / "f.jpg"
        path.write_bytes(files[k])
        ref = M._load_rgb(str(path), DEV)[0]
        assert floats[k].dtype == torch.float32 and torch.equal(floats[k].view(torch.int32), ref.view(torch.int32)), cases[k].name
        (alone,) = JD.decode([files[k]], device=DEV)
        assert torch.equal(alone, images[k]), cases[k].name


def test_batch_of_three_equals_three_single_calls(JD, own):
    files = [own(D.noise(45, 67, s), "420", 90, f"three-{s}") for s in (31, 32, 33)]
    together = JD.decode(files, device=DEV)
    for f, im in zip(files, together):
        (alone,) = JD.decode([f], device=DEV)
        assert torch.equal(alone, im) and np.array_equal(im.cpu().numpy(), D.pillow_pixels(f).transpose(2, 0, 1))
    assert not torch.equal(together[0], together[1])


def test_malformed_files_end_in_their_status_between_two_good_images(JD, own, emulate):
    from gaussianprediction_amd import _lib
    for c in D.malformed(own):
        files = [c.goods[0], c.file, c.goods[1]]
        images, status = _once(JD, files)
        assert status == [0, c.status, 0], (c.name, status)
        _, est = emulate([JD.parse(f) for f in files])
        assert est == status, c.name
        for k in (0, 2):
            assert np.array_equal(images[k], D.pillow_pixels(files[k]).transpose(2, 0, 1)), c.name
        with pytest.raises(_lib.GpHipError, match=rf"bad-{c.name}\.jpg: .*status {c.status} \(GP_JPEG_DECODE_{JD.STATUS[c.status]}\)"):
            JD.decode(files, device=DEV, names=["a.jpg", f"bad-{c.name}.jpg", "b.jpg"])
    with pytest.raises(ValueError, match="RST markers do not count"):
        JD.decode([D.rst_out_of_order(own)], device=DEV)


def test_round_trip_through_the_encoder(JD):
    from gaussianprediction_amd import jpeg_ops
    imgs = torch.from_numpy(np.stack([J.blobs(100, 90, s) for s in range(3)])).to(DEV)
    for sub in ("420", "444"):
        files = jpeg_ops.encode_to_bytes(imgs, quality=85, subsampling=sub)
        back = JD.decode(files, device=DEV)
        for f, im, src in zip(files, back, imgs):
            assert np.array_equal(im.cpu().numpy(), D.pillow_pixels(f).transpose(2, 0, 1))
            assert (im.to(torch.float32) - src.to(torch.float32)).abs().mean() < 3        # (it is the picture, not only Pillow's bytes)


def test_decode_avi_equals_pillow_frame_by_frame(JD, tmp_path):
    from gaussianprediction_amd import jpeg_ops
    from jpeg_ref import riff_walk
    frames = torch.from_numpy(np.stack([J.blobs(80, 96, s) for s in range(5)])).to(DEV)
    path = tmp_path / "v.avi"
    vw = jpeg_ops.VideoWriter(path, 24)
    vw.submit(frames[:2])
    vw.submit(frames[2:])
    vw.close()
    files = [f for _, f in riff_walk(path.read_bytes())["frames"]]
    want = np.stack([D.pillow_pixels(f).transpose(2, 0, 1) for f in files])
    got = JD.decode_avi(path, device=DEV)
    assert got.shape == (5, 3, 80, 96) and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    picked = JD.decode_avi(path, device=DEV, dtype=torch.float32, frames=[4, 0])
    assert torch.equal(picked.cpu(), got[[4, 0]].cpu().to(torch.float32) / 255.0)             # (the division as the host does it: correctly rounded)
    with pytest.raises(ValueError, match="frame 5 of 5"):
        JD.decode_avi(path, device=DEV, frames=[5])


def test_evaluate_dirs_with_device_decode_gives_the_default_paths_numbers(JD, tmp_path):
    """Four pairs of .png renders and .jpg ground truth, two methods: one with this project's JPEG files, one with Pillow's (no
    restart markers: the serial path).  At 48 x 64 both paths refuse alike (MS-SSIM needs min(H, W) > 160, as on the parent commit),
    so the dictionaries are compared at the smallest size the default path scores, 163 x 178."""
    from gaussianprediction_amd import _lib, metrics as M
    small = tmp_path / "small"
    D.eval_directory(small, 48, 64, DEV)
    for kw in (dict(), dict(device_decode=True)):
        with pytest.raises(_lib.GpHipError, match="MS-SSIM needs"):
            M.evaluate_dirs(str(small), device=DEV, **kw)
    root = tmp_path / "run"
    D.eval_directory(root, 163, 178, DEV)
    want = M.evaluate_dirs(str(root), device=DEV)
    files = [json.load(open(root / n)) for n in ("results.json", "per_view.json")]
    for kw in (dict(), dict(png_group=3), dict(png_group=1)):
        got = M.evaluate_dirs(str(root), device=DEV, device_decode=True, **kw)
        assert got == want and list(got) == ["ours", "theirs"] and len(got["ours"]["per_view"]["PSNR"]) == 4
        assert [json.load(open(root / n)) for n in ("results.json", "per_view.json")] == files
    assert want["ours"]["summary"] != want["theirs"]["summary"]
    with pytest.raises(ValueError, match=r"00000\.jpg"):                                        # device_png alone keeps refusing a .jpg
        M.evaluate_dirs(str(root), device=DEV, device_png=True, write=False)
