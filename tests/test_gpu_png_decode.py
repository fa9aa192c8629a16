"""PNG decoding on the device (include/gp_png_decode.h, png_decode): every case of tests/png_decode_cases.py -- the ones
tests/test_png_decode_host.py has put through the same workgroup programs on the CPU, the malformed ones under the sanitizers -- through
the kernels.  uint8 output equal to Pillow's array, float32 output bit-equal to metrics._load_rgb's tensor, two calls bit-identical,
an image of a mixed batch equal to its B = 1 call, the guard behind every output slot untouched, this project's own files decoded
BANDED in one pass, every malformed file refused with its status between two good images, the composite against the reader's
float64 formula, and evaluate_dirs(device_png=True) equal to the default path key for key and float for float."""
import io
import json

import numpy as np
import pytest
import torch

import png_decode_cases as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 16


@pytest.fixture(scope="module")
def PD():
    from gaussianprediction_amd import png_decode
    return png_decode


def _pillow(data):
    from PIL import Image
    arr = np.array(Image.open(io.BytesIO(data)))
    return arr[:, :, None] if arr.ndim == 2 else arr


def _once(PD, files, banded=None, **kw):
    """One pass with guards: (images as numpy or None, status, modes); the guard elements behind every slot are checked here."""
    items = [PD.parse(f, f"<{k}>") for k, f in enumerate(files)]
    banded = [it.banded for it in items] if banded is None else banded
    images, status, modes, slots = PD.decode_once(items, banded, device=DEV, guard=GUARD, **kw)
    for dst in slots:
        raw = dst.cpu().numpy()
        assert (raw[:, -GUARD:].view(np.uint8) == 0xA5).all()
    return [im.cpu().numpy() if s == 0 else None for im, s in zip(images, status)], status, modes


def _check(PD, cases, tmp_path):
    from gaussianprediction_amd import metrics as M
    files = [c.file for c in cases]
    images, modes = PD.decode(files, device=DEV, return_modes=True)
    again = PD.decode(files, device=DEV)
    floats = PD.decode(files, device=DEV, dtype=torch.float32, channels=3)
    for k, c in enumerate(cases):
        want = _pillow(c.file)
        assert np.array_equal(want, c.want), c.name
        got = images[k].cpu().numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, want.transpose(2, 0, 1)), c.name
        assert modes[k] == c.mode, (c.name, modes[k])
        assert torch.equal(images[k], again[k]), c.name                                     # two calls: the same bits
        path = tmp_path / "f.png"
        path.write_bytes(c.file)
        ref = M._load_rgb(str(path), DEV)[0]
        assert floats[k].dtype == torch.float32 and torch.equal(floats[k].view(torch.int32), ref.view(torch.int32)), c.name
    return images


WELL = D.wellformed()
KINDS = {"filters": "filters-", "rows-and-widths": ("rows-", "width-"), "zlib": ("zlib-", "window-"), "by-hand": ("fixed-", "dynamic-"),
         "foreign": "foreign-"}


@pytest.mark.parametrize("kind", list(KINDS))
def test_files_decode_to_pillows_pixels(PD, kind, tmp_path):
    cases = [c for c in WELL if c.name.startswith(KINDS[kind])]
    images = _check(PD, cases, tmp_path)
    guarded, status, _ = _once(PD, [c.file for c in cases])                                # the first pass, with guards
    for c, im, g, s in zip(cases, images, guarded, status):
        assert s in (0, D.NOT_BANDED) and (s == 0 or c.mode == D.SERIAL), (c.name, s)
        assert g is None or np.array_equal(g, im.cpu().numpy()), c.name
    for c, im in list(zip(cases, images))[::5]:                                            # an image of the mixed batch is its B = 1 call
        (alone,) = PD.decode([c.file], device=DEV)
        assert torch.equal(alone, im), c.name


def test_pillows_own_files(PD, tmp_path):
    cases = D.pillow_cases()
    images = _check(PD, cases, tmp_path)
    for c, im in zip(cases, images):
        (alone,), status, modes = _once(PD, [c.file])
        assert status == [0] and modes == [D.SERIAL] and np.array_equal(alone, im.cpu().numpy()), c.name


def test_this_projects_files_decode_banded_in_one_pass(PD, tmp_path):
    """Written by png_ops on the device.  ONE pass: the serial pass behind decode() would hide a broken fast path."""
    from gaussianprediction_amd import png_ops
    cases = []
    for name, img, fnone in D.own_inputs():
        (data,) = png_ops.encode_to_bytes(torch.from_numpy(img).to(DEV), filter_none=fnone)
        cases.append(D.own_case(name, data, img))
    assert sum(c.mode == D.BANDED for c in cases) == 6
    images, status, modes = _once(PD, [c.file for c in cases])
    again, _, _ = _once(PD, [c.file for c in cases])
    for c, im, im2, s, m in zip(cases, images, again, status, modes):
        assert s == 0 and m == c.mode == D.BANDED, (c.name, s, m)
        assert np.array_equal(im, _pillow(c.file).transpose(2, 0, 1)) and np.array_equal(im, c.want.transpose(2, 0, 1)) and np.array_equal(im, im2), c.name
        (alone,), _, _ = _once(PD, [c.file])
        assert np.array_equal(alone, im), c.name
    _check(PD, cases, tmp_path)
    serial, status, modes = _once(PD, [c.file for c in cases], banded=[False] * 6)         # the same files as one stream each
    assert status == [0] * 6 and modes == [D.SERIAL] * 6 and all(np.array_equal(a, b) for a, b in zip(serial, images))


@pytest.mark.parametrize("bg", [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0)])
def test_composite_against_the_readers_formula(PD, bg):
    c = D.composite_case()
    want = torch.from_numpy(D.composite_reference(c.want, bg).transpose(2, 0, 1).copy())   # [REF scene/dataset_readers.py:214-218]
    back = torch.tensor(bg, device=DEV)
    (u8,) = PD.decode([c.file], device=DEV, background=back)
    (f32,) = PD.decode([c.file], device=DEV, background=back, dtype=torch.float32)
    assert u8.dtype == torch.uint8 and torch.equal(u8.cpu(), want)
    assert torch.equal(f32.cpu().view(torch.int32), (want.to(torch.float32) / 255.0).view(torch.int32))
    (plain,) = PD.decode([c.file], device=DEV)
    assert np.array_equal(plain.cpu().numpy(), c.want.transpose(2, 0, 1))
    (guarded,), status, _ = _once(PD, [c.file], background=back)
    assert status == [0] and np.array_equal(guarded, want.numpy())


def test_malformed_files_end_in_their_status_between_two_good_images(PD):
    from gaussianprediction_amd import _lib
    a, b = D.good_small(1), D.good_small(2)
    for c in D.malformed():
        images, status, modes = _once(PD, [a.file, c.file, b.file])
        assert status == [0, c.status, 0], (c.name, status)
        assert modes == [D.SERIAL] * 3
        assert np.array_equal(images[0], a.want.transpose(2, 0, 1)) and np.array_equal(images[2], b.want.transpose(2, 0, 1)), c.name
        with pytest.raises(_lib.GpHipError, match=rf"bad-{c.name}\.png: .*status {c.status} \(GP_PNG_DECODE_{PD.STATUS[c.status]}\)"):
            PD.decode([a.file, c.file, b.file], device=DEV, names=["a.png", f"bad-{c.name}.png", "b.png"])


def test_a_damaged_band_comes_back_not_banded_and_then_names_its_fault(PD):
    from gaussianprediction_amd import _lib
    c = next(c for c in WELL if c.name == "foreign-full-flush")
    it = PD.parse(c.file)
    bad = D.png_file(60, 120, 3, [bytes(it.pieces[0]), bytes(it.pieces[1])[:-3]])
    images, status, modes = _once(PD, [c.file, bad])
    assert status == [0, D.NOT_BANDED] and modes == [D.BANDED, D.BANDED] and np.array_equal(images[0], c.want.transpose(2, 0, 1))
    with pytest.raises(_lib.GpHipError, match="GP_PNG_DECODE_TRUNCATED"):
        PD.decode([c.file, bad], device=DEV)


def _directory(root, H, W):
    from PIL import Image
    from gaussianprediction_amd import png_ops
    for method, own in (("ours", True), ("theirs", False)):
        for sub in ("renders", "gt"):
            (root / method / sub).mkdir(parents=True)
        for i in range(4):
            for sub, seed in (("renders", 10 * i + own), ("gt", 10 * i + 5)):
                img = D.noise(H, W, 3, seed)
                path = root / method / sub / f"{i:05d}.png"
                if own:
                    path.write_bytes(png_ops.encode_to_bytes(torch.from_numpy(img.transpose(2, 0, 1).copy()).to(DEV))[0])
                else:
                    Image.fromarray(img).save(path)


def test_evaluate_dirs_with_device_png_gives_the_default_paths_numbers(PD, tmp_path):
    """Four pairs, two methods, one with Pillow-written files and one with this project's.  At 37 x 45 both paths refuse alike
    (MS-SSIM needs min(H, W) > 160, as on the parent commit), so the dictionaries are compared at 163 x 178."""
    from gaussianprediction_amd import _lib, metrics as M
    small = tmp_path / "small"
    _directory(small, 37, 45)
    for kw in (dict(), dict(device_png=True)):
        with pytest.raises(_lib.GpHipError, match="MS-SSIM needs"):
            M.evaluate_dirs(str(small), device=DEV, **kw)
    root = tmp_path / "run"
    _directory(root, 163, 178)
    want = M.evaluate_dirs(str(root), device=DEV)
    files = [json.load(open(root / n)) for n in ("results.json", "per_view.json")]
    deltas = [(root / "theirs" / "deltas" / f"{i:05d}.jpg").read_bytes() for i in range(4)]
    for kw in (dict(), dict(png_group=3), dict(png_group=1)):
        got = M.evaluate_dirs(str(root), device=DEV, device_png=True, **kw)
        assert got == want and list(got) == ["ours", "theirs"] and len(got["ours"]["per_view"]["PSNR"]) == 4
        assert [json.load(open(root / n)) for n in ("results.json", "per_view.json")] == files
        assert [(root / "theirs" / "deltas" / f"{i:05d}.jpg").read_bytes() for i in range(4)] == deltas
    assert want["ours"]["summary"] != want["theirs"]["summary"]
