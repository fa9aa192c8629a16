"""The self-synchronising JPEG entropy stage on the device (include/gp_jpeg_sync.h, jpeg_sync): every case of tests/jpeg_sync_cases.py --
the ones tests/test_jpeg_sync_host.py has put through the same workgroup programs on the CPU, the malformed ones under the sanitizers --
through the kernels, with guard bytes round every output slot and the scratch buffer.  Status OK on every well-formed file; the device's
bytes equal the one-lane path's, Pillow's and the emulator's; the info words equal the emulator's; float32 output is the bytes / 255; two
calls are bit-identical; an image of a batch equals its B = 1 call; every malformed stream is SERIAL between two good images and raises
the one-lane path's error through decode(sync=True); decode_files and decode_avi with sync=True equal sync=False."""
import os

import numpy as np
import pytest
import torch

import jpeg_cases as J
import jpeg_decode_cases as D
import jpeg_sync_cases as SC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 16


@pytest.fixture(scope="module")
def JD():
    from gaussianprediction_amd import jpeg_decode
    return jpeg_decode


@pytest.fixture(scope="module")
def JS():
    from gaussianprediction_amd import jpeg_sync
    return jpeg_sync


@pytest.fixture(scope="module")
def emulate(tmp_path_factory):
    """csrc/jpeg_sync_core.h on the CPU (tests/jpeg_sync_emulate.cpp, built plain): run(items) -> (images, status, info)."""
    return SC.build_emulator(tmp_path_factory.mktemp("jpeg_sync_emulate"), sanitize=False)


@pytest.fixture(scope="module")
def well(JS):
    return SC.wellformed(JS.S, JS.C)


def test_the_library_exports_the_stage_and_decode_takes_sync(JD, JS):
    """Fails without the feature."""
    from gaussianprediction_amd import _lib
    assert hasattr(_lib.lib(), "gp_jpeg_sync_decode") and int(JS.lib().gp_jpeg_sync_abi_version()) == 1
    f = D.pillow_file(D.noise(40, 88, 3), quality=90, subsampling=0)
    (fast,) = JD.decode([f], device=DEV, sync=True)
    (slow,) = JD.decode([f], device=DEV, sync=False)
    assert JS.eligible(JD.parse(f)) and torch.equal(fast, slow)
    with pytest.raises(RuntimeError, match="sync must be"):
        JD.decode([f], device=DEV, sync="yes")


KINDS = ["short-", "length", "rounds-", "chunks-", "periodic-white-512", "periodic-white-2048", "partial-", "narrow-", "tables-", "disc-", "natural-"]


@pytest.mark.parametrize("kind", KINDS)
def test_device_equals_the_one_lane_path_pillow_and_the_emulator(JD, JS, well, emulate, kind):
    cases = [c for c in well if c.name.startswith(kind)]
    assert cases
    items = [JD.parse(c.file, c.name) for c in cases]
    images, status, info = JS.decode_once(items, device=DEV, guard=GUARD)          # (the guards are checked inside)
    again, status2, info2 = JS.decode_once(items, device=DEV, guard=GUARD)
    floats, _, _ = JS.decode_once(items, device=DEV, dtype=torch.float32, guard=GUARD)
    serial = JD.decode([c.file for c in cases], device=DEV, sync=False)
    emulated, est, einfo = emulate(items)
    assert status == status2 == est == [SC.OK] * len(cases), status             # never SERIAL on a well-formed file
    assert info == info2 == einfo == [c.ref.info for c in cases]
    for k, c in enumerate(cases):
        got = images[k].cpu().numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, emulated[k]), c.name                  # the same program on the CPU
        assert torch.equal(images[k], serial[k]), c.name                                            # the one-lane path
        assert np.array_equal(got, D.pillow_pixels(c.file).transpose(2, 0, 1)), c.name              # Pillow's decoder
        assert torch.equal(images[k], again[k]), c.name                                             # two calls: the same bits
        assert floats[k].dtype == torch.float32 and torch.equal(floats[k].cpu(), images[k].cpu().to(torch.float32) / 255.0), c.name      # (the division as the host does it: correctly rounded)
    for k in range(0, len(cases), 3):                                                              # an image of the batch is its B = 1 call
        (alone,), (s,), (w,) = JS.decode_once([items[k]], device=DEV, guard=GUARD)
        assert s == SC.OK and w == info[k] and torch.equal(alone, images[k]), cases[k].name


def test_constructed_stream_equals_the_one_lane_path(JD, JS, emulate):
    c = SC.constructed(JS.S, JS.C)
    it = JD.parse(c.file, c.name)
    (img,), (s,), (w,) = JS.decode_once([it], device=DEV, guard=GUARD)
    (want,) = JD.decode([c.file], device=DEV)
    (em,), _, (ew,) = emulate([it])
    assert s == SC.OK and w == ew == c.ref.info and torch.equal(img, want) and np.array_equal(img.cpu().numpy(), em)


def test_batch_of_three_equals_three_single_calls(JD, JS):
    cases = SC.batch()
    items = [JD.parse(c.file, c.name) for c in cases]
    together, status, info = JS.decode_once(items, device=DEV, guard=GUARD)
    assert status == [SC.OK] * 3
    for it, c, im, w in zip(items, cases, together, info):
        (alone,), (s,), (w1,) = JS.decode_once([it], device=DEV, guard=GUARD)
        assert s == SC.OK and w1 == w and torch.equal(alone, im) and np.array_equal(im.cpu().numpy(), D.pillow_pixels(c.file).transpose(2, 0, 1))
    assert not torch.equal(together[0], together[1])


def test_malformed_streams_are_serial_and_raise_the_one_lane_error(JD, JS, emulate):
    from gaussianprediction_amd import _lib
    for c in SC.malformed():
        files = [c.goods[0], c.file, c.goods[1]]
        items = [JD.parse(f, n) for f, n in zip(files, ("a", c.name, "b"))]
        images, status, info = JS.decode_once(items, device=DEV, guard=GUARD)
        _, est, einfo = emulate(items)
        assert status == est == [SC.OK, SC.SERIAL, SC.OK] and info == einfo, (c.name, status)
        for k in (0, 2):
            assert np.array_equal(images[k].cpu().numpy(), D.pillow_pixels(files[k]).transpose(2, 0, 1)), c.name
        names, errors = ["a.jpg", f"bad-{c.name}.jpg", "b.jpg"], []
        for sync in (False, True, "auto"):
            with pytest.raises(_lib.GpHipError, match=rf"bad-{c.name}\.jpg: .*status {c.status} \(GP_JPEG_DECODE_{JD.STATUS[c.status]}\)") as e:
                JD.decode(files, device=DEV, names=names, sync=sync)
            errors.append(str(e.value))
        assert errors[0] == errors[1] == errors[2], c.name


def test_decode_files_and_decode_avi_with_sync_equal_the_one_lane_results(JD, tmp_path):
    from gaussianprediction_amd import jpeg_ops
    paths = []
    for i in range(6):
        img = J.textured(64, 96, 40 + i)
        p = tmp_path / (f"frame{i}.jpeg" if i % 3 == 2 else f"{i:05d}.jpg")       # (the names say nothing: the bytes do)
        if i % 2:
            p.write_bytes(jpeg_ops.encode_to_bytes(torch.from_numpy(img).to(DEV), subsampling="420")[0])      # a restart marker every 8 MCUs
        else:
            p.write_bytes(D.pillow_file(img, quality=92, subsampling=2 if i % 4 else 0))                      # none
        paths.append(p)
    (tmp_path / "small.jpg").write_bytes(D.pillow_file(J.textured(8, 8, 1), quality=90))                      # one segment, too short to be eligible
    paths.append(tmp_path / "small.jpg")
    slow = JD.decode_files(paths, device=DEV)
    for sync in (True, "auto"):
        fast = JD.decode_files(paths, device=DEV, sync=sync)
        assert len(fast) == len(slow) == 7 and all(torch.equal(a, b) for a, b in zip(fast, slow))
    unit = JD.decode_files(paths, device=DEV, dtype=torch.float32, sync=True)
    assert all(torch.equal(u.cpu(), a.cpu().to(torch.float32) / 255.0) for u, a in zip(unit, slow))
    frames = [D.pillow_file(J.blobs(80, 96, s), quality=85, subsampling=2) for s in range(5)]
    avi = jpeg_ops.AviFile(tmp_path / "v.avi", 96, 80, 24)
    for f in frames:
        avi.add(f)
    avi.close()
    want = np.stack([D.pillow_pixels(f).transpose(2, 0, 1) for f in frames])
    slow = JD.decode_avi(tmp_path / "v.avi", device=DEV)
    fast = JD.decode_avi(tmp_path / "v.avi", device=DEV, sync=True)
    assert torch.equal(fast, slow) and np.array_equal(fast.cpu().numpy(), want)
    assert torch.equal(JD.decode_avi(tmp_path / "v.avi", device=DEV, frames=[3, 0], sync=True), slow[[3, 0]])


def test_evaluate_dirs_with_decode_sync_gives_the_same_numbers(tmp_path):
    from gaussianprediction_amd import metrics as M
    root = tmp_path / "run"
    D.eval_directory(root, 163, 178, DEV)
    want = M.evaluate_dirs(str(root), device=DEV, device_decode=True, write=False)
    assert M.evaluate_dirs(str(root), device=DEV, device_decode=True, decode_sync=True, write=False) == want
