"""JPEG encoding on the device (include/gp_jpeg.h, jpeg_ops): for every case of tests/jpeg_cases.py at both subsamplings the device's
file is byte for byte the file of the same workgroup programs run on the CPU (tests/jpeg_emulate.cpp), which tests/test_jpeg_host.py
holds against Pillow, its own entropy decoder and the exact transform; batches, repeated calls and the two input kinds agree; the
writers write behind the stream; render_video, render_kpts and evaluate_dirs produce their videos and JPEG files only when asked."""
import io
import json
import os
import threading

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_cases as J
import png_cases as P

pytestmark = pytest.mark.gpu

CANARY = 0xA5
CASES = {name: (img, qt) for name, img, qt in J.cases()}
SUBS = ("420", "444")


@pytest.fixture(scope="module")
def JPG():
    from gaussianprediction_amd import jpeg_ops
    return jpeg_ops


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return J.build_emulator(tmp_path_factory.mktemp("jpeg_emulate"))


def _encode(JPG, imgs, sub, qt):
    """(files as bytes, the whole slots as numpy, sizes) of one call into canary-filled slots."""
    x = torch.from_numpy(imgs).cuda()
    B, _, H, W = x.shape
    out = torch.full((B, JPG.bound(H, W, sub) + 64), CANARY, dtype=torch.uint8, device="cuda")
    buf, sizes = JPG.encode(x, subsampling=sub, qtables=qt, out=out)
    assert buf.data_ptr() == out.data_ptr() and sizes.dtype == torch.int32 and sizes.shape == (B,)
    slots, n = out.cpu().numpy(), sizes.cpu().tolist()
    return [slots[b, :n[b]].tobytes() for b in range(B)], slots, n


def _psnr(a, b):
    mse = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("name", list(CASES))
def test_device_file_is_the_emulators_file(JPG, emulator, name, sub):
    img, qt = CASES[name]
    qt = qt if qt is not None else JPG.quant_tables(90)
    _, H, W = img.shape
    files, slots, sizes = _encode(JPG, img[None], sub, qt)
    assert 0 < sizes[0] <= JPG.bound(H, W, sub)
    assert (slots[0, sizes[0]:] == CANARY).all()                                 # nothing at or beyond the file's length
    want = emulator(img, sub, qt)
    assert len(files[0]) == len(want) and files[0] == want


def test_batches_calls_and_input_kinds_agree(JPG):
    rng = np.random.default_rng(3)
    imgs = np.stack([J.textured(45, 67, 1), rng.integers(0, 256, (3, 45, 67), dtype=np.uint8), P.ramp(45, 67)])
    for sub in SUBS:
        files, slots, sizes = _encode(JPG, imgs, sub, None)
        again, slots2, sizes2 = _encode(JPG, imgs, sub, None)
        assert sizes == sizes2 and np.array_equal(slots, slots2)                 # two calls: the same bits
        assert len(set(files)) == 3
        for b in range(3):
            assert (slots[b, sizes[b]:] == CANARY).all()
            alone, _, _ = _encode(JPG, imgs[b:b + 1], sub, None)
            assert alone[0] == files[b]                                          # row b of the batch is the B = 1 call on image b
    # uint8 input and the float input it is the quantisation of; the list form; quality and tables
    x = torch.from_numpy(np.stack([P.disc(37, 53, 7), P.edge_floats((3, 37, 53), 8)])).cuda()
    q = torch.from_numpy(P.quantise(x.cpu().numpy())).cuda()
    from_float = JPG.encode_to_bytes(x)
    assert JPG.encode_to_bytes(q) == from_float == JPG.encode_to_bytes([x[0], x[1]])
    assert JPG.encode_to_bytes(x[1]) == from_float[1:] and JPG.encode_to_bytes(x.double()) == from_float
    assert JPG.encode_to_bytes(x, qtables=JPG.quant_tables(90)) == from_float != JPG.encode_to_bytes(x, quality=75)
    assert JPG.encode_to_bytes(x, subsampling="444") != from_float
    with pytest.raises(RuntimeError, match="out must be"):
        JPG.encode(x, out=torch.empty(2, JPG.bound(37, 53) - 8, dtype=torch.uint8, device="cuda"))


def test_writer_writes_behind_the_stream_and_reports_a_worker_error(JPG, tmp_path):
    x = torch.from_numpy(np.stack([P.disc(37, 45, s) for s in range(5)])).cuda()
    want = JPG.encode_to_bytes(x, quality=75)
    with JPG.JpegWriter(slots=2, threads=2, quality=75) as w:                    # more images than buffers: the submit waits for free ones
        w.submit(x, [tmp_path / f"{i:05d}.jpg" for i in range(5)])
        w.submit(x[0], tmp_path / "single.jpg")
        big = torch.from_numpy(P.disc(90, 120, 1)).cuda()                        # a larger image: the pinned buffers are replaced
        w.submit([big], [str(tmp_path / "big.jpg")])
    assert w.files == 7
    for i in range(5):
        assert open(tmp_path / f"{i:05d}.jpg", "rb").read() == want[i]
    assert open(tmp_path / "single.jpg", "rb").read() == want[0]
    assert open(tmp_path / "big.jpg", "rb").read() == JPG.encode_to_bytes(big, quality=75)[0]
    bad = JPG.JpegWriter()
    bad.submit(x[:2], [tmp_path / "missing" / "a.jpg", tmp_path / "missing" / "b.jpg"])
    with pytest.raises(FileNotFoundError):
        bad.close()
    assert not [t for t in threading.enumerate() if t.name.startswith("JpegWriter")]
    bad.close()                                                                  # (a second close is quiet)


def _check_video(path, frames8, fps_rate, fps_scale):
    """The RIFF walk of the host test over a finished video; every chunk decodes to within the host test's PSNR bar of what Pillow's
    own encoder gives for the frame at the same tables."""
    from test_jpeg_host import PSNR_MARGIN_DB, _pillow_encode, check_avi
    from gaussianprediction_amd import jpeg_ops
    n, _, H, W = frames8.shape
    r = check_avi(open(path, "rb").read(), n, W, H, fps_rate, fps_scale)
    qt = jpeg_ops.quant_tables(jpeg_ops.VIDEO_QUALITY)
    deficits = []
    for (_, payload), src in zip(r["frames"], frames8):
        got = np.array(Image.open(io.BytesIO(payload))).transpose(2, 0, 1)
        ref = np.array(Image.open(io.BytesIO(_pillow_encode(src, qt, "420")))).transpose(2, 0, 1)
        print(f"{os.path.basename(str(path))}: PSNR {_psnr(got, src):.3f} dB (Pillow {_psnr(ref, src):.3f}, {_psnr(got, src) - _psnr(ref, src):+.3f})")
        deficits.append(_psnr(ref, src) - _psnr(got, src))
    assert max(deficits) <= PSNR_MARGIN_DB, deficits
    return r


def test_video_writer_over_five_frames(JPG, tmp_path):
    x = torch.from_numpy(np.stack([P.disc(37, 53, s) for s in range(5)])).cuda()
    path = tmp_path / "v.avi"
    with JPG.VideoWriter(path, 10, slots=2) as v:
        v.submit(x[:3])
        v.submit(x[3])
        v.submit([x[4]])
        with pytest.raises(RuntimeError, match="a frame of 38 x 53"):
            v.submit(torch.zeros(3, 38, 53, device="cuda"))
    assert v.frames == 5 and not [t for t in threading.enumerate() if t.name.startswith("VideoWriter")]
    r = _check_video(path, P.quantise(x.cpu().numpy()), 10, 1)
    assert [f for _, f in r["frames"]] == JPG.encode_to_bytes(x, quality=90)     # in submission order, the encoder's own files


# ---- the callers: only when asked ----
H, W, IT = 163, 178, 50000


@pytest.fixture(scope="module")
def scene():
    from types import SimpleNamespace
    from test_gpu_render import build
    from gaussianprediction_amd.cameras import orbit_cameras
    pc = build(N=3000, K=60, W=W, H=H)[0]
    cams = orbit_cameras(5, 4.0, 0.6911, W, H, device="cuda")
    for v, cam in enumerate(cams):
        cam.original_image = torch.from_numpy(P.disc(H, W, 40 + v)).cuda()
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    return SimpleNamespace(pc=pc, cams=cams, pipe=pipe, bg=torch.zeros(3, device="cuda"))


def _png(path):
    return np.array(Image.open(path)).transpose(2, 0, 1)


def test_render_video_writes_the_avi_beside_the_frames(scene, tmp_path):
    from gaussianprediction_amd import eval_render as ER
    root = str(tmp_path / "scene_name" / "model")
    eval_path, stats = ER.render_video(root, "video", IT, scene.cams[:3], scene.pc, scene.pipe, scene.bg, interpolation=2, video=True)
    method = os.path.join(eval_path, f"ours_{IT}")
    names = [f"{i:05d}.png" for i in range(5)]
    assert stats["frames"] == 5 == 2 * ((3 - 1) // 1) + 1 and stats["video"] == os.path.join(method, "scene_name.avi")
    assert sorted(os.listdir(method)) == ["renders_video", "scene_name.avi"]
    assert sorted(os.listdir(os.path.join(method, "renders_video"))) == names    # exactly the PNG names it listed before
    frames8 = np.stack([_png(os.path.join(method, "renders_video", n)) for n in names])
    assert frames8.shape == (5, 3, H, W) and frames8.max() > 12
    _check_video(stats["video"], frames8, 120, 1)
    # a path of the caller's; and the default writes no video and reports none
    other = str(tmp_path / "other.avi")
    _, stats = ER.render_video(root, "video2", IT, scene.cams[:2], scene.pc, scene.pipe, scene.bg, interpolation=2, video=other, fps=24)
    assert stats["video"] == other and stats["frames"] == 3
    _check_video(other, np.stack([_png(os.path.join(root, "eval", "video2", f"ours_{IT}", "renders_video", n)) for n in names[:3]]), 24, 1)
    eval_path, stats = ER.render_video(root, "video3", IT, scene.cams[:2], scene.pc, scene.pipe, scene.bg, interpolation=2)
    assert "video" not in stats and os.listdir(os.path.join(eval_path, f"ours_{IT}")) == ["renders_video"]


def test_render_kpts_writes_its_video_when_asked(tmp_path):
    from test_gpu_gcn import IT as GCN_IT, _stage3_model
    from gaussianprediction_amd import motion
    g, cams, pipe, bg = _stage3_model()
    for v, cam in enumerate(cams):
        cam.original_image = torch.from_numpy(P.disc(cam.image_height, cam.image_width, v)).cuda()
    steps = [g.keypoint_motion(torch.tensor([t], dtype=torch.float32, device="cuda"), GCN_IT) for t in (0.1, 0.4, 0.7)]
    kx, kr = torch.stack([s[0] for s in steps]), torch.stack([s[1] for s in steps])
    a = motion.render_kpts(cams, g, pipe, bg, kx, kr, GCN_IT, metrics=True, out_dir=str(tmp_path / "plain"))
    b = motion.render_kpts(cams, g, pipe, bg, kx, kr, GCN_IT, metrics=True, out_dir=str(tmp_path / "video"), video=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and float(a[0].max()) > 0.05
    names = [f"{i:05d}.png" for i in range(3)]
    assert sorted(os.listdir(tmp_path / "plain" / "renders")) == names
    assert sorted(os.listdir(tmp_path / "video" / "renders")) == names + ["video.avi"]
    frames8 = P.quantise(torch.stack(b).cpu().numpy())
    _check_video(tmp_path / "video" / "renders" / "video.avi", frames8, 10, 1)
    with pytest.raises(ValueError, match="out_dir"):
        motion.render_kpts(cams, g, pipe, bg, kx, kr, GCN_IT, video=True)


def test_evaluate_dirs_writes_its_deltas_on_the_device_when_asked(scene, tmp_path):
    from test_jpeg_host import PSNR_MARGIN_DB
    from gaussianprediction_amd import eval_render as ER, metrics as M
    trees = {}
    for kind in ("host", "device"):
        eval_path, _ = ER.render_set(str(tmp_path / kind), "test", IT, scene.cams[:3], scene.pc, scene.pipe, scene.bg)
        got = M.evaluate_dirs(eval_path, device_jpeg=(kind == "device"))
        trees[kind] = (eval_path, got)
    (hp, hgot), (dp, dgot) = trees["host"], trees["device"]
    assert hgot == dgot
    for name in ("results.json", "per_view.json"):
        assert open(os.path.join(hp, name), "rb").read() == open(os.path.join(dp, name), "rb").read()
    names = [f"{i:05d}.jpg" for i in range(3)]
    assert sorted(os.listdir(os.path.join(dp, f"ours_{IT}", "deltas"))) == names == sorted(os.listdir(os.path.join(hp, f"ours_{IT}", "deltas")))
    for i, n in enumerate(names):
        render = _png(os.path.join(dp, f"ours_{IT}", "renders", f"{i:05d}.png")).astype(np.float32) / np.float32(255)
        gt = _png(os.path.join(dp, f"ours_{IT}", "gt", f"{i:05d}.png")).astype(np.float32) / np.float32(255)
        err = (np.abs(render - gt) * np.float32(255)).astype(np.uint8)           # the error image itself: trunc(|render - gt| * 255)
        im = Image.open(os.path.join(dp, f"ours_{IT}", "deltas", n))
        im.load()
        assert im.size == (W, H) and im.mode == "RGB"
        ours, host = np.array(im).transpose(2, 0, 1), _png(os.path.join(hp, f"ours_{IT}", "deltas", n))
        print(f"deltas/{n}: PSNR {_psnr(ours, err):.3f} dB (the host path's file {_psnr(host, err):.3f}, {_psnr(ours, err) - _psnr(host, err):+.3f})")
        assert err.max() > 12 and _psnr(ours, err) >= _psnr(host, err) - PSNR_MARGIN_DB
