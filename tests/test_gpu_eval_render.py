"""The render-to-disk loops (eval_render) on a synthetic model: render_set writes the reference's tree, every file decodes to the
quantisation of what render() gives in its exact mode, and evaluate_dirs on the tree equals evaluate_views on the same cameras;
render_video and render_trainSequence write their layouts; render_kpts with a PngWriter writes the pixels of its default path."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import png_cases as P

pytestmark = pytest.mark.gpu

H, W, IT = 163, 178, 50000


def _decode(path):
    from PIL import Image
    return np.array(Image.open(path))


def _q8(img):
    return P.quantise(img.detach().cpu().numpy()).transpose(1, 2, 0)


@pytest.fixture(scope="module")
def scene():
    from test_gpu_render import build
    from gaussianprediction_amd.cameras import orbit_cameras
    pc = build(N=3000, K=60, W=W, H=H)[0]
    cams = orbit_cameras(5, 4.0, 0.6911, W, H, device="cuda")
    for v, cam in enumerate(cams):
        cam.original_image = torch.from_numpy(P.disc(H, W, 40 + v)).cuda()
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    bg = torch.zeros(3, device="cuda")
    return SimpleNamespace(pc=pc, cams=cams, pipe=pipe, bg=bg)


def test_render_set_writes_the_tree_and_evaluate_dirs_scores_it(scene, tmp_path):
    import gaussianprediction_amd as gpa
    from gaussianprediction_amd import eval_render as ER, metrics as M
    root = str(tmp_path / "model")
    eval_path, stats = ER.render_set(root, "test", IT, scene.cams, scene.pc, scene.pipe, scene.bg)
    assert eval_path == os.path.join(root, "eval", "test")
    assert stats["frames"] == 5 and stats["seconds"] > 0 and stats["views_per_s"] == 5 / stats["seconds"] and stats["rerendered"] >= 0
    method = os.path.join(eval_path, f"ours_{IT}")
    names = [f"{i:05d}.png" for i in range(5)]
    assert sorted(os.listdir(os.path.join(method, "renders"))) == names == sorted(os.listdir(os.path.join(method, "gt")))
    kp = np.loadtxt(os.path.join(root, "kpts_fps.txt"))
    assert np.allclose(kp, scene.pc.get_superGaussians.detach().cpu().numpy()) and not os.path.exists(os.path.join(root, "kpts_incre.txt"))
    for i, cam in enumerate(scene.cams):
        with torch.no_grad():
            want = gpa.render(cam, scene.pc, scene.pipe, scene.bg, time=torch.from_numpy(cam.time).cuda(), it=IT)["render"]
        assert float(want.max()) > 0.05
        assert np.array_equal(_decode(os.path.join(method, "renders", names[i])), _q8(want)), i
        assert np.array_equal(_decode(os.path.join(method, "gt", names[i])), _q8(cam.original_image)), i
    # the directory form scores the same 8-bit renders against the 8-bit ground truth
    got = M.evaluate_dirs(eval_path, write=False)[f"ours_{IT}"]["summary"]
    gts = [torch.from_numpy(P.quantise(cam.original_image.cpu().numpy())).to(torch.float32).div(255.0).cuda() for cam in scene.cams]
    want = M.evaluate_views(scene.pc, scene.cams, gts, scene.pipe, scene.bg, IT, quantize8=True)["summary"]
    assert set(got) == {"SSIM", "PSNR", "MS-SSIM", "D-SSIM"}
    for k, v in got.items():
        print(k, v, want[k])
        assert abs(v - want[k]) <= 1e-9, (k, v, want[k])
    # args with adaptive keypoints: the rest of the keypoints go to kpts_incre.txt
    args = SimpleNamespace(max_points=40, adaptive_points_num=20)
    ER.render_set(root, "test", IT, scene.cams[:1], scene.pc, scene.pipe, scene.bg, args=args)
    assert np.loadtxt(os.path.join(root, "kpts_fps.txt")).shape == (40, 3) and np.loadtxt(os.path.join(root, "kpts_incre.txt")).shape == (20, 3)


def test_render_video_and_train_sequence_layouts(scene, tmp_path):
    import gaussianprediction_amd as gpa
    from gaussianprediction_amd import eval_render as ER
    from gaussianprediction_amd.cameras import Camera
    root = str(tmp_path / "model")
    eval_path, stats = ER.render_video(root, "video", IT, scene.cams[:3], scene.pc, scene.pipe, scene.bg, interpolation=2)
    vdir = os.path.join(eval_path, f"ours_{IT}", "renders_video")
    assert eval_path == os.path.join(root, "eval", "video") and stats["frames"] == 5
    assert sorted(os.listdir(vdir)) == [f"{i:05d}.png" for i in range(5)]
    # frame 2 is view 1 itself (ratio 1 from view 0), frame 1 lies half way: its pose and time are the interpolated ones
    for frame_id, (pi, vi, ratio) in {2: (0, 1, 1.0), 1: (0, 1, 0.5)}.items():
        prev, view = scene.cams[pi], scene.cams[vi]
        new_t, new_R = ER.interpolation_pose(view, prev, ratio)
        t = torch.from_numpy(prev.time) + round(ratio * 2) * ((torch.from_numpy(view.time) - torch.from_numpy(prev.time)) / 2)
        cam = Camera(R=new_R, T=new_t, FoVx=prev.FoVx, FoVy=prev.FoVy, width=W, height=H, time=float(t), device="cuda")
        with torch.no_grad():
            want = gpa.render(cam, scene.pc, scene.pipe, scene.bg, time=t.cuda(), it=IT)["render"]
        assert np.array_equal(_decode(os.path.join(vdir, f"{frame_id:05d}.png")), _q8(want)), frame_id
    eval_path, stats = ER.render_trainSequence(root, "train", IT, scene.cams[:4], scene.pc, scene.pipe, scene.bg, scene.cams, freeze_view_number=3)
    sdir = os.path.join(eval_path, f"ours_{IT}", "renders", "view_003")
    names = [f"{i:05d}.png" for i in range(4)]
    assert stats["frames"] == 4 and sorted(os.listdir(sdir)) == names == sorted(os.listdir(os.path.join(eval_path, f"ours_{IT}", "gt")))
    with torch.no_grad():
        want = gpa.render(scene.cams[3], scene.pc, scene.pipe, scene.bg, time=torch.from_numpy(scene.cams[1].time).cuda(), it=IT)["render"]
    assert np.array_equal(_decode(os.path.join(sdir, names[1])), _q8(want))                # the frozen view at view 1's time
    assert np.array_equal(_decode(os.path.join(eval_path, f"ours_{IT}", "gt", names[1])), _q8(scene.cams[1].original_image))


def test_a_callers_writer_and_a_missing_directory(scene, tmp_path):
    import threading
    from gaussianprediction_amd import eval_render as ER, png_ops
    w = png_ops.PngWriter()
    eval_path, stats = ER.render_set(str(tmp_path / "m"), "test", IT, scene.cams[:2], scene.pc, scene.pipe, scene.bg, writer=w)
    w.close()
    assert w.files == 4 and len(os.listdir(os.path.join(eval_path, f"ours_{IT}", "renders"))) == 2
    w = png_ops.PngWriter()
    w.submit(scene.cams[0].original_image, str(tmp_path / "no-such-directory" / "00000.png"))
    with pytest.raises(FileNotFoundError):
        w.close()
    assert not [t for t in threading.enumerate() if t.name.startswith("PngWriter")]


def test_render_kpts_through_a_writer_writes_the_default_paths_pixels(tmp_path):
    from test_gpu_gcn import IT as GCN_IT, _stage3_model
    from gaussianprediction_amd import motion, png_ops
    g, cams, pipe, bg = _stage3_model()
    for v, cam in enumerate(cams):
        cam.original_image = torch.from_numpy(P.disc(cam.image_height, cam.image_width, v)).cuda()
    steps = [g.keypoint_motion(torch.tensor([t], dtype=torch.float32, device="cuda"), GCN_IT) for t in (0.1, 0.4, 0.7)]
    kx, kr = torch.stack([s[0] for s in steps]), torch.stack([s[1] for s in steps])
    a = motion.render_kpts(cams, g, pipe, bg, kx, kr, GCN_IT, metrics=True, out_dir=str(tmp_path / "host"))
    with png_ops.PngWriter() as w:
        b = motion.render_kpts(cams, g, pipe, bg, kx, kr, GCN_IT, metrics=True, out_dir=str(tmp_path / "device"), writer=w)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and float(a[0].max()) > 0.05
    for sub in ("renders", "gt"):
        names = sorted(os.listdir(tmp_path / "host" / sub))
        assert names == sorted(os.listdir(tmp_path / "device" / sub)) == [f"{i:05d}.png" for i in range(3)]
        for n in names:
            assert np.array_equal(_decode(tmp_path / "host" / sub / n), _decode(tmp_path / "device" / sub / n)), (sub, n)
