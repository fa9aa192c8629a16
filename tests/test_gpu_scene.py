"""-m gpu: the Scene layer on the device -- the datasets of tests/golden/scenes/ loaded through dataset_readers + scene.load_cameras,
whose images come from the device decoders (png_decode, jpeg_decode) and are held bit for bit to what the reference's readers
produced (the record of tests/golden/make_scene_vectors.py) or to the files' own bytes, and a round trip: rendered views written as a
D-NeRF folder, loaded back with Scene, trained on for three steps."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from gaussianprediction_amd import dataset_readers as dr  # noqa: E402
from gaussianprediction_amd import jpeg_decode, png_decode, png_ops  # noqa: E402
from gaussianprediction_amd import scene as sc  # noqa: E402
from scene_cases import SCENES, copy_scene, record, scene_args  # noqa: E402


def as_float(pixels):
    """uint8 [H, W, C] -> float32 [C, H, W] = byte / 255, on the CPU: what the reference's PILtoTorch makes of an image."""
    return torch.from_numpy(np.ascontiguousarray(pixels)).permute(2, 0, 1).to(torch.float32) / 255.0


def file_pixels(path):
    return np.array(Image.open(path))


@pytest.mark.parametrize("white, data_device", [(False, "cuda"), (True, "cuda"), (True, "cpu")])
def test_dnerf_images_equal_the_reference_composite(tmp_path, white, data_device):
    np.random.seed(7)
    info = dr.readNerfSyntheticInfo(copy_scene("dnerf", tmp_path), white, True)
    arrays = record()[0]
    args = scene_args("", tmp_path / "m", data_device=data_device)
    for split in ("train", "test", "render"):
        cams = sc.load_cameras(getattr(info, f"{split}_cameras"), 1.0, args)
        want = arrays[f"dnerf_eval_{'white' if white else 'black'}/{split}/image"]
        assert len(cams) == len(want) == {"train": 5, "test": 3, "render": 1}[split]
        for cam, px in zip(cams, want):
            assert cam.original_image.shape == (3, 16, 24) and cam.original_image.dtype == torch.float32
            assert cam.original_image.device.type == data_device and cam.world_view_transform.device.type == "cuda"
            assert torch.equal(cam.original_image.cpu(), as_float(px)), (split, cam.image_name)


def test_hyper_images_equal_the_files_bytes(tmp_path):
    info = dr.readHyperDataInfos(copy_scene("hyper", tmp_path), 1.0, 0.5)
    args = scene_args("", tmp_path / "m")
    for infos in (info.train_cameras, info.test_cameras):
        for cam, ci in zip(sc.load_cameras(infos, 1.0, args), infos):
            assert cam.original_image.is_cuda and cam.image_name == ci.image_name and cam.time is ci.time
            assert torch.equal(cam.original_image.cpu(), as_float(file_pixels(ci.image.path))), ci.image_name


def test_colmap_images_and_one_decoder_call_per_kind(tmp_path, monkeypatch):
    calls = {"png": [], "jpeg": []}
    png_files, jpeg_files = png_decode.decode_files, jpeg_decode.decode_files
    monkeypatch.setattr(png_decode, "decode_files", lambda paths, **kw: calls["png"].append((list(paths), kw)) or png_files(paths, **kw))
    monkeypatch.setattr(jpeg_decode, "decode_files", lambda paths, **kw: calls["jpeg"].append((list(paths), kw)) or jpeg_files(paths, **kw))
    info = dr.readColmapSceneInfo(copy_scene("colmap", tmp_path), None, False)
    infos = info.train_cameras
    cams = sc.load_cameras(infos, 1.0, scene_args("", tmp_path / "m"))
    assert len(calls["png"]) == 1 and len(calls["jpeg"]) == 1                       # nine files, two calls
    assert len(calls["png"][0][0]) == 3 and len(calls["jpeg"][0][0]) == 6
    assert calls["png"][0][1]["dtype"] == torch.float32 and calls["png"][0][1]["background"] is None
    assert calls["jpeg"][0][1]["dtype"] == torch.float32 and calls["jpeg"][0][1]["sync"] is True
    direct = dict(zip(calls["jpeg"][0][0], jpeg_files(calls["jpeg"][0][0], device="cuda", dtype=torch.float32)))
    for cam, ci in zip(cams, infos):
        assert cam.original_image.shape == (3, 24, 32) and cam.original_image.is_cuda
        if ci.image.kind == "jpeg":
            assert torch.equal(cam.original_image, direct[ci.image.path]), ci.image_name    # the loader adds nothing to the decoder
        elif ci.image.channels == 4:
            px = as_float(file_pixels(ci.image.path))
            assert torch.equal(cam.original_image.cpu(), px[:3] * px[3:4]) and ci.image_name == "v_05"
        else:
            assert torch.equal(cam.original_image.cpu(), as_float(file_pixels(ci.image.path))), ci.image_name
    # a D-NeRF list: one PNG call with the background, no JPEG call
    calls["png"].clear(), calls["jpeg"].clear()
    np.random.seed(7)
    dn = dr.readNerfSyntheticInfo(copy_scene("dnerf", tmp_path), True, False)
    assert len(sc.load_cameras(dn.train_cameras, 1.0, scene_args("", tmp_path / "m"))) == 8
    assert len(calls["png"]) == 1 and not calls["jpeg"] and len(calls["png"][0][0]) == 8
    assert calls["png"][0][1]["background"].tolist() == [1.0, 1.0, 1.0] and calls["png"][0][1]["background"].is_cuda
    assert sc.load_cameras([], 1.0, scene_args("", tmp_path / "m")) == [] and len(calls["png"]) == 1


def test_a_file_the_decoders_refuse_raises_naming_it(tmp_path):
    src = copy_scene("colmap", tmp_path)
    bad = os.path.join(src, "images", "v_03.jpg")
    Image.open(os.path.join(SCENES, "colmap/images/v_03.jpg")).save(bad, quality=90, subsampling=1)          # 4:2:2
    info = dr.readColmapSceneInfo(src, None, False)                                 # the header walk takes it: it is a JPEG of 32 x 24
    with pytest.raises(ValueError, match="v_03.jpg.*2x1"):
        sc.load_cameras(info.train_cameras, 1.0, scene_args("", tmp_path / "m"))


# ---- round trip ------------------------------------------------------------------------------------------------------------------------
def _model_args():
    return SimpleNamespace(beta=0.1, d=4, w=256, feature_dim=32, jointly_iteration=10, second_stage_iteration=40, third_stage_iteration=60,
                           nearest_num=6, norm_rotation=True, step_opacity=False, step_opacity_iteration=5000, opacity_type="implicit",
                           xyz_noise_iteration=0, max_points=24, adaptive_points_num=8, adaptive_from_iter=5, adaptive_end_iter=18,
                           adaptive_interval=5, densify_from_grad="True", densify_from_teaching=False, teaching_threshold=0.2,
                           knn_type="hybird", feature_amplify=5.0, max_gaussian_size=3000, time_noise_ratio=0.5, time_noise_iteration=30,
                           use_time_decay=True)


def test_round_trip_through_a_dnerf_folder_and_three_train_steps(tmp_path, monkeypatch):
    from gaussian_renderer import render
    from scene import GaussianModel, Scene
    from gaussianprediction_amd.cameras import orbit_cameras
    from gaussianprediction_amd.scene_synth import SceneSpec, make_gaussians
    from gaussianprediction_amd.train_step import TrainStep
    from gaussianprediction_amd.training import default_training_args
    W, H, n = 64, 48, 1500
    torch.manual_seed(0)
    raw = make_gaussians(SceneSpec(n_gaussians=n, scale_lo=0.03, scale_hi=0.12, seed=4), device="cuda")
    source = GaussianModel(3, _model_args())
    source.set_inputDim(12, 60)
    source.create_from_tensors(raw["xyz"], raw["features_dc"], raw["features_rest"], raw["scaling"], raw["rotation"], raw["opacity"], raw["motion_feature"])
    views = orbit_cameras(6, 4.0, 0.69, W, H, device="cuda")
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    with torch.no_grad():
        renders = torch.stack([render(c, source, pipe, torch.zeros(3, device="cuda"), time=torch.from_numpy(c.time).cuda(), it=1)["render"] for c in views])
    src = tmp_path / "folder"
    os.makedirs(src / "train")
    for k, data in enumerate(png_ops.encode_to_bytes(renders)):
        with open(src / "train" / f"r_{k:03d}.png", "wb") as fp:
            fp.write(data)

    def frame(k):
        w2c = np.eye(4)
        w2c[:3, :3], w2c[:3, 3] = views[k].R.T, views[k].T
        c2w = np.linalg.inv(w2c)
        c2w[:3, 1:3] *= -1                                                         # COLMAP axes -> the OpenGL axes the file holds
        return {"file_path": f"./train/r_{k:03d}", "time": 0.9 * float(views[k].time[0]), "transform_matrix": c2w.tolist()}     # (every time < 1)

    for name, picks in (("train", range(6)), ("test", (1, 4))):
        with open(src / f"transforms_{name}.json", "w") as fp:
            json.dump({"camera_angle_x": views[0].FoVx, "frames": [frame(k) for k in picks]}, fp)
    rng = np.random.default_rng(0)
    dr.store_ply(str(src / "points3d.ply"), raw["xyz"].cpu().numpy(), rng.uniform(0, 255, size=(n, 3)))

    gaussians = GaussianModel(3, _model_args())
    gaussians.set_inputDim(12, 60)
    calls = []
    png_files = png_decode.decode_files
    monkeypatch.setattr(png_decode, "decode_files", lambda paths, **kw: calls.append(list(paths)) or png_files(paths, **kw))
    scene = Scene(scene_args(str(src), tmp_path / "out"), gaussians, shuffle=False)
    assert len(calls) == 1 and len(calls[0]) == 6       # Scene decodes its three lists in one pass, a file that stands in two of them once
    cams = scene.getTrainCameras()
    assert len(cams) == 6 and [c.image_name for c in scene.getTestCameras()] == ["r_001", "r_004"] and scene.getRenderCameras()[0].image_name == "r_001"
    for k, (cam, view) in enumerate(zip(cams, views)):
        px = file_pixels(src / "train" / f"r_{k:03d}.png")
        assert px.shape == (H, W, 3) and px.max() > 40                              # (something was rendered)
        assert cam.original_image.is_cuda and torch.equal(cam.original_image.cpu(), as_float(px))
        for name in ("world_view_transform", "full_proj_transform"):
            assert (getattr(cam, name) - getattr(view, name)).abs().max().item() <= 1e-5, (k, name)
        assert (cam.image_width, cam.image_height) == (W, H) and abs(cam.FoVy - view.FoVy) < 1e-12
    assert gaussians.get_xyz.shape[0] == n and os.path.getsize(tmp_path / "out" / "input.ply") == os.path.getsize(src / "points3d.ply")
    opt = default_training_args(iterations=90, position_lr_max_steps=90)
    gaussians.training_setup(opt)
    ts = TrainStep(gaussians, cams, [c.original_image for c in cams], 1, lambda_dssim=opt.lambda_dssim, schedule=True, training_args=opt)
    losses = []
    for it in range(1, 4):
        ts.iteration = it
        loss, _ = ts.step(it % len(cams))
        losses.append(float(loss))
    ts.sync_params()
    assert np.isfinite(losses).all() and losses[0] > 0
    scene.save(3)
    assert os.path.isfile(tmp_path / "out" / "point_cloud" / "iteration_3" / "point_cloud.ply")
