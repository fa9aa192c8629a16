"""Host side of the Scene layer (no GPU): gaussianprediction_amd.dataset_readers and gaussianprediction_amd.scene against the record
tests/golden/make_scene_vectors.py took of the reference's own readers on the datasets of tests/golden/scenes/.  Where a step needs
decoded images, load_cameras gets an injected decoder (`_decode=`)."""
import json
import os
import random
import shutil

import numpy as np
import pytest
import torch

from gaussianprediction_amd import dataset_readers as dr
from gaussianprediction_amd import scene as sc
from gaussianprediction_amd.io_formats import read_ply_vertices
from scene_cases import ATOL, SCENES, check_cameras_json, check_info, copy_scene, record, scene_args


def blank_decode(records, device):
    """load_cameras' decoder without a device: zeros of the shape the device decoders return."""
    return [torch.zeros(3 if r.background is not None else r.channels, r.height, r.width) for r in records]


class Recorder:
    """What Scene asks of the model."""

    def __init__(self):
        self.calls = []

    def create_from_pcd(self, pcd, extent):
        self.calls.append(("create_from_pcd", pcd, extent))

    def load_ply(self, path):
        self.calls.append(("load_ply", path))

    def save_ply(self, path):
        self.calls.append(("save_ply", path))


# ---- the readers against the record --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag, kw", [("dnerf_eval_black", dict(white_background=False, eval=True)),
                                     ("dnerf_eval_white", dict(white_background=True, eval=True)),
                                     ("dnerf_noeval", dict(white_background=False, eval=False)),
                                     ("dnerf_t06", dict(white_background=False, eval=True, max_time=0.6))])
def test_dnerf_reader(tmp_path, tag, kw):
    src = copy_scene("dnerf", tmp_path)
    info = dr.readNerfSyntheticInfo(src, **kw)
    check_info(info, tag)
    ground = [1, 1, 1] if kw["white_background"] else [0, 0, 0]
    for c in info.train_cameras + info.test_cameras + info.render_cameras:
        assert c.image == dr.ImageRecord(c.image_path, "png", 24, 16, 4, ground) and c.image.size == (24, 16) and os.path.isfile(c.image.path)
    assert info.ply_path == os.path.join(src, "points3d.ply") and info.point_cloud.points.shape == (50000, 3)


@pytest.mark.parametrize("val_ids", [False, True])
@pytest.mark.parametrize("max_time", [1.0, 0.75])
def test_hyper_reader(tmp_path, val_ids, max_time):
    src = copy_scene("hyper", tmp_path, val_ids=val_ids)
    info = dr.readHyperDataInfos(src, max_time, 0.5)
    check_info(info, f"hyper_{'val' if val_ids else 'noval'}_{'full' if max_time == 1.0 else 't075'}")
    for c in info.train_cameras + info.test_cameras:
        assert c.time.dtype == np.float32 and c.time.shape == (1,) and (c.width, c.height) == (24, 16)
        assert c.image == dr.ImageRecord(f"{src}/rgb/2x/{c.image_name}", "png", 24, 16, 3, None)
    assert info.render_cameras is info.test_cameras and info.point_cloud.points.shape == (50, 3)


def test_hyper_reader_asserts_that_both_sides_of_max_time_are_populated(tmp_path):
    with pytest.raises(AssertionError):
        dr.readHyperDataInfos(copy_scene("hyper", tmp_path), 0.0, 0.5)      # (no frame has time < 0)


@pytest.mark.parametrize("text", [False, True])
@pytest.mark.parametrize("eval_", [True, False])
def test_colmap_reader(tmp_path, text, eval_):
    """Binary, and the same model as text (which holds a SIMPLE_PINHOLE camera: the reference's text reader stops there)."""
    src = copy_scene("colmap", tmp_path, text=text)
    info = dr.readColmapSceneInfo(src, None, eval_)
    check_info(info, "colmap_eval" if eval_ else "colmap_noeval")
    names = [c.image_name for c in sorted(info.train_cameras + info.test_cameras, key=lambda c: c.image_name)]
    assert names == [f"v_{k:02d}" for k in range(9)]
    kinds = {c.image_name: (c.image.kind, c.image.channels) for c in info.train_cameras + info.test_cameras}
    assert kinds["v_00"] == ("jpeg", 3) and kinds["v_07"] == ("png", 3) and kinds["v_05"] == ("png", 4)
    assert all(c.image.background is None and c.image.size == (32, 24) for c in info.train_cameras)
    arrays = record()[0]
    assert np.array_equal(info.point_cloud.points, arrays["colmap_ply/points"]) and np.array_equal(info.point_cloud.colors, arrays["colmap_ply/colors"])
    assert np.array_equal(info.point_cloud.normals, arrays["colmap_ply/normals"])


# ---- the COLMAP parsers --------------------------------------------------------------------------------------------------------------
def test_colmap_binary_and_text_give_the_same_model():
    b, t = os.path.join(SCENES, "colmap/sparse/0"), os.path.join(SCENES, "colmap/sparse_txt/0")
    cb, ct = dr.read_cameras_bin(f"{b}/cameras.bin"), dr.read_cameras_txt(f"{t}/cameras.txt")
    assert list(cb) == list(ct) == [1, 2] and [c.model for c in cb.values()] == ["SIMPLE_PINHOLE", "PINHOLE"]
    for k in cb:
        assert cb[k][:4] == ct[k][:4] and np.array_equal(cb[k].params, ct[k].params)
    ib, it = dr.read_images_bin(f"{b}/images.bin"), dr.read_images_txt(f"{t}/images.txt")
    assert list(ib) == list(it) == list(range(1, 10))
    for k in ib:
        assert (ib[k].id, ib[k].camera_id, ib[k].name) == (it[k].id, it[k].camera_id, it[k].name)
        assert np.array_equal(ib[k].qvec, it[k].qvec) and np.array_equal(ib[k].tvec, it[k].tvec)
    assert [ib[k].name for k in (1, 5)] == ["v_06.jpg", "v_00.jpg"]                 # the name order is not the id order
    arrays = record()[0]
    for kind, got in (("bin", dr.read_points3D_bin(f"{b}/points3D.bin")), ("txt", dr.read_points3D_txt(f"{t}/points3D.txt"))):
        for name, a in zip(("xyz", "rgb", "error"), got):
            want = arrays[f"colmap_points_{kind}/{name}"]
            assert a.shape == want.shape == (40, {"xyz": 3, "rgb": 3, "error": 1}[name]) and a.dtype == want.dtype and np.array_equal(a, want), (kind, name)


@pytest.mark.parametrize("text", [False, True])
def test_colmap_points_are_converted_to_the_reference_ply_once(tmp_path, text):
    src = copy_scene("colmap", tmp_path, text=text)
    ply = os.path.join(src, "sparse/0/points3D.ply")
    assert not os.path.exists(ply)
    dr.readColmapSceneInfo(src, None, True)
    v = read_ply_vertices(ply)
    assert [(n, v.dtype[n].str) for n in v.dtype.names] == [(n, "<f4") for n in ("x", "y", "z", "nx", "ny", "nz")] + [(n, "|u1") for n in ("red", "green", "blue")]
    arrays = record()[0]
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], axis=1), arrays["colmap_points_bin/xyz"].astype(np.float32))
    assert np.array_equal(np.stack([v["red"], v["green"], v["blue"]], axis=1), arrays["colmap_points_bin/rgb"].astype(np.uint8))
    assert not np.stack([v["nx"], v["ny"], v["nz"]]).any()
    stamp = os.stat(ply).st_mtime_ns
    dr.readColmapSceneInfo(src, None, True)
    assert os.stat(ply).st_mtime_ns == stamp                                        # (not written again)


def test_colmap_other_camera_models_are_walked_and_refused_by_name(tmp_path):
    cams = dr.read_cameras_bin(os.path.join(SCENES, "colmap/cameras_bad.bin"))
    assert cams[1].model == "OPENCV" and cams[1].params.shape == (8,)
    src = copy_scene("colmap", tmp_path)
    shutil.copyfile(os.path.join(src, "cameras_bad.bin"), os.path.join(src, "sparse/0/cameras.bin"))
    with pytest.raises(ValueError, match="OPENCV"):
        dr.readColmapSceneInfo(src, None, True)


def test_truncated_images_bin_raises(tmp_path):
    data = open(os.path.join(SCENES, "colmap/sparse/0/images.bin"), "rb").read()
    for cut in (len(data) - 5, len(data) // 2, 70, 4):
        path = os.path.join(tmp_path, f"images_{cut}.bin")
        with open(path, "wb") as fp:
            fp.write(data[:cut])
        with pytest.raises(ValueError, match="truncated"):
            dr.read_images_bin(path)
    pts = open(os.path.join(SCENES, "colmap/sparse/0/points3D.bin"), "rb").read()
    path = os.path.join(tmp_path, "points3D.bin")
    with open(path, "wb") as fp:
        fp.write(pts[:-3])
    with pytest.raises(ValueError, match="truncated"):
        dr.read_points3D_bin(path)


def test_qvec2rotmat():
    q = np.array([0.5, -0.5, 0.5, 0.5])
    R = dr.qvec2rotmat(q)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and np.isclose(np.linalg.det(R), 1.0)
    assert np.array_equal(dr.qvec2rotmat([1, 0, 0, 0]), np.eye(3))
    assert np.allclose(dr.qvec2rotmat([np.cos(0.3), 0, 0, np.sin(0.3)]), [[np.cos(0.6), -np.sin(0.6), 0], [np.sin(0.6), np.cos(0.6), 0], [0, 0, 1]], atol=1e-15)


# ---- point cloud files ---------------------------------------------------------------------------------------------------------------
def test_store_ply_truncates_colours_and_fetch_ply_reads_it_back(tmp_path):
    path = os.path.join(tmp_path, "p.ply")
    xyz = np.array([[0.1, -2.5, 3.0], [1e-3, 7.0, -0.25]])
    dr.store_ply(path, xyz, np.array([[0.0, 0.999, 1.0], [127.5, 254.99, 255.0]]))
    head = open(path, "rb").read().split(b"end_header\n")[0].decode()
    assert head == "ply\nformat binary_little_endian 1.0\nelement vertex 2\n" + "".join(f"property float {n}\n" for n in ("x", "y", "z", "nx", "ny", "nz")) + \
        "".join(f"property uchar {n}\n" for n in ("red", "green", "blue"))
    assert os.path.getsize(path) == len(head) + len("end_header\n") + 2 * 27
    pcd = dr.fetch_ply(path)
    assert np.array_equal(pcd.points, xyz.astype(np.float32)) and pcd.points.dtype == np.float32
    assert np.array_equal(pcd.colors, np.array([[0, 0, 1], [127, 254, 255]]) / 255.0) and not pcd.normals.any()


@pytest.mark.parametrize("seed", [0, 11])
def test_dnerf_random_cloud_is_the_formulas_draw(tmp_path, seed):
    src = copy_scene("dnerf", tmp_path)
    np.random.seed(seed)
    info = dr.readNerfSyntheticInfo(src, False, True)
    np.random.seed(seed)
    xyz = np.random.random((50000, 3)) * 2.6 - 1.3
    rgb = (np.random.random((50000, 3)) / 255.0 * 0.28209479177387814 + 0.5) * 255
    assert np.array_equal(info.point_cloud.points, xyz.astype(np.float32))
    assert np.array_equal(info.point_cloud.colors, rgb.astype(np.uint8) / 255.0) and set(np.unique(rgb.astype(np.uint8))) == {127}
    size = os.path.getsize(info.ply_path)
    np.random.seed(seed + 1)
    again = dr.readNerfSyntheticInfo(src, False, True)                              # the file is there now: nothing is drawn
    assert os.path.getsize(info.ply_path) == size and np.array_equal(again.point_cloud.points, info.point_cloud.points)


def test_nerfpp_norm():
    cams = [dr.CameraInfo(0, np.eye(3), -np.array(c, dtype=np.float64), 1.0, 1.0, None, "", "", 1, 1) for c in ([1, 0, 0], [-1, 0, 0], [0, 4, 0], [0, 0, 0])]
    norm = dr.getNerfppNorm(cams)       # centres (R = I: -T) are the four points, their mean (0, 1, 0), the farthest (0, 4, 0)
    assert np.allclose(norm["translate"], [0, -1, 0], atol=1e-15) and np.isclose(norm["radius"], 3.3, atol=1e-15)


# ---- image records -------------------------------------------------------------------------------------------------------------------
def test_image_record_reads_headers_only(tmp_path):
    assert dr.image_record(os.path.join(SCENES, "colmap/images/v_00.jpg"))[1:] == ("jpeg", 32, 24, 3, None)
    assert dr.image_record(os.path.join(SCENES, "colmap/images/v_05.png"), [1, 1, 1])[1:] == ("png", 32, 24, 4, [1, 1, 1])
    data = open(os.path.join(SCENES, "dnerf/train/r_000.png"), "rb").read()
    path = os.path.join(tmp_path, "cut.png")
    with open(path, "wb") as fp:
        fp.write(data[:40])                                                         # the IHDR chunk alone is enough for a record
    assert dr.image_record(path)[1:5] == ("png", 24, 16, 4)
    with open(path, "wb") as fp:
        fp.write(b"GIF89a" + bytes(40))
    with pytest.raises(ValueError, match="neither a PNG nor a JPEG"):
        dr.image_record(path)


# ---- Scene ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, tag, kw", [("dnerf", "dnerf_eval_black", {}), ("hyper", "hyper_noval_full", {}), ("colmap", "colmap_eval", {}),
                                           ("dnerf", "dnerf_noeval", dict(eval=False))])
def test_scene_writes_input_ply_and_cameras_json(tmp_path, name, tag, kw):
    src = copy_scene(name, tmp_path)
    np.random.seed(7)
    model = Recorder()
    args = scene_args(src, tmp_path / "out", data_device="cpu", **kw)
    s = sc.Scene(args, model, shuffle=False, device="cpu", _decode=blank_decode)
    source = {"dnerf": "points3d.ply", "hyper": "points3D_downsample.ply", "colmap": "sparse/0/points3D.ply"}[name]
    assert open(os.path.join(args.model_path, "input.ply"), "rb").read() == open(os.path.join(src, source), "rb").read()
    table = record()[1][tag]
    check_cameras_json(json.load(open(os.path.join(args.model_path, "cameras.json"))), tag)
    assert s.total_frame == table["total_frame"] and abs(s.cameras_extent - record()[0][f"{tag}/radius"]) <= ATOL
    for split, cams in (("train", s.getTrainCameras()), ("test", s.getTestCameras()), ("render", s.getRenderCameras() if table["splits"]["render"]["uid"] else [])):
        rec = table["splits"][split]
        assert [c.image_name for c in cams] == rec["image_name"] and [c.colmap_id for c in cams] == rec["uid"] and [c.uid for c in cams] == list(range(len(cams)))
        assert all(c.original_image.shape == (3, h, w) and (c.image_width, c.image_height) == (w, h) for c, w, h in zip(cams, rec["width"], rec["height"]))
    (call,) = model.calls
    assert call[0] == "create_from_pcd" and call[2] == s.cameras_extent and call[1].points.shape[1] == 3
    s.save(30)
    assert model.calls[-1] == ("save_ply", os.path.join(args.model_path, "point_cloud/iteration_30", "point_cloud.ply"))


def test_scene_shuffles_as_the_reference_does(tmp_path):
    src = copy_scene("dnerf", tmp_path)
    np.random.seed(7)
    splits = record()[1]["dnerf_eval_black"]["splits"]
    for seed in (0, 5):
        random.seed(seed)
        s = sc.Scene(scene_args(src, tmp_path / f"out{seed}", data_device="cpu"), Recorder(), shuffle=True, device="cpu", _decode=blank_decode)
        random.seed(seed)
        train, test = list(splits["train"]["image_name"]), list(splits["test"]["image_name"])
        random.shuffle(train)
        random.shuffle(test)
        assert [c.image_name for c in s.getTrainCameras()] == train and [c.image_name for c in s.getTestCameras()] == test
        assert [c.image_name for c in s.getRenderCameras()] == splits["render"]["image_name"]
        assert [c.uid for c in s.getTrainCameras()] == list(range(len(train)))      # uid: the place after the shuffle
    assert train != splits["train"]["image_name"]


def test_scene_type_detection_follows_the_reference_precedence(tmp_path, monkeypatch):
    class Reached(Exception):
        pass

    def stop(kind):
        def reader(*a, **kw):
            raise Reached(kind, a, kw)
        return reader

    for kind in ("Colmap", "Blender", "Hyper"):
        monkeypatch.setitem(sc.sceneLoadTypeCallbacks, kind, stop(kind))
    src = tmp_path / "src"
    os.makedirs(src / "sparse")
    open(src / "transforms_train.json", "w").close()
    open(src / "points.npy", "w").close()
    args = scene_args(str(src), tmp_path / "out", images="images_2", max_time=0.7)
    for kind, want_a, want_kw, gone in (("Colmap", (str(src), "images_2", True), {}, "sparse"),
                                        ("Blender", (str(src), False, True), {"max_time": 0.7}, "transforms_train.json"),
                                        ("Hyper", (str(src), 0.7, 0.25), {}, "points.npy")):
        with pytest.raises(Reached) as e:
            sc.Scene(args, Recorder(), ratio=0.25, device="cpu", _decode=blank_decode)
        assert e.value.args == (kind, want_a, want_kw)
        (shutil.rmtree if gone == "sparse" else os.remove)(src / gone)
    with pytest.raises(ValueError, match="could not recognize the scene type"):
        sc.Scene(args, Recorder(), device="cpu", _decode=blank_decode)


def test_search_for_max_iteration_and_load_iteration(tmp_path):
    src = copy_scene("hyper", tmp_path)
    args = scene_args(src, tmp_path / "out", data_device="cpu")
    for it in (7, 3000, 200):
        os.makedirs(os.path.join(args.model_path, "point_cloud", f"iteration_{it}"))
    assert sc.searchForMaxIteration(os.path.join(args.model_path, "point_cloud")) == 3000
    for ask, want in ((-1, 3000), (200, 200)):
        model = Recorder()
        s = sc.Scene(args, model, load_iteration=ask, shuffle=False, device="cpu", _decode=blank_decode)
        assert s.loaded_iter == want
        assert model.calls == [("load_ply", os.path.join(args.model_path, "point_cloud", f"iteration_{want}", "point_cloud.ply"))]
        assert not os.path.exists(os.path.join(args.model_path, "input.ply")) and not os.path.exists(os.path.join(args.model_path, "cameras.json"))
        assert len(s.getTrainCameras()) == 3


# ---- load_cameras with an injected decoder -------------------------------------------------------------------------------------------
def test_load_cameras_builds_reference_cameras(tmp_path):
    info = dr.readColmapSceneInfo(copy_scene("colmap", tmp_path), None, False)
    infos = info.train_cameras
    g = torch.Generator().manual_seed(1)
    seen = []

    def decode(records, device):
        seen.append((list(records), device))
        return [torch.rand(r.channels, r.height, r.width, generator=g) * 1.5 - 0.2 for r in records]       # (values outside 0..1: the clamp)

    args = scene_args("", tmp_path / "m", data_device="cpu")
    cams = sc.load_cameras(infos, 1.0, args, device="cpu", _decode=decode)
    assert len(seen) == 1 and seen[0][0] == [c.image for c in infos] and seen[0][1] == "cpu"               # one call for the whole list
    g = torch.Generator().manual_seed(1)
    for k, (cam, ci) in enumerate(zip(cams, infos)):
        raw = torch.rand(ci.image.channels, 24, 32, generator=g) * 1.5 - 0.2
        want = raw[:3].clamp(0.0, 1.0) * (raw[3:4] if ci.image.channels == 4 else 1.0)
        assert torch.equal(cam.original_image, want) and cam.original_image.device.type == "cpu" and cam.data_device == torch.device("cpu")
        assert isinstance(cam, sc.SceneCamera) and (cam.uid, cam.colmap_id, cam.image_name) == (k, ci.uid, ci.image_name)
        assert cam.R is ci.R and cam.T is ci.T and cam.FoVx == ci.FovX and cam.FoVy == ci.FovY and cam.time == 0.0
        assert (cam.image_width, cam.image_height, cam.znear, cam.zfar, cam.scale) == (32, 24, 0.01, 100.0, 1.0) and not cam.trans.any()
        assert cam.fwd_flow is None and cam.bwd_flow_mask is None
        w2c = np.eye(4)
        w2c[:3, :3], w2c[:3, 3] = ci.R.T, ci.T
        assert np.abs(cam.world_view_transform.numpy().T - w2c).max() < 1e-6
        assert torch.allclose(cam.full_proj_transform, cam.world_view_transform @ cam.projection_matrix)
        assert np.abs(cam.camera_center.numpy() - np.linalg.inv(w2c)[:3, 3]).max() < 1e-5
    assert sum(ci.image.channels == 4 for ci in infos) == 1
    # dict entries, as the reference's flow datasets hand them over: cameras under the same keys, None stays None, one decoder call
    seen.clear()
    pairs = [{"cam": infos[0], "fwd_cam": infos[1], "bwd_cam": None}, infos[2], {"cam": infos[3], "fwd_cam": None, "bwd_cam": infos[4]}]
    out = sc.load_cameras(pairs, 1.0, args, device="cpu", _decode=decode)
    assert len(seen) == 1 and [r.path for r in seen[0][0]] == [infos[k].image.path for k in range(5)]
    assert out[0]["bwd_cam"] is None and out[2]["fwd_cam"] is None and isinstance(out[1], sc.SceneCamera)
    assert [out[0]["cam"].image_name, out[0]["fwd_cam"].image_name, out[1].image_name, out[2]["cam"].image_name, out[2]["bwd_cam"].image_name] == \
        [c.image_name for c in infos[:5]]
    assert (out[0]["cam"].uid, out[0]["fwd_cam"].uid, out[1].uid, out[2]["bwd_cam"].uid) == (0, 0, 1, 2)
    again = sc.SceneCamera.from_Camera(out[1])
    assert torch.equal(again.original_image, out[1].original_image) and again.image_name == out[1].image_name and again.uid == 1
    assert torch.equal(again.full_proj_transform, out[1].full_proj_transform)
    assert sc.load_cameras([], 1.0, args, device="cpu", _decode=decode) == []


def test_decode_records_refuses_mixed_backgrounds_and_unknown_kinds():
    a, b = dr.ImageRecord("a.png", "png", 2, 2, 4, [0, 0, 0]), dr.ImageRecord("b.png", "png", 2, 2, 4, [1, 1, 1])
    with pytest.raises(ValueError, match="different backgrounds"):
        sc.decode_records([a, b], "cuda")
    with pytest.raises(ValueError, match="neither"):
        sc.decode_records([dr.ImageRecord("a.gif", "gif", 2, 2, 3)], "cuda")


def test_camera_to_json_equals_the_record(tmp_path):
    for name, tag, read in (("dnerf", "dnerf_eval_white", lambda p: dr.readNerfSyntheticInfo(p, True, True)),
                            ("hyper", "hyper_val_t075", lambda p: dr.readHyperDataInfos(p, 0.75, 0.5)),
                            ("colmap", "colmap_noeval", lambda p: dr.readColmapSceneInfo(p, None, False))):
        np.random.seed(7)
        info = read(copy_scene(name, tmp_path, val_ids=True) if name == "hyper" else copy_scene(name, tmp_path))
        entries = [sc.camera_to_JSON(k, c) for k, c in enumerate(list(info.test_cameras) + list(info.train_cameras))]
        check_cameras_json(json.loads(json.dumps(entries)), tag)


# ---- the import shim -----------------------------------------------------------------------------------------------------------------
def test_scene_shim_names_are_the_packages_objects():
    import scene
    import scene.cameras
    import scene.dataset_readers
    import scene.deformable_field
    import scene.gaussian_model
    import gaussianprediction_amd as gpa
    assert scene.Scene is sc.Scene and scene.GaussianModel is gpa.GaussianModel
    assert scene.cameras.Camera is sc.SceneCamera and scene.cameras.MiniCam is sc.MiniCam
    assert scene.gaussian_model.GaussianModel is gpa.GaussianModel and scene.gaussian_model.BasicPointCloud is dr.BasicPointCloud
    assert scene.deformable_field.Deformable_Field is gpa.Deformable_Field
    m = scene.dataset_readers
    assert m.sceneLoadTypeCallbacks is dr.sceneLoadTypeCallbacks and set(dr.sceneLoadTypeCallbacks) == {"Colmap", "Blender", "Hyper"}
    assert (m.CameraInfo, m.SceneInfo, m.fetchPly, m.storePly, m.getNerfppNorm) == (dr.CameraInfo, dr.SceneInfo, dr.fetch_ply, dr.store_ply, dr.getNerfppNorm)
    assert dr.CameraInfo._fields == ("uid", "R", "T", "FovY", "FovX", "image", "image_path", "image_name", "width", "height", "time")
    assert dr.SceneInfo._fields == ("point_cloud", "train_cameras", "test_cameras", "render_cameras", "nerf_normalization", "ply_path", "total_frame")
    assert hasattr(gpa.GaussianModel, "save_ply") and hasattr(gpa.GaussianModel, "create_from_pcd")
    cam = scene.cameras.MiniCam(4, 3, 0.5, 0.6, 0.01, 100.0, torch.eye(4), torch.eye(4))
    assert torch.equal(cam.camera_center, torch.zeros(3)) and (cam.image_width, cam.image_height) == (4, 3)


def test_dnerf_rgb_files_carry_no_background_because_the_composite_is_the_identity(tmp_path):
    """The reference composites every D-NeRF file after convert("RGBA"); with alpha 255 its formula gives back the byte it was given,
    for each of the 256 and both backgrounds -- so the record of a three-channel file asks for no composite."""
    v = np.arange(256, dtype=np.uint8).reshape(1, 256, 1)
    norm = np.concatenate([v, v, v, np.full_like(v, 255)], axis=2) / 255.0
    for ground in ([0, 0, 0], [1, 1, 1]):
        arr = norm[:, :, :3] * norm[:, :, 3:4] + np.array(ground) * (1 - norm[:, :, 3:4])
        assert np.array_equal((arr * 255.0).astype(np.int64) & 255, np.broadcast_to(v, (1, 256, 3)))
    from PIL import Image
    src = copy_scene("dnerf", tmp_path)
    Image.open(os.path.join(src, "train/r_001.png")).convert("RGB").save(os.path.join(src, "train/r_001.png"))
    Image.open(os.path.join(src, "train/r_002.png")).convert("L").save(os.path.join(src, "test/r_000.png"))
    train, _ = dr._transforms_cameras(src, "transforms_train.json", True, ".png")
    assert [c.image.background for c in train[:3]] == [[1, 1, 1], None, [1, 1, 1]] and [c.image.channels for c in train[:3]] == [4, 3, 4]
    with pytest.raises(ValueError, match="r_000.png.*1 channel"):
        dr._transforms_cameras(src, "transforms_test.json", True, ".png")
