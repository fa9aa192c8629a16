"""`Scene`: what the reference runs between its command line and the first iteration [REF scene/__init__.py, utils/camera_utils.py,
scene/cameras.py, utils/system_utils.py] -- the dataset reader for the folder's kind, `input.ply` and `cameras.json`, the seeded
shuffle, the cameras with their ground truth, and the model's first Gaussians.

The readers (dataset_readers.py) decode nothing: every camera carries an ImageRecord.  `load_cameras` turns a whole camera list into
images with ONE png_decode.decode_files call and ONE jpeg_decode.decode_files call (float32 = byte / 255, the D-NeRF composite
inside the PNG kernel), so the pixels never pass through the host and the device is read only for the decoders' status words.
`Scene` puts its three lists through one such pass together (DESIGN.md section 20 has the measurement behind that).  There
is no host decoder behind this: a file the device decoders refuse raises their ValueError, which names the file."""
from __future__ import annotations

import json
import os
import random

import numpy as np
import torch

from .cameras import Camera, fov2focal
from .dataset_readers import sceneLoadTypeCallbacks


class SceneCamera(Camera):
    """cameras.Camera under the constructor and attribute names of the reference's Camera [REF scene/cameras.py:17-72].  `device`
    (not in the reference, which says .cuda()) is where the matrices live."""

    def __init__(self, colmap_id, R, T, FoVx, FoVy, image, gt_alpha_mask, image_name, uid, trans=np.array([0.0, 0.0, 0.0]), scale=1.0,
                 data_device="cuda", time=0., fwd_flow=None, bwd_flow=None, fwd_flow_mask=None, bwd_flow_mask=None, *, device="cuda"):
        super().__init__(R, T, FoVx, FoVy, image.shape[2], image.shape[1], device=device, uid=uid, trans=trans, scale=scale)
        self.R, self.T, self.FoVx, self.FoVy = R, T, FoVx, FoVy        # as given, not converted
        self.colmap_id, self.image_name, self.time, self.trans, self.scale = colmap_id, image_name, time, trans, scale
        self.fwd_flow, self.fwd_flow_mask, self.bwd_flow, self.bwd_flow_mask = fwd_flow, fwd_flow_mask, bwd_flow, bwd_flow_mask
        self.data_device = where = torch.device(data_device)
        shown = image.clamp(0.0, 1.0).to(where)                         # (a tensor of this camera's own)
        self.original_image = shown if gt_alpha_mask is None else shown.mul_(gt_alpha_mask.to(where))

    @classmethod
    def from_Camera(cls, Camera):
        c = Camera
        return cls(c.colmap_id, c.R, c.T, c.FoVx, c.FoVy, c.original_image, None, c.image_name, c.uid, c.trans, c.scale, c.data_device, c.time,
                   c.fwd_flow, c.bwd_flow, c.fwd_flow_mask, c.bwd_flow_mask, device=c.world_view_transform.device)


class MiniCam:
    """A camera given by its matrices alone [REF scene/cameras.py:74-85]."""

    def __init__(self, width, height, fovy, fovx, znear, zfar, world_view_transform, full_proj_transform):
        self.image_width, self.image_height = width, height
        self.FoVy, self.FoVx = fovy, fovx
        self.znear, self.zfar = znear, zfar
        self.world_view_transform, self.full_proj_transform = world_view_transform, full_proj_transform
        self.camera_center = torch.inverse(self.world_view_transform)[3][:3]


def decode_records(records, device):
    """The images of ImageRecords as float32 [C, H, W] tensors on `device`: one png_decode.decode_files call for the PNG files (three
    channels composited over the records' background where they carry one, else all of the file's channels) and one
    jpeg_decode.decode_files call for the JPEG files (sync=True: files without restart markers go through jpeg_sync)."""
    from . import jpeg_decode, png_decode
    out = [None] * len(records)
    png = [i for i, r in enumerate(records) if r.kind == "png"]
    jpeg = [i for i, r in enumerate(records) if r.kind == "jpeg"]
    if len(png) + len(jpeg) != len(records):
        raise ValueError("load_cameras: an image record is neither \"png\" nor \"jpeg\": " + repr(next(r for r in records if r.kind not in ("png", "jpeg"))))
    if png:
        grounds = {None if records[i].background is None else tuple(float(v) for v in records[i].background) for i in png}
        if len(grounds) != 1:
            raise ValueError(f"load_cameras: one camera list with different backgrounds {sorted(grounds, key=repr)}")
        (ground,) = grounds
        ground = None if ground is None else torch.tensor(ground, dtype=torch.float32, device=device)
        for i, im in zip(png, png_decode.decode_files([records[i].path for i in png], device=device, dtype=torch.float32, background=ground)):
            out[i] = im
    if jpeg:
        for i, im in zip(jpeg, jpeg_decode.decode_files([records[i].path for i in jpeg], device=device, dtype=torch.float32, sync=True)):
            out[i] = im
    return out


def load_cameras(cam_infos, resolution_scale, args, device="cuda", _decode=None):
    """The reference's cameraList_from_camInfos [REF utils/camera_utils.py:72-134]: a SceneCamera per CameraInfo, uid = its place in
    the list; entries that are dicts {"cam", "fwd_cam", "bwd_cam"} come back as dicts of cameras (None stays None).  The reference's
    PILtoTorch ignores the resolution loadCam works out, so images are never resized, and `resolution_scale` / `args.resolution` change
    nothing here either.  `args.data_device` is where the finished images end up.  _decode: (records, device) -> images, for tests."""
    slots = []                                       # (entry, key or None, info), in list order
    for k, c in enumerate(cam_infos):
        if isinstance(c, dict):
            slots += [(k, key, c[key]) for key in ("cam", "fwd_cam", "bwd_cam") if c[key] is not None]
        else:
            slots.append((k, None, c))
    images = (_decode or decode_records)([info.image for _, _, info in slots], device)
    out = [{"cam": None, "fwd_cam": None, "bwd_cam": None} if isinstance(c, dict) else None for c in cam_infos]
    for (k, key, info), image in zip(slots, images):
        flows = {f: getattr(info, f) for f in ("fwd_flow", "bwd_flow", "fwd_flow_mask", "bwd_flow_mask")} if "fwd_flow" in info._fields else {}
        cam = SceneCamera(colmap_id=info.uid, R=info.R, T=info.T, FoVx=info.FovX, FoVy=info.FovY, image=image[:3],
                          gt_alpha_mask=image[3:4] if image.shape[0] == 4 else None, image_name=info.image_name, uid=k,
                          data_device=args.data_device, time=info.time, device=device, **flows)
        if key is None:
            out[k] = cam
        else:
            out[k][key] = cam
    return out


def _decoded_once(lists, device, decode):
    """Decode the image records of several camera lists in one `decode` call, every (file, background) once; returns a load_cameras
    `_decode` that hands the finished images out.  Cameras never share storage: SceneCamera's clamp makes each its own tensor."""
    key = lambda r: (r.path, r.kind, None if r.background is None else tuple(r.background))   # noqa: E731
    records = {}
    for cams in lists:
        for c in cams:
            for info in ([c[k] for k in ("cam", "fwd_cam", "bwd_cam") if c[k] is not None] if isinstance(c, dict) else [c]):
                records.setdefault(key(info.image), info.image)
    table = dict(zip(records, decode(list(records.values()), device)))
    return lambda wanted, device: [table[key(r)] for r in wanted]


def camera_to_JSON(id, camera):
    """A cameras.json entry of a CameraInfo [REF utils/camera_utils.py:136-156]."""
    w2c = np.zeros((4, 4))
    w2c[:3, :3] = camera.R.transpose()
    w2c[:3, 3] = camera.T
    w2c[3, 3] = 1.0
    c2w = np.linalg.inv(w2c)
    return {"id": id, "img_name": camera.image_name, "width": camera.width, "height": camera.height, "position": c2w[:3, 3].tolist(),
            "rotation": [row.tolist() for row in c2w[:3, :3]], "fy": fov2focal(camera.FovY, camera.height),
            "fx": fov2focal(camera.FovX, camera.width)}


def searchForMaxIteration(folder):
    """The largest N of the `iteration_N` entries of `folder` [REF utils/system_utils.py:26-28]."""
    return max(int(name.split("_")[-1]) for name in os.listdir(folder))


def _read_scene(args, ratio):
    """The SceneInfo of args.source_path, its kind told by what the folder holds, in the reference's precedence."""
    source = args.source_path
    holds = lambda name: os.path.exists(os.path.join(source, name))   # noqa: E731
    if holds("sparse"):
        return sceneLoadTypeCallbacks["Colmap"](source, args.images, args.eval)
    if holds("transforms_train.json"):
        return sceneLoadTypeCallbacks["Blender"](source, args.white_background, args.eval, max_time=args.max_time)
    if holds("points.npy"):
        return sceneLoadTypeCallbacks["Hyper"](source, args.max_time, ratio)
    raise ValueError(f"{source}: could not recognize the scene type (no sparse/, transforms_train.json or points.npy)")


class Scene:
    """[REF scene/__init__.py:21-107].  args: source_path, model_path, images, eval, white_background, max_time, resolution,
    data_device.  `device` and `_decode` (load_cameras') are not in the reference."""

    def __init__(self, args, gaussians, load_iteration=None, shuffle=True, resolution_scales=[1.0], ratio=0.5, *, device="cuda", _decode=None):
        self.model_path, self.loaded_iter, self.gaussians = args.model_path, None, gaussians
        if load_iteration:
            self.loaded_iter = searchForMaxIteration(os.path.join(self.model_path, "point_cloud")) if load_iteration == -1 else load_iteration
            print(f"Loading the trained model of iteration {self.loaded_iter}")
        self.train_cameras, self.test_cameras, self.render_cameras = {}, {}, {}
        scene_info = _read_scene(args, ratio)
        self.total_frame, self.cameras_extent = scene_info.total_frame, scene_info.nerf_normalization["radius"]

        if not self.loaded_iter:
            with open(scene_info.ply_path, "rb") as src, open(os.path.join(self.model_path, "input.ply"), "wb") as dst:
                dst.write(src.read())
            listed = list(scene_info.test_cameras or []) + list(scene_info.train_cameras or [])
            entries = [camera_to_JSON(k, cam["cam"] if isinstance(cam, dict) else cam) for k, cam in enumerate(listed)]
            with open(os.path.join(self.model_path, "cameras.json"), "w") as fp:
                json.dump(entries, fp)

        if shuffle:                                  # Python's global generator, train then test: a seeded run orders them as the reference does
            random.shuffle(scene_info.train_cameras)
            random.shuffle(scene_info.test_cameras)

        # A decoder call takes as long as its slowest file (a PNG of one deflate stream is one workgroup), however many files it holds:
        # the three lists, and every scale (nothing is resized), are decoded in ONE pass, a file that stands in two lists once.
        _decode = _decoded_once([scene_info.train_cameras, scene_info.test_cameras, scene_info.render_cameras or []], device, _decode or decode_records)
        for scale in resolution_scales:
            self.train_cameras[scale] = load_cameras(scene_info.train_cameras, scale, args, device, _decode)
            self.test_cameras[scale] = load_cameras(scene_info.test_cameras, scale, args, device, _decode)
            if len(scene_info.render_cameras or []):
                self.render_cameras[scale] = load_cameras(scene_info.render_cameras, scale, args, device, _decode)

        if self.loaded_iter:
            self.gaussians.load_ply(os.path.join(self.model_path, "point_cloud", "iteration_" + str(self.loaded_iter), "point_cloud.ply"))
        else:
            gaussians.create_from_pcd(scene_info.point_cloud, self.cameras_extent)

    def save(self, iteration):
        self.gaussians.save_ply(os.path.join(self.model_path, "point_cloud/iteration_{}".format(iteration), "point_cloud.ply"))

    def getTrainCameras(self, scale=1.0):
        return self.train_cameras[scale]

    def getTestCameras(self, scale=1.0):
        return self.test_cameras[scale]

    def getRenderCameras(self, scale=1.0):
        return self.render_cameras[scale]
