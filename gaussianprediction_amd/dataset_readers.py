"""The dataset readers behind `Scene` (host only: numpy and the standard library; nothing here imports device code or decodes a pixel):
D-NeRF / Blender folders, HyperNeRF folders and COLMAP sparse models, returning the reference's `SceneInfo` of `CameraInfo`s
[REF scene/dataset_readers.py, scene/hyper_loader.py, scene/colmap_loader.py], written from the file layouts.

`CameraInfo.image` is an `ImageRecord`, not a decoded image: the path, the container kind, the size and channel count read from the
file's header alone, and the background the D-NeRF reader composites RGBA files over (None elsewhere).  scene.load_cameras turns a
whole list of records into device images with one png_decode and one jpeg_decode call; a record has `.size` = (W, H), which is all
the reference's loadCam reads of a PIL image before it converts it.

The COLMAP files are read into memory once and sliced with np.frombuffer; 2D points and tracks are stepped over, never unpacked."""
from __future__ import annotations

import json
import os
from collections import namedtuple
from typing import NamedTuple

import numpy as np

from .cameras import focal2fov, fov2focal, world_to_view
from .io_formats import read_ply_vertices

SH_C0 = 0.28209479177387814
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
RANDOM_CLOUD_POINTS = 50_000


BasicPointCloud = namedtuple("BasicPointCloud", "points colors normals")


class ImageRecord(NamedTuple):
    """What the reference did to an image file before loadCam, as data."""
    path: str
    kind: str                   # "png" or "jpeg"
    width: int
    height: int
    channels: int
    background: object = None   # [r, g, b] in 0..1 to composite an RGBA file over (the D-NeRF reader), or None

    @property
    def size(self):
        return self.width, self.height


# the reference's field names; `time` has a default because the COLMAP reader has none to give
CameraInfo = namedtuple("CameraInfo", "uid R T FovY FovX image image_path image_name width height time", defaults=(0.0,))
SceneInfo = namedtuple("SceneInfo", "point_cloud train_cameras test_cameras render_cameras nerf_normalization ply_path total_frame", defaults=(1,))


def SH2RGB(sh):
    return sh * SH_C0 + 0.5


# ---- image headers ------------------------------------------------------------------------------------------------------------------
_PNG_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def image_record(path, background=None):
    """The ImageRecord of a PNG or JPEG file from its header: the IHDR chunk, or the marker walk up to the frame header."""
    path = os.fspath(path)
    with open(path, "rb") as fp:
        head = fp.read(65536)
        if head[:8] == PNG_SIGNATURE:
            if len(head) < 33 or head[12:16] != b"IHDR":
                raise ValueError(f"{path}: a PNG file without an IHDR chunk")
            width, height = int.from_bytes(head[16:20], "big"), int.from_bytes(head[20:24], "big")
            if head[25] not in _PNG_CHANNELS:
                raise ValueError(f"{path}: PNG colour type {head[25]}")
            return ImageRecord(path, "png", width, height, _PNG_CHANNELS[head[25]], background)
        if head[:2] != b"\xff\xd8":
            raise ValueError(f"{path} is neither a PNG nor a JPEG file")
        data, pos = head, 2
        while True:
            if pos + 4 > len(data):
                more = fp.read()
                if not more:
                    raise ValueError(f"{path}: a JPEG file without a frame header")
                data += more
                continue
            if data[pos] != 0xff:
                raise ValueError(f"{path}: byte {pos}: a JPEG marker was expected")
            m = data[pos + 1]
            if m == 0xff:
                pos += 1
                continue
            length = int.from_bytes(data[pos + 2:pos + 4], "big")
            if 0xc0 <= m <= 0xcf and m not in (0xc4, 0xc8, 0xcc):
                if pos + 10 > len(data):
                    data += fp.read()
                if pos + 10 > len(data):
                    raise ValueError(f"{path}: a JPEG frame header runs past the end of the file")
                height, width = int.from_bytes(data[pos + 5:pos + 7], "big"), int.from_bytes(data[pos + 7:pos + 9], "big")
                return ImageRecord(path, "jpeg", width, height, data[pos + 9], background)
            if m == 0xda or m == 0xd9 or length < 2:
                raise ValueError(f"{path}: a JPEG file without a frame header")
            pos += 2 + length


# ---- point clouds -------------------------------------------------------------------------------------------------------------------
def store_ply(path, xyz, rgb):
    """The point cloud file the reference's storePly writes [REF scene/dataset_readers.py:120-135]: binary little endian, float
    x y z nx ny nz (normals zero), uchar red green blue -- the colours cast as numpy casts floats to bytes (truncation)."""
    xyz, rgb = np.asarray(xyz), np.asarray(rgb)
    table = np.zeros(xyz.shape[0], dtype=[(n, "<f4") for n in ("x", "y", "z", "nx", "ny", "nz")] + [(n, "u1") for n in ("red", "green", "blue")])
    for k, n in enumerate(("x", "y", "z")):
        table[n] = xyz[:, k]
    for k, n in enumerate(("red", "green", "blue")):
        table[n] = rgb[:, k].astype(np.uint8)
    header = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {table.shape[0]}\n" + \
        "".join(f"property float {n}\n" for n in ("x", "y", "z", "nx", "ny", "nz")) + \
        "".join(f"property uchar {n}\n" for n in ("red", "green", "blue")) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(table.tobytes())


def fetch_ply(path):
    """BasicPointCloud of a PLY file: positions, colours / 255.0, normals [REF scene/dataset_readers.py:112-118]."""
    v = read_ply_vertices(path)
    cols = lambda names: np.stack([v[n] for n in names], axis=1)   # noqa: E731  (row-major [N, 3]: create_from_pcd keeps the layout it is given)
    return BasicPointCloud(points=cols(("x", "y", "z")), colors=cols(("red", "green", "blue")) / 255.0, normals=cols(("nx", "ny", "nz")))


def _fetch_or_none(path):
    try:
        return fetch_ply(path)
    except (OSError, ValueError, KeyError):
        return None


# ---- normalisation ------------------------------------------------------------------------------------------------------------------
def getNerfppNorm(cam_infos):
    """{"translate": -centre, "radius": 1.1 x the largest distance of a camera centre from their mean}.  The reference takes the
    centres from its float32 world-to-view matrix [REF utils/graphics_utils.py:38-49], so they, their mean and the radius are float32
    numbers: the same here (cameras.world_to_view is that matrix), or the radius would differ in the eighth digit."""
    centres = np.hstack([np.linalg.inv(world_to_view(c.R, c.T))[:3, 3:4] for c in cam_infos])      # [3, n] float32
    centre = np.mean(centres, axis=1, keepdims=True)
    radius = np.max(np.linalg.norm(centres - centre, axis=0, keepdims=True)) * 1.1
    return {"translate": -centre.flatten(), "radius": radius}


# ---- D-NeRF / Blender ---------------------------------------------------------------------------------------------------------------
def _transforms_cameras(path, name, white_background, extension, max_time=1.0):
    """(the frames with time < max_time, the others) of one transforms_*.json."""
    with open(os.path.join(path, name)) as fp:
        contents = json.load(fp)
    angle_x = contents["camera_angle_x"]
    background = [1, 1, 1] if white_background else [0, 0, 0]
    before, after = [], []
    for idx, frame in enumerate(contents["frames"]):
        file = os.path.join(path, frame["file_path"] + extension)
        c2w = np.array(frame["transform_matrix"], dtype=np.float64)
        c2w[:3, 1:3] *= -1                       # OpenGL axes (y up, z back) -> COLMAP's (y down, z forward)
        view = np.linalg.inv(c2w)
        record = image_record(file, background)
        if record.channels == 3:
            # the reference composites every file after convert("RGBA"); an opaque pixel comes out as the byte it was, for every byte
            # and either background ((v / 255.0) * 1.0 + b * 0.0) * 255.0 truncates to v: tests/test_scene_host.py), so there is nothing to do
            record = record._replace(background=None)
        elif record.channels != 4:
            raise ValueError(f"{file}: a D-NeRF image with {record.channels} channel(s): RGBA and RGB files are read")
        info = CameraInfo(uid=idx, R=view[:3, :3].T, T=view[:3, 3], FovY=focal2fov(fov2focal(angle_x, record.width), record.height), FovX=angle_x,
                          image=record, image_path=file, image_name=os.path.splitext(os.path.basename(file))[0], width=record.width,
                          height=record.height, time=np.array([frame["time"]]))
        (before if float(frame["time"]) < max_time else after).append(info)
    return before, after


def readNerfSyntheticInfo(path, white_background, eval, extension=".png", max_time=1.0):
    train, test = _transforms_cameras(path, "transforms_train.json", white_background, extension, max_time)
    if max_time == 1.0:
        test, _ = _transforms_cameras(path, "transforms_test.json", white_background, extension)
    if os.path.isfile(os.path.join(path, "transforms_render.json")):
        render, _ = _transforms_cameras(path, "transforms_render.json", white_background, extension)
    else:
        render = test
    if not eval:
        train.extend(test)
        test = []
    norm = getNerfppNorm(train)
    cloud = os.path.join(path, "points3d.ply")
    if not os.path.isfile(cloud):
        # no sparse model comes with these scenes: random points inside the synthetic scenes' bounds, from numpy's global generator
        xyz = np.random.random((RANDOM_CLOUD_POINTS, 3)) * 2.6 - 1.3
        shs = np.random.random((RANDOM_CLOUD_POINTS, 3)) / 255.0
        store_ply(cloud, xyz, SH2RGB(shs) * 255)
    return SceneInfo(point_cloud=_fetch_or_none(cloud), train_cameras=train, test_cameras=test, render_cameras=render,
                     nerf_normalization=norm, ply_path=cloud)


# ---- HyperNeRF ----------------------------------------------------------------------------------------------------------------------
def _hyper_split(ids, val_ids, train_ids, times, max_time):
    n = len(ids)
    if max_time < 1.0:
        if not val_ids:
            train = [i for i in range(n) if i % 4 == 0 and times[i] < max_time]
            test = [i for i in range(n) if (i - 2) % 4 == 0 and times[i] >= max_time]
        else:
            train = [i for i in range(n) if ids[i] in train_ids and times[i] < max_time]
            test = [i for i in range(n) if ids[i] in val_ids and times[i] >= max_time]
        if not train or not test:
            raise AssertionError(f"max_time = {max_time} leaves {len(train)} training and {len(test)} test frames")
        return train, test
    if not val_ids:
        train = [i for i in range(n) if i % 4 == 0]
        return train, [i + 2 for i in train[:-1]]
    return [i for i in range(n) if ids[i] in train_ids], [i for i in range(n) if ids[i] in val_ids]


def readHyperDataInfos(datadir, max_time=1.0, resize=0.5):
    datadir = os.path.expanduser(os.fspath(datadir))
    load = lambda name: json.load(open(os.path.join(datadir, name)))   # noqa: E731
    load("scene.json")                                                   # (near, far, scale, center: read by nothing downstream)
    meta, dataset = load("metadata.json"), load("dataset.json")
    ids, val_ids = dataset["ids"], dataset["val_ids"]
    warp = [meta[i]["warp_id"] for i in ids]
    times = [w / max(warp) for w in warp]
    train, test = _hyper_split(ids, val_ids, dataset["train_ids"] if val_ids else [], times, max_time)
    folder = f"{datadir}/rgb/{int(1 / resize)}x"
    cams = []
    for i in ids:
        with open(f"{datadir}/camera/{i}.json") as fp:
            cam = json.load(fp)
        # the reference holds these as float32 arrays and its products stay in float32: the same here, so that R and T are the same numbers
        orientation, position = np.array(cam["orientation"], np.float32), np.array(cam["position"], np.float32)
        cams.append((orientation.T, -position @ orientation.T, float(np.float32(cam["focal_length"])), cam["image_size"]))
    full_w, full_h = int(cams[0][3][0]), int(cams[0][3][1])             # the camera JSON's image_size, not the loaded image's

    def info(uid, i, record, time):
        R, T, focal, _ = cams[i]
        return CameraInfo(uid=uid, R=R, T=T, FovY=focal2fov(focal, full_h), FovX=focal2fov(focal, full_w), image=record, image_path=folder,
                          image_name=f"{ids[i]}.png", width=record.width if record else full_w, height=record.height if record else full_h, time=time)

    def loaded(split):
        return [info(i, i, image_record(f"{folder}/{ids[i]}.png"), np.array([times[i]]).astype(np.float32)) for i in split]

    train_cams, test_cams = loaded(train), loaded(test)
    cloud = os.path.join(datadir, "points3D_downsample.ply")
    norm = getNerfppNorm([info(u, i, None, times[i]) for u, i in enumerate(train)])
    return SceneInfo(point_cloud=fetch_ply(cloud), train_cameras=train_cams, test_cameras=test_cams, render_cameras=test_cams,
                     nerf_normalization=norm, ply_path=cloud, total_frame=len(ids))


# ---- COLMAP -------------------------------------------------------------------------------------------------------------------------
# model id -> (name, number of parameters), COLMAP's published camera model table
COLMAP_CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8),
                        5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4),
                        9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}
_IMAGE_HEAD = np.dtype([("id", "<i4"), ("q", "<f8", 4), ("t", "<f8", 3), ("camera", "<i4")])              # 64 bytes, unaligned
_POINT_HEAD = np.dtype([("id", "<u8"), ("xyz", "<f8", 3), ("rgb", "u1", 3), ("error", "<f8")])            # 43 bytes, unaligned


class ColmapCamera(NamedTuple):
    id: int
    model: str
    width: int
    height: int
    params: np.ndarray


class ColmapImage(NamedTuple):
    id: int
    qvec: np.ndarray            # (w, x, y, z)
    tvec: np.ndarray
    camera_id: int
    name: str


class _Bytes:
    """A file held in memory, read front to back; a read past its end raises ValueError naming the file."""

    def __init__(self, path):
        self.path = os.fspath(path)
        with open(self.path, "rb") as fp:
            self.data = fp.read()
        self.pos = 0

    def skip(self, n):
        if n < 0 or self.pos + n > len(self.data):
            raise ValueError(f"{self.path}: truncated at byte {len(self.data)} ({n} bytes wanted at byte {self.pos})")
        self.pos += n
        return self.pos - n

    def take(self, dtype, count=1):
        dtype = np.dtype(dtype)
        return np.frombuffer(self.data, dtype=dtype, count=count, offset=self.skip(dtype.itemsize * count))

    def u64(self):
        return int(self.take("<u8")[0])


def qvec2rotmat(qvec):
    """Rotation matrix of a quaternion (w, x, y, z)."""
    w, x, y, z = (float(v) for v in qvec)
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])


def read_cameras_bin(path):
    """cameras.bin: u64 n, then n x (i32 id, i32 model, u64 W, u64 H, f64 params[k of the model]) -> {id: ColmapCamera}."""
    f = _Bytes(path)
    out = {}
    for _ in range(f.u64()):
        cid, model = (int(v) for v in f.take("<i4", 2))
        width, height = (int(v) for v in f.take("<u8", 2))
        if model not in COLMAP_CAMERA_MODELS:
            raise ValueError(f"{f.path}: camera {cid} has model id {model}, which COLMAP's table does not list")
        name, k = COLMAP_CAMERA_MODELS[model]
        out[cid] = ColmapCamera(cid, name, width, height, f.take("<f8", k).copy())
    return out


def read_images_bin(path):
    """images.bin: u64 n, then n x (i32 id, f64 q[4], f64 t[3], i32 camera_id, a NUL-terminated name, u64 m, m x 24 bytes of 2D
    points, which are stepped over) -> {id: ColmapImage}, in file order."""
    f = _Bytes(path)
    out = {}
    for _ in range(f.u64()):
        head = f.take(_IMAGE_HEAD)[0]
        end = f.data.find(b"\x00", f.pos)
        if end < 0:
            raise ValueError(f"{f.path}: truncated inside an image name at byte {f.pos}")
        name = f.data[f.pos:end].decode("utf-8")
        f.pos = end + 1
        f.skip(24 * f.u64())
        out[int(head["id"])] = ColmapImage(int(head["id"]), head["q"].copy(), head["t"].copy(), int(head["camera"]), name)
    return out


def read_points3D_bin(path):
    """points3D.bin: u64 n, then n x (u64 id, f64 xyz[3], u8 rgb[3], f64 error, u64 L, L x (i32, i32), stepped over)
    -> (xyz [n, 3] float64, rgb [n, 3] float64, error [n, 1] float64)."""
    f = _Bytes(path)
    n = f.u64()
    at = np.empty(n, dtype=np.int64)
    for i in range(n):                           # (only the track lengths are looked at here: they say where the next point begins)
        at[i] = f.skip(_POINT_HEAD.itemsize)
        f.skip(8 * f.u64())
    raw = np.frombuffer(f.data, dtype=np.uint8)[at[:, None] + np.arange(_POINT_HEAD.itemsize)]
    heads = np.ascontiguousarray(raw).view(_POINT_HEAD).reshape(n)
    return heads["xyz"].astype(np.float64), heads["rgb"].astype(np.float64), heads["error"].astype(np.float64).reshape(n, 1)


def _text_rows(path):
    with open(path, "r") as fp:
        lines = fp.read().split("\n")
    return lines


def read_cameras_txt(path):
    """cameras.txt: `id MODEL W H params...` per line -> {id: ColmapCamera}."""
    out = {}
    for line in _text_rows(path):
        tok = line.split()
        if not tok or tok[0].startswith("#"):
            continue
        out[int(tok[0])] = ColmapCamera(int(tok[0]), tok[1], int(tok[2]), int(tok[3]), np.array([float(v) for v in tok[4:]]))
    return out


def read_images_txt(path):
    """images.txt: `id qw qx qy qz tx ty tz camera_id name`, then one line of 2D points (stepped over) -> {id: ColmapImage}."""
    out, lines, k = {}, _text_rows(path), 0
    while k < len(lines):
        tok = lines[k].split()
        k += 1
        if not tok or tok[0].startswith("#"):
            continue
        if len(tok) < 10:
            raise ValueError(f"{path}: line {k}: an image line has ten fields")
        out[int(tok[0])] = ColmapImage(int(tok[0]), np.array([float(v) for v in tok[1:5]]), np.array([float(v) for v in tok[5:8]]), int(tok[8]), tok[9])
        k += 1                                   # the line of 2D points, empty or not
    return out


def read_points3D_txt(path):
    """points3D.txt: `id x y z r g b error track...` per line -> what read_points3D_bin returns."""
    rows = [line.split()[1:8] for line in _text_rows(path) if line.strip() and not line.lstrip().startswith("#")]
    table = np.array(rows, dtype=np.float64).reshape(len(rows), 7)
    return table[:, 0:3].copy(), table[:, 3:6].copy(), table[:, 6:7].copy()


def _binary_or_text(folder, stem, read_bin, read_txt):
    try:
        return read_bin(os.path.join(folder, stem + ".bin"))
    except (OSError, ValueError):
        return read_txt(os.path.join(folder, stem + ".txt"))


def readColmapSceneInfo(path, images, eval, llffhold=8):
    sparse = os.path.join(path, "sparse/0")
    try:
        extrinsics, intrinsics = read_images_bin(os.path.join(sparse, "images.bin")), read_cameras_bin(os.path.join(sparse, "cameras.bin"))
    except (OSError, ValueError):
        extrinsics, intrinsics = read_images_txt(os.path.join(sparse, "images.txt")), read_cameras_txt(os.path.join(sparse, "cameras.txt"))
    folder = os.path.join(path, "images" if images is None else images)
    cams = []
    for extr in extrinsics.values():
        intr = intrinsics[extr.camera_id]
        if intr.model == "SIMPLE_PINHOLE":
            fx = fy = intr.params[0]
        elif intr.model == "PINHOLE":
            fx, fy = intr.params[0], intr.params[1]
        else:
            raise ValueError(f"{sparse}: camera {intr.id} has model {intr.model}: only undistorted datasets (PINHOLE or SIMPLE_PINHOLE) are read")
        file = os.path.join(folder, os.path.basename(extr.name))
        cams.append(CameraInfo(uid=intr.id, R=qvec2rotmat(extr.qvec).T, T=np.array(extr.tvec), FovY=focal2fov(fy, intr.height),
                               FovX=focal2fov(fx, intr.width), image=image_record(file), image_path=file,
                               image_name=os.path.basename(file).split(".")[0], width=intr.width, height=intr.height))
    cams.sort(key=lambda c: c.image_name)
    train = [c for k, c in enumerate(cams) if k % llffhold != 0] if eval else cams
    test = [c for k, c in enumerate(cams) if k % llffhold == 0] if eval else []
    norm = getNerfppNorm(train)
    cloud = os.path.join(sparse, "points3D.ply")
    if not os.path.isfile(cloud):
        xyz, rgb, _ = _binary_or_text(sparse, "points3D", read_points3D_bin, read_points3D_txt)
        store_ply(cloud, xyz, rgb)
    return SceneInfo(point_cloud=_fetch_or_none(cloud), train_cameras=train, test_cameras=test, render_cameras=test,
                     nerf_normalization=norm, ply_path=cloud)


sceneLoadTypeCallbacks = {"Colmap": readColmapSceneInfo, "Blender": readNerfSyntheticInfo, "Hyper": readHyperDataInfos}
