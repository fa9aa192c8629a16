"""Build-container script (needs the reference tree and Pillow; NOT run on the GPU box): writes three tiny datasets under
tests/golden/scenes/ from a fixed numpy seed, then runs the reference's own readers [REF scene/dataset_readers.py, scene/hyper_loader.py,
scene/colmap_loader.py, utils/camera_utils.py camera_to_JSON] on temporary copies of them and records what they return in
tests/golden/scenes.npz and tests/golden/scenes.json (data only).  tests/test_scene_host.py and tests/test_gpu_scene.py hold
gaussianprediction_amd.dataset_readers and gaussianprediction_amd.scene against the record.

The reference's modules are imported from its tree at run time, nothing is copied: `scene` and `utils` are entered into sys.modules as
bare packages whose __path__ is the reference's folder (its scene/__init__.py pulls in CUDA-only packages), with stand-ins for
`plyfile` (not installed: a reader and a writer of the one layout the readers use), `scene.gaussian_model` (BasicPointCloud alone) and
`pytorch3d` where it is missing.

Three things the reference cannot do as it stands, and what is recorded instead:
  * its COLMAP reader builds CameraInfo without `time`, a field without a default, and raises TypeError: the record is taken with a
    CameraInfo whose `time` defaults to 0.0;
  * its D-NeRF reader hands Image.fromarray an int8 array with mode "RGB"; the Pillow releases of its day took the array's bytes as
    they lie, the one installed here refuses the dtype: the record is taken with a fromarray that views int8 as uint8, which is
    those releases' behaviour;
  * its text intrinsics reader asserts PINHOLE, so the text model (which holds a SIMPLE_PINHOLE camera) is recorded only through
    read_points3D_text.

    python tests/golden/make_scene_vectors.py [/path/to/reference]
"""
import importlib
import io
import json
import os
import shutil
import struct
import sys
import tempfile
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
SCENES = os.path.join(HERE, "scenes")
W, H = 24, 16


# ---- the datasets -------------------------------------------------------------------------------------------------------------------
def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def rgba(rng, w, h):
    """Random colours; alpha 0, 255 and values in between, a third each."""
    px = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    kind = rng.integers(0, 3, size=(h, w))
    px[..., 3] = np.where(kind == 0, 0, np.where(kind == 1, 255, px[..., 3]))
    return px


def smooth_rgb(rng, w, h):
    y, x = np.mgrid[0:h, 0:w]
    a, b, c = rng.uniform(0.1, 0.5, size=3)
    px = np.stack([127 + 120 * np.sin(a * x + b * y), 127 + 120 * np.cos(b * x - c * y), 127 + 120 * np.sin(c * x) * np.cos(a * y)], axis=-1)
    return np.clip(px + rng.normal(0, 6, size=px.shape), 0, 255).astype(np.uint8)


def make_dnerf(rng):
    root = os.path.join(SCENES, "dnerf")
    times = {"train": [0.0, 0.2, 0.4, 0.6, 0.8, 1.0], "test": [0.1, 0.5, 0.9], "render": [0.0, 1.0]}
    for split, ts in times.items():
        os.makedirs(os.path.join(root, split), exist_ok=True)
        frames = []
        for k, t in enumerate(ts):
            c2w = np.eye(4)
            c2w[:3, :3] = rotation(rng)
            c2w[:3, 3] = rng.uniform(-4, 4, size=3)
            Image.fromarray(rgba(rng, W, H), "RGBA").save(os.path.join(root, split, f"r_{k:03d}.png"))
            frames.append({"file_path": f"./{split}/r_{k:03d}", "time": t, "transform_matrix": c2w.tolist()})
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as fp:
            json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames}, fp, indent=1)


def make_hyper(rng):
    from gaussianprediction_amd.io_formats import save_point_cloud_ply
    root = os.path.join(SCENES, "hyper")
    for d in ("camera", "rgb/2x"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    ids = [f"{k:06d}" for k in range(1, 13)]
    meta = {}
    for k, i in enumerate(ids):
        cam = {"orientation": rotation(rng).tolist(), "position": rng.uniform(-1, 1, size=3).tolist(), "focal_length": 51.3 + 0.01 * k,
               "principal_point": [24.0, 16.0], "skew": 0.0, "pixel_aspect_ratio": 1.0, "radial_distortion": [0.0, 0.0, 0.0],
               "tangential_distortion": [0.0, 0.0], "image_size": [2 * W, 2 * H]}
        with open(os.path.join(root, "camera", f"{i}.json"), "w") as fp:
            json.dump(cam, fp, indent=1)
        Image.fromarray(smooth_rgb(rng, W, H), "RGB").save(os.path.join(root, "rgb/2x", f"{i}.png"))
        meta[i] = {"warp_id": 3 * k + (k % 2), "appearance_id": k, "camera_id": 0}
    val = [ids[k] for k in (1, 5, 9, 11)]
    dump = lambda name, obj: json.dump(obj, open(os.path.join(root, name), "w"), indent=1)   # noqa: E731
    dump("scene.json", {"near": 0.01, "far": 2.0, "scale": 0.05, "center": [0.1, -0.2, 0.3]})
    dump("metadata.json", meta)
    dump("dataset.json", {"count": 12, "num_exemplars": 12, "ids": ids, "train_ids": ids, "val_ids": []})
    dump("dataset_val.json", {"count": 12, "num_exemplars": 8, "ids": ids, "train_ids": [i for i in ids if i not in val], "val_ids": val})
    pts = rng.uniform(-1, 1, size=(50, 3))
    np.save(os.path.join(root, "points.npy"), pts)
    save_point_cloud_ply(os.path.join(root, "points3D_downsample.ply"), pts, colors=rng.uniform(0, 1, size=(50, 3)), normals=np.zeros((50, 3)))


def make_colmap(rng):
    root = os.path.join(SCENES, "colmap")
    for d in ("images", "sparse/0", "sparse_txt/0"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    w, h = 32, 24
    cameras = [(1, 0, "SIMPLE_PINHOLE", [40.25, 16.0, 12.0]), (2, 1, "PINHOLE", [38.5, 41.75, 16.0, 12.0])]
    names = ["v_06.jpg", "v_02.jpg", "v_08.png", "v_04.jpg", "v_00.jpg", "v_07.png", "v_01.jpg", "v_05.png", "v_03.jpg"]     # ids 1..9
    images = []
    for k, name in enumerate(names):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        images.append((k + 1, q, rng.uniform(-3, 3, size=3), 1 + k % 2, name, rng.uniform(0, 32, size=(int(rng.integers(0, 5)), 2)), ))
        path = os.path.join(root, "images", name)
        if name.endswith(".jpg"):
            Image.fromarray(smooth_rgb(rng, w, h), "RGB").save(path, quality=90, subsampling=2)
        elif name == "v_05.png":
            Image.fromarray(rgba(rng, w, h), "RGBA").save(path)
        else:
            Image.fromarray(smooth_rgb(rng, w, h), "RGB").save(path)
    points = [(100 + 7 * k, rng.uniform(-2, 2, size=3), rng.integers(0, 256, size=3), float(rng.uniform(0, 2)),
               rng.integers(0, 9, size=(k % 6, 2))) for k in range(40)]

    def cameras_bin(rows):
        out = struct.pack("<Q", len(rows))
        for cid, model, _, params in rows:
            out += struct.pack("<iiQQ", cid, model, w, h) + struct.pack(f"<{len(params)}d", *params)
        return out

    out = struct.pack("<Q", len(images))
    for iid, q, t, cid, name, xys in images:
        out += struct.pack("<i4d3di", iid, *q, *t, cid) + name.encode() + b"\x00" + struct.pack("<Q", len(xys))
        for j, (x, y) in enumerate(xys):
            out += struct.pack("<ddq", x, y, -1 if j % 2 else 100 + 7 * j)
    pts = struct.pack("<Q", len(points))
    for pid, xyz, rgb, err, track in points:
        pts += struct.pack("<Q3d3BdQ", pid, *xyz, *(int(v) for v in rgb), err, len(track)) + b"".join(struct.pack("<ii", int(a), int(b)) for a, b in track)
    write = lambda rel, data: open(os.path.join(root, rel), "wb").write(data)   # noqa: E731
    write("sparse/0/cameras.bin", cameras_bin(cameras))
    write("sparse/0/images.bin", out)
    write("sparse/0/points3D.bin", pts)
    write("cameras_bad.bin", cameras_bin([(1, 4, "OPENCV", [40.0, 40.0, 16.0, 12.0, 0.01, -0.02, 0.0, 0.0])]))
    r = repr
    text = "# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n"
    text += "".join(f"{cid} {name} {w} {h} " + " ".join(r(float(p)) for p in params) + "\n" for cid, _, name, params in cameras)
    write("sparse_txt/0/cameras.txt", text.encode())
    text = "# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n#   POINTS2D[] as (X, Y, POINT3D_ID)\n"
    for iid, q, t, cid, name, xys in images:
        text += f"{iid} " + " ".join(r(float(v)) for v in (*q, *t)) + f" {cid} {name}\n"
        text += " ".join(f"{r(float(x))} {r(float(y))} {-1 if j % 2 else 100 + 7 * j}" for j, (x, y) in enumerate(xys)) + "\n"
    write("sparse_txt/0/images.txt", text.encode())
    text = "# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n"
    for pid, xyz, rgb, err, track in points:
        text += f"{pid} " + " ".join(r(float(v)) for v in xyz) + " " + " ".join(str(int(v)) for v in rgb) + f" {r(err)}" + \
            "".join(f" {int(a)} {int(b)}" for a, b in track) + "\n"
    write("sparse_txt/0/points3D.txt", text.encode())


# ---- the reference's readers, imported from its tree --------------------------------------------------------------------------------
def plyfile_stand_in():
    """`plyfile` as far as fetchPly and storePly use it: PlyData.read(path)['vertex'][name], PlyElement.describe(array, 'vertex'),
    PlyData([element]).write(path) -- binary little endian, the header plyfile writes for a structured array."""
    from gaussianprediction_amd.io_formats import read_ply_vertices
    mod = types.ModuleType("plyfile")
    kinds = {"f4": "float", "f8": "double", "u1": "uchar"}

    class PlyElement:
        def __init__(self, data, name):
            self.data, self.name = data, name

        @staticmethod
        def describe(data, name):
            return PlyElement(data, name)

    class PlyData:
        def __init__(self, elements):
            self.elements = elements

        @staticmethod
        def read(path):
            return {"vertex": read_ply_vertices(path)}

        def write(self, path):
            (el,) = self.elements
            head = "ply\nformat binary_little_endian 1.0\n" + f"element {el.name} {len(el.data)}\n" + \
                "".join(f"property {kinds[el.data.dtype[n].str[1:]]} {n}\n" for n in el.data.dtype.names) + "end_header\n"
            with open(path, "wb") as fp:
                fp.write(head.encode("ascii") + el.data.astype(el.data.dtype.newbyteorder("<")).tobytes())

    mod.PlyData, mod.PlyElement = PlyData, PlyElement
    return mod


def reference_modules():
    for name in ("scene", "utils"):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(REF, name)]
        sys.modules[name] = pkg
    sys.modules["plyfile"] = plyfile_stand_in()
    graphics = importlib.import_module("utils.graphics_utils")
    gm = types.ModuleType("scene.gaussian_model")
    gm.BasicPointCloud = graphics.BasicPointCloud
    sys.modules["scene.gaussian_model"] = gm
    try:
        import pytorch3d.transforms  # noqa: F401
    except ImportError:
        p3d, tr = types.ModuleType("pytorch3d"), types.ModuleType("pytorch3d.transforms")
        tr.matrix_to_quaternion = tr.quaternion_to_matrix = None
        p3d.transforms = tr
        sys.modules.update({"pytorch3d": p3d, "pytorch3d.transforms": tr})
    readers = importlib.import_module("scene.dataset_readers")
    camera_utils = importlib.import_module("utils.camera_utils")
    colmap = importlib.import_module("scene.colmap_loader")
    pil = types.SimpleNamespace(open=Image.open, fromarray=lambda a, mode=None: Image.fromarray(a.view(np.uint8) if a.dtype == np.int8 else a, mode))
    readers.Image = pil                                                     # (int8 bytes as they lie: see the docstring)
    ref_info = readers.CameraInfo
    readers.CameraInfo = lambda **kw: ref_info(**{"time": 0.0, **kw})      # (the COLMAP reader leaves `time` out: see the docstring)
    return readers, camera_utils.camera_to_JSON, colmap


def record_scene(tag, info, arrays, table, to_json, images=False):
    entry = {"total_frame": int(info.total_frame), "splits": {}, "cameras_json": []}
    for split in ("train", "test", "render"):
        cams = getattr(info, f"{split}_cameras")
        entry["splits"][split] = {"image_name": [c.image_name for c in cams], "uid": [int(c.uid) for c in cams],
                                  "width": [int(c.width) for c in cams], "height": [int(c.height) for c in cams]}
        arrays[f"{tag}/{split}/R"] = np.array([np.asarray(c.R, dtype=np.float64) for c in cams]).reshape(len(cams), 3, 3)
        arrays[f"{tag}/{split}/T"] = np.array([np.asarray(c.T, dtype=np.float64) for c in cams]).reshape(len(cams), 3)
        arrays[f"{tag}/{split}/FovX"] = np.array([float(c.FovX) for c in cams])
        arrays[f"{tag}/{split}/FovY"] = np.array([float(c.FovY) for c in cams])
        arrays[f"{tag}/{split}/time"] = np.array([float(np.asarray(c.time).reshape(-1)[0]) for c in cams])
        if images:
            arrays[f"{tag}/{split}/image"] = np.array([np.array(c.image) for c in cams], dtype=np.uint8).reshape(len(cams), H, W, 3)
    arrays[f"{tag}/translate"] = np.asarray(info.nerf_normalization["translate"], dtype=np.float64)
    arrays[f"{tag}/radius"] = np.float64(info.nerf_normalization["radius"])
    listed = list(info.test_cameras) + list(info.train_cameras)             # (Scene's order: test cameras first)
    entry["cameras_json"] = [to_json(k, c) for k, c in enumerate(listed)]
    table[tag] = entry


def main():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    shutil.rmtree(SCENES, ignore_errors=True)
    rng = np.random.default_rng(20261020)
    make_dnerf(rng)
    make_hyper(rng)
    make_colmap(rng)
    readers, to_json, colmap = reference_modules()
    arrays, table = {}, {}
    sink = io.StringIO()
    stdout, sys.stdout = sys.stdout, sink                                   # (the readers print progress)
    try:
        with tempfile.TemporaryDirectory() as tmp:
            work = os.path.join(tmp, "scenes")
            shutil.copytree(SCENES, work)
            d = os.path.join(work, "dnerf")
            for tag, kw in (("dnerf_eval_black", dict(white_background=False, eval=True)), ("dnerf_eval_white", dict(white_background=True, eval=True)),
                            ("dnerf_noeval", dict(white_background=False, eval=False)),
                            ("dnerf_t06", dict(white_background=False, eval=True, max_time=0.6))):
                np.random.seed(7)                                           # (the first call writes the random points3d.ply)
                record_scene(tag, readers.readNerfSyntheticInfo(d, **kw), arrays, table, to_json, images=True)
            hy = os.path.join(work, "hyper")
            for variant in ("noval", "val"):
                if variant == "val":
                    shutil.copyfile(os.path.join(hy, "dataset_val.json"), os.path.join(hy, "dataset.json"))
                for max_time in (1.0, 0.75):
                    record_scene(f"hyper_{variant}_{'full' if max_time == 1.0 else 't075'}", readers.readHyperDataInfos(hy, max_time, 0.5), arrays, table, to_json)
            co = os.path.join(work, "colmap")
            for tag, ev in (("colmap_eval", True), ("colmap_noeval", False)):
                record_scene(tag, readers.readColmapSceneInfo(co, None, ev), arrays, table, to_json)
            for kind, fn, rel in (("bin", colmap.read_points3D_binary, "sparse/0/points3D.bin"), ("txt", colmap.read_points3D_text, "sparse_txt/0/points3D.txt")):
                xyz, rgb, err = fn(os.path.join(co, rel))
                arrays[f"colmap_points_{kind}/xyz"], arrays[f"colmap_points_{kind}/rgb"], arrays[f"colmap_points_{kind}/error"] = xyz, rgb, err
            ply = readers.fetchPly(os.path.join(co, "sparse/0/points3D.ply"))   # (what the reference's conversion wrote, read back)
            arrays["colmap_ply/points"], arrays["colmap_ply/colors"], arrays["colmap_ply/normals"] = ply.points, ply.colors, ply.normals
    finally:
        sys.stdout = stdout
    np.savez_compressed(os.path.join(HERE, "scenes.npz"), **arrays)
    with open(os.path.join(HERE, "scenes.json"), "w") as fp:
        json.dump(table, fp, indent=1)
    size = sum(os.path.getsize(os.path.join(b, f)) for b, _, fs in os.walk(SCENES) for f in fs)
    print(f"wrote {SCENES} ({size} bytes), scenes.npz ({os.path.getsize(os.path.join(HERE, 'scenes.npz'))} bytes), scenes.json: {sorted(table)}")


if __name__ == "__main__":
    main()
