"""Loading a scene, measured on the GPU: `Scene(...)` on a D-NeRF-sized folder (200 RGBA PNG files of 800 x 800, eval split) and on a
HyperNeRF-sized one (80 frames, 40 + 39 of them loaded, RGB PNG files of 1352 x 1014 -- the size of bench.py's scene -- under rgb/2x/), both
written by Pillow from synthetic renders (25 and 20 distinct frames, each stored under several names), against the same readers with
the images decoded by Pillow on the host, one file after the other, composited in numpy and copied up one by one, every camera list on
its own: the reference's way [REF scene/dataset_readers.py:210-218, utils/general_utils.py:21-27, scene/cameras.py:44,
scene/__init__.py:79-86].  That host path lives here only, as load_cameras(_decode=...); the package has none.  A third row decodes
list by list on the device, which is what Scene's one pass over all lists is measured against.  Prints, per folder, the wall time of
each (first call and the best of two more), the decoder passes = reads of the device (decode_stage.once reads the status words once
per pass), and whether the images agree bit for bit.  Writes profiles/scene_probe.txt.

    python tools/scene_probe.py            (needs a GPU and Pillow)
"""
import json
import os
import shutil
import sys
import tempfile
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from gaussianprediction_amd import GaussianModel, decode_stage, render  # noqa: E402
from gaussianprediction_amd import dataset_readers as DR  # noqa: E402
from gaussianprediction_amd.cameras import orbit_cameras  # noqa: E402
from gaussianprediction_amd.io_formats import save_point_cloud_ply  # noqa: E402
from gaussianprediction_amd.scene import Scene, camera_to_JSON, load_cameras  # noqa: E402
from gaussianprediction_amd.scene_synth import SceneSpec, make_gaussians  # noqa: E402

DEV = torch.device("cuda", 0)


class NoModel:
    """The loader alone is timed: what Scene hands the model is dropped."""

    def create_from_pcd(self, pcd, extent):
        pass


def renders(n, W, H, arc):
    margs = SimpleNamespace(beta=0.1, d=4, w=256, feature_dim=32, second_stage_iteration=30000, third_stage_iteration=40000, jointly_iteration=1000,
                            nearest_num=6, norm_rotation=True, step_opacity=False, step_opacity_iteration=5000, opacity_type="implicit",
                            xyz_noise_iteration=0)
    raw = make_gaussians(SceneSpec(n_gaussians=200_000, scale_lo=0.01, scale_hi=0.04, seed=9), device=DEV)
    pc = GaussianModel(3, margs)
    pc.set_inputDim(12, 60)
    pc.create_from_tensors(raw["xyz"], raw["features_dc"], raw["features_rest"], raw["scaling"], raw["rotation"], raw["opacity"], raw["motion_feature"])
    cams = orbit_cameras(n, 4.0, 0.69, W, H, arc_deg=arc, device=DEV)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    with torch.no_grad():
        out = [render(c, pc, pipe, torch.zeros(3, device=DEV), time=torch.from_numpy(c.time).to(DEV), it=1)["render"].clamp(0, 1) for c in cams]
    return cams, [(x * 255 + 0.5).floor().to(torch.uint8).permute(1, 2, 0).cpu().numpy() for x in out], raw["xyz"][:50_000].cpu().numpy()


def dnerf_folder(root, n=200, distinct=25, W=800, H=800):
    cams, frames, pts = renders(distinct, W, H, 360.0)
    os.makedirs(os.path.join(root, "train"))
    first = []
    for k, px in enumerate(frames):                                                # alpha: 0 off the object, 255 inside, a ramp between
        alpha = np.clip(px.max(axis=2).astype(np.float32) * 6, 0, 255).astype(np.uint8)
        first.append(os.path.join(root, "train", f"r_{k:03d}.png"))
        Image.fromarray(np.dstack([px, alpha]), "RGBA").save(first[-1])
    listed = {"train": [], "test": []}
    for k in range(n):
        if k >= distinct:
            shutil.copyfile(first[k % distinct], os.path.join(root, "train", f"r_{k:03d}.png"))
        w2c = np.eye(4)
        w2c[:3, :3], w2c[:3, 3] = cams[k % distinct].R.T, cams[k % distinct].T
        c2w = np.linalg.inv(w2c)
        c2w[:3, 1:3] *= -1
        listed["train" if k < 150 else "test"].append({"file_path": f"./train/r_{k:03d}", "time": (k % 150) / 150, "transform_matrix": c2w.tolist()})
    for name, fr in listed.items():
        with open(os.path.join(root, f"transforms_{name}.json"), "w") as fp:
            json.dump({"camera_angle_x": cams[0].FoVx, "frames": fr}, fp)
    DR.store_ply(os.path.join(root, "points3d.ply"), pts, np.full(pts.shape, 128.0))
    return sum(os.path.getsize(os.path.join(root, "train", f)) for f in os.listdir(os.path.join(root, "train")))


def hyper_folder(root, n=160, distinct=20, W=1352, H=1014):
    cams, frames, pts = renders(distinct, W, H, 40.0)
    for d in ("camera", "rgb/2x"):
        os.makedirs(os.path.join(root, d))
    ids = [f"{k:06d}" for k in range(n)]
    for k, i in enumerate(ids):
        c = cams[k % distinct]
        if k < distinct:
            Image.fromarray(frames[k], "RGB").save(os.path.join(root, "rgb/2x", f"{i}.png"))
        elif k % 2 == 0:                                                           # (only every second frame is ever loaded)
            shutil.copyfile(os.path.join(root, "rgb/2x", f"{ids[k % distinct]}.png"), os.path.join(root, "rgb/2x", f"{i}.png"))
        with open(os.path.join(root, "camera", f"{i}.json"), "w") as fp:
            json.dump({"orientation": c.R.T.tolist(), "position": (-c.R @ c.T).tolist(), "focal_length": 2 * W / (2 * np.tan(c.FoVx / 2)),
                       "principal_point": [W, H], "skew": 0.0, "pixel_aspect_ratio": 1.0, "radial_distortion": [0, 0, 0],
                       "tangential_distortion": [0, 0], "image_size": [2 * W, 2 * H]}, fp)
    dump = lambda name, obj: json.dump(obj, open(os.path.join(root, name), "w"))   # noqa: E731
    dump("scene.json", {"near": 0.01, "far": 10.0, "scale": 1.0, "center": [0, 0, 0]})
    dump("metadata.json", {i: {"warp_id": k, "appearance_id": k, "camera_id": 0} for k, i in enumerate(ids)})
    dump("dataset.json", {"count": n, "num_exemplars": n, "ids": ids, "train_ids": ids, "val_ids": []})
    np.save(os.path.join(root, "points.npy"), pts)
    save_point_cloud_ply(os.path.join(root, "points3D_downsample.ply"), pts, colors=np.full(pts.shape, 0.5), normals=np.zeros_like(pts))
    folder = os.path.join(root, "rgb/2x")
    return sum(os.path.getsize(os.path.join(folder, f)) for f in os.listdir(folder))


def pillow_decode(records, device):
    """The reference's image path, file by file: Image.open, the D-NeRF composite in numpy where the record asks for it, / 255.0,
    permute, and one host-to-device copy per image."""
    out = []
    for r in records:
        image = Image.open(r.path)
        if r.background is not None:
            norm = np.array(image.convert("RGBA")) / 255.0
            arr = norm[:, :, :3] * norm[:, :, 3:4] + np.array(r.background) * (1 - norm[:, :, 3:4])
            px = (arr * 255.0).astype(np.uint8)                    # (the reference's np.byte holds the same eight bits)
        else:
            px = np.array(image)
        out.append((torch.from_numpy(px) / 255.0).permute(2, 0, 1).to(device))
    return out


def timed(make):
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scene = make()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts[0], min(ts[1:]), scene


def list_by_list(args, ratio, decode):
    """Scene's sequence with every camera list decoded on its own, the render list again although it is the test list: the reference's
    [REF scene/__init__.py:44-86].  decode: load_cameras' _decode (None: the device decoders)."""
    if os.path.exists(os.path.join(args.source_path, "transforms_train.json")):
        info = DR.readNerfSyntheticInfo(args.source_path, args.white_background, args.eval, max_time=args.max_time)
    else:
        info = DR.readHyperDataInfos(args.source_path, args.max_time, ratio)
    shutil.copyfile(info.ply_path, os.path.join(args.model_path, "input.ply"))
    with open(os.path.join(args.model_path, "cameras.json"), "w") as fp:
        json.dump([camera_to_JSON(k, c) for k, c in enumerate(info.test_cameras + info.train_cameras)], fp)
    train, test, view = (load_cameras(cams, 1.0, args, DEV, decode) for cams in (info.train_cameras, info.test_cameras, info.render_cameras))
    return SimpleNamespace(getTrainCameras=lambda: train, getTestCameras=lambda: test, render_cameras=view)


def measure(lines, label, root, nbytes, ratio=0.5):
    args = SimpleNamespace(source_path=root, model_path=os.path.join(root, "out"), images=None, eval=True, white_background=True, max_time=1.0,
                           resolution=-1, data_device="cuda")
    os.makedirs(args.model_path, exist_ok=True)
    passes = [0]
    once = decode_stage.once

    def counted(*a, **k):
        passes[0] += 1
        return once(*a, **k)

    rows = {}
    decode_stage.once = counted
    try:
        for name, make in (("Scene: device decoders, one pass", lambda: Scene(args, NoModel(), shuffle=False, ratio=ratio, device=DEV)),
                           ("device decoders, list by list", lambda: list_by_list(args, ratio, None)),
                           ("Pillow on the host, list by list", lambda: list_by_list(args, ratio, pillow_decode))):
            passes[0] = 0
            rows[name] = timed(make) + (passes[0] / 3,)
    finally:
        decode_stage.once = once
    (_, d_best, on_device, _), _, (_, h_best, on_host, _) = rows.values()
    pairs = list(zip(on_device.getTrainCameras() + on_device.getTestCameras(), on_host.getTrainCameras() + on_host.getTestCameras()))
    same = all(torch.equal(a.original_image, b.original_image) for a, b in pairs)
    h, w = pairs[0][0].original_image.shape[1:]
    lines.append(f"{label}: {len(pairs)} images of {w} x {h} in the train and test lists, the test list once more as the render list "
                 f"({nbytes / 1e6:.0f} MB of PNG files in the folder)")
    for name, (first, best, _, reads) in rows.items():
        lines.append(f"  {name:34s} first {first * 1e3:9.1f} ms   best of 2 more {best * 1e3:9.1f} ms   {reads:4.1f} device reads")
    lines.append(f"  Pillow list by list / Scene (best) {h_best / d_best:5.2f} x    images equal bit for bit: {same}")


def main():
    lines = [f"Scene(...) on {torch.cuda.get_device_name(DEV)}, {os.cpu_count()} host CPUs visible; wall time, readers and cameras.json included, model creation left out"]
    for label, build in (("D-NeRF-sized", dnerf_folder), ("HyperNeRF-sized", hyper_folder)):
        root = tempfile.mkdtemp(prefix="scene_probe_")
        try:
            nbytes = build(root)
            measure(lines, label, root, nbytes)
        finally:
            shutil.rmtree(root, ignore_errors=True)
        print("\n".join(lines[-5:]), flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "scene_probe.txt"), "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
