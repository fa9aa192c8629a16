"""What tests/test_scene_host.py and tests/test_gpu_scene.py share: the datasets of tests/golden/scenes/, the record
tests/golden/make_scene_vectors.py took of the reference's readers on them (scenes.npz, scenes.json), copies of a dataset in the state
a test wants, and the comparison of a camera list with the record."""
import json
import os
import shutil
from types import SimpleNamespace

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = os.path.join(GOLDEN, "scenes")
ATOL = 1e-9     # float64 formulas on values of order 1 through one 4x4 inverse: rounding is ~1e-13; the margin is for another LAPACK
_record = None


def record():
    """(arrays of scenes.npz as a dict, the table of scenes.json), loaded once."""
    global _record
    if _record is None:
        with np.load(os.path.join(GOLDEN, "scenes.npz")) as z:
            arrays = {k: z[k] for k in z.files}
        with open(os.path.join(GOLDEN, "scenes.json")) as fp:
            _record = (arrays, json.load(fp))
    return _record


def copy_scene(name, tmp_path, val_ids=False, text=False):
    """A writable copy of tests/golden/scenes/<name>.  val_ids: the HyperNeRF dataset.json variant with val_ids.  text: the COLMAP
    model as text in sparse/0, the binary files gone."""
    dst = os.path.join(str(tmp_path), name)
    shutil.copytree(os.path.join(SCENES, name), dst)
    if val_ids:
        shutil.copyfile(os.path.join(dst, "dataset_val.json"), os.path.join(dst, "dataset.json"))
    if text:
        shutil.rmtree(os.path.join(dst, "sparse/0"))
        shutil.copytree(os.path.join(dst, "sparse_txt/0"), os.path.join(dst, "sparse/0"))
    return dst


def scene_args(source, model, **kw):
    os.makedirs(model, exist_ok=True)
    base = dict(source_path=source, model_path=str(model), images=None, eval=True, white_background=False, max_time=1.0, resolution=-1,
                data_device="cuda")
    base.update(kw)
    return SimpleNamespace(**base)


def check_split(cams, tag, split):
    """A list of CameraInfo against the record: names, uids and sizes exactly, R, T, FoVs and times within ATOL."""
    arrays, table = record()
    rec = table[tag]["splits"][split]
    assert [c.image_name for c in cams] == rec["image_name"], (tag, split)
    assert [int(c.uid) for c in cams] == rec["uid"] and [c.width for c in cams] == rec["width"] and [c.height for c in cams] == rec["height"]
    for k, c in enumerate(cams):
        for field, got in (("R", c.R), ("T", c.T), ("FovX", c.FovX), ("FovY", c.FovY), ("time", np.asarray(c.time).reshape(-1)[0])):
            err = np.abs(np.asarray(got, dtype=np.float64) - arrays[f"{tag}/{split}/{field}"][k]).max()
            assert err <= ATOL, (tag, split, k, field, err)


def check_info(info, tag):
    arrays, table = record()
    for split in ("train", "test", "render"):
        check_split(getattr(info, f"{split}_cameras"), tag, split)
    assert info.total_frame == table[tag]["total_frame"]
    assert np.abs(info.nerf_normalization["translate"] - arrays[f"{tag}/translate"]).max() <= ATOL
    assert abs(info.nerf_normalization["radius"] - arrays[f"{tag}/radius"]) <= ATOL


def check_cameras_json(entries, tag):
    want = record()[1][tag]["cameras_json"]
    assert len(entries) == len(want)
    for got, ref in zip(entries, want):
        assert set(got) == set(ref) and all(got[k] == ref[k] for k in ("id", "img_name", "width", "height"))
        for k in ("position", "rotation", "fx", "fy"):
            assert np.abs(np.asarray(got[k], dtype=np.float64) - np.asarray(ref[k], dtype=np.float64)).max() <= ATOL, (tag, got["id"], k)
