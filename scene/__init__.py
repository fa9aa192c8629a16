"""Import-name shim: `from scene import Scene, GaussianModel` [REF train.py:23, eval.py:16] resolves to the MI355X implementation.

Provided: `scene.dataset_readers` (the three readers, sceneLoadTypeCallbacks, CameraInfo, SceneInfo, fetchPly, storePly),
`scene.cameras` (Camera, MiniCam), `scene.gaussian_model` (GaussianModel, BasicPointCloud) and `scene.deformable_field`
(Deformable_Field).  Not provided: scene.colmap_loader, scene.hyper_loader and scene.utils -- the readers are their only callers."""
from gaussianprediction_amd.gaussian_model import GaussianModel  # noqa: F401
from gaussianprediction_amd.scene import Scene  # noqa: F401
