"""`scene.cameras` of the reference: Camera is gaussianprediction_amd.scene.SceneCamera."""
from gaussianprediction_amd.scene import MiniCam, SceneCamera as Camera  # noqa: F401
