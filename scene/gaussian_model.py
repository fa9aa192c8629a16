"""`scene.gaussian_model` of the reference."""
from gaussianprediction_amd.dataset_readers import BasicPointCloud  # noqa: F401
from gaussianprediction_amd.gaussian_model import GaussianModel  # noqa: F401
