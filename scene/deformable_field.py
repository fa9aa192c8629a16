"""`scene.deformable_field` of the reference."""
from gaussianprediction_amd.deformable_field import Deformable_Field  # noqa: F401
