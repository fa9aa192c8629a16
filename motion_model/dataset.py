"""Import-name shim: `from motion_model.dataset import GCN3DDataset` [REF train_GCN.py:14] resolves to
`gaussianprediction_amd.motion.GCN3DDataset`: the reference's constructor arguments, `nodes_num`, train / test windows and item keys,
with the keypoint trajectories taken from the K-row MLP pass alone (GaussianModel.keypoint_motion).

Not provided: the abstract GCNBaseDataset and the `val` split (nothing reads it)."""
from gaussianprediction_amd.motion import GCN3DDataset, keypoint_trajectories  # noqa: F401
