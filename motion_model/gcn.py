"""Import-name shim: `from motion_model.gcn import GCN_xyzr, get_dct_matrix` [REF train_GCN.py:13] resolves to
`gaussianprediction_amd.motion`.  Constructor signatures, parameter / buffer names and state_dict() keys are the reference's, so its
`ckpt.pth` loads here and one written here loads there; every layer runs on the HIP kernels (no CPU path).

Not provided: SemskeConv, _GraphConv, Generator (unreached by the reference's entry points); p_dropout > 0 raises NotImplementedError."""
from gaussianprediction_amd.motion import GraphConvolution, GC_Block, GCN, Channel_GCN, GCN_xyzr, get_dct_matrix  # noqa: F401
