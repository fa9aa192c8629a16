"""Import-name shim: the reference's `motion_model` package [REF motion_model/gcn.py, motion_model/dataset.py] resolves to
`gaussianprediction_amd.motion` (the GCN keypoint motion predictor on the HIP layer kernels of include/gp_gcn.h).

Provided: `motion_model.gcn` (GraphConvolution, GC_Block, GCN, Channel_GCN, GCN_xyzr, get_dct_matrix) and `motion_model.dataset`
(GCN3DDataset).  Not provided: SemskeConv, _GraphConv, Generator and GCNBaseDataset's `val` split -- no entry point of the reference
reaches them."""
