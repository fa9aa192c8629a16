"""`scene.dataset_readers` of the reference, from gaussianprediction_amd.dataset_readers."""
from gaussianprediction_amd.dataset_readers import (BasicPointCloud, CameraInfo, SceneInfo, getNerfppNorm, readColmapSceneInfo,  # noqa: F401
                                                    readHyperDataInfos, readNerfSyntheticInfo, sceneLoadTypeCallbacks)
from gaussianprediction_amd.dataset_readers import fetch_ply as fetchPly, store_ply as storePly  # noqa: F401
