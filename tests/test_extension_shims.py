"""CPU: the reference's CUDA-extension imports (simple_knn._C, tinycudann, pytorch3d.ops, pytorch3d.transforms, frnn, pointops_cuda)
resolve to this repository's shims, and every call the reference makes into them (tests/golden/extension_surface.json, recorded by
tests/golden/make_extension_surface.py) binds to the shim's signature."""
import importlib
import inspect
import json
import math
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SURFACE = json.load(open(os.path.join(HERE, "golden", "extension_surface.json")))
MODULES = ["simple_knn._C", "tinycudann", "pytorch3d.ops", "pytorch3d.transforms", "frnn", "pointops_cuda"]
# pointops entry points behind utils/fps.py's Grouping / Subtraction / Aggregation / Interpolation wrappers, which nothing in the
# reference calls: deliberately not provided (a call fails loudly with AttributeError)
NOT_PROVIDED = {"pointops_cuda." + n for n in ("grouping_forward_cuda", "grouping_backward_cuda", "subtraction_forward_cuda",
                                                "subtraction_backward_cuda", "aggregation_forward_cuda", "aggregation_backward_cuda",
                                                "interpolation_forward_cuda", "interpolation_backward_cuda")}
# what each shim returns when the call site unpacks it
RETURN_ARITY = {"frnn.frnn_grid_points": 4, "pytorch3d.ops.knn_points": 3}


def _resolve(dotted):
    mod, name = dotted.rsplit(".", 1)
    return getattr(importlib.import_module(mod), name)


@pytest.mark.parametrize("name", MODULES)
def test_module_resolves_to_this_repository(name):
    m = importlib.import_module(name)
    assert os.path.realpath(m.__file__).startswith(os.path.realpath(ROOT) + os.sep), m.__file__
    assert "unpinned" in (m.__doc__ or ""), f"{name}: the docstring must state that parity is unpinned"


def test_shims_do_not_load_the_library_at_import():
    src = {n: inspect.getsource(importlib.import_module(n)) for n in MODULES}
    for n, text in src.items():
        top = [l for l in text.splitlines() if l.startswith(("import ", "from "))]
        assert not any("gaussianprediction_amd" in l for l in top), (n, top)


def test_every_recorded_import_exists():
    assert {i["import"].split(".")[0] for i in SURFACE["imports"]} >= {"simple_knn", "tinycudann", "pytorch3d", "frnn", "pointops_cuda"}
    for imp in SURFACE["imports"]:
        dotted = imp["import"]
        if dotted in MODULES:
            importlib.import_module(dotted)
        else:
            assert callable(_resolve(dotted)), imp


def test_every_recorded_call_binds():
    seen = set()
    for call in SURFACE["calls"]:
        callee = call["callee"]
        if callee in NOT_PROVIDED:
            mod, name = callee.rsplit(".", 1)
            assert not hasattr(importlib.import_module(mod), name), callee
            continue
        fn = _resolve(callee)
        sig = inspect.signature(fn)
        sig.bind(*range(call["positional"]), **{k: None for k in call["keywords"]})
        if call["unpacked"] is not None:
            assert RETURN_ARITY[callee] == call["unpacked"], call
        seen.add(callee)
    assert seen == {"frnn.frnn_grid_points", "pytorch3d.ops.knn_points", "simple_knn._C.distCUDA2", "tinycudann.NetworkWithInputEncoding",
                    "pointops_cuda.furthestsampling_cuda", "pointops_cuda.knnquery_cuda", "pytorch3d.transforms.matrix_to_quaternion",
                    "pytorch3d.transforms.quaternion_to_matrix"}, seen


def test_return_arity_of_the_tuple_shims():
    from pytorch3d.ops import _KNN
    assert len(_KNN._fields) == 3 and _KNN._fields == ("dists", "idx", "knn")
    src = inspect.getsource(importlib.import_module("frnn").frnn_grid_points)
    assert "return dists, idxs, nn, grid" in src


def _reference_configs():
    enc = {"otype": "Grid", "type": "Hash", "n_levels": 16, "n_features_per_level": 4, "log2_hashmap_size": 19, "base_resolution": 16,
           "per_level_scale": math.exp(math.log(2048 / 16) / 15), "interpolation": "Linear"}
    net = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
    return enc, net


@pytest.mark.parametrize("section,key,value", [
    ("enc", "n_levels", 8), ("enc", "n_features_per_level", 2), ("enc", "otype", "Frequency"), ("enc", "interpolation", "Smoothstep"),
    ("enc", "hash", "CoherentPrime"), ("net", "n_neurons", 128), ("net", "n_hidden_layers", 3), ("net", "activation", "Sigmoid"),
    ("net", "output_activation", "Sigmoid"), ("net", "otype", "CutlassMLP"), ("net", "feedback_alignment", True)])
def test_tinycudann_refuses_other_configurations(section, key, value):
    import tinycudann as tcnn
    enc, net = _reference_configs()
    (enc if section == "enc" else net)[key] = value
    with pytest.raises(ValueError, match=repr(key)):
        tcnn.NetworkWithInputEncoding(n_input_dims=3, n_output_dims=12, encoding_config=enc, network_config=net)


def test_tinycudann_refuses_other_sizes():
    import tinycudann as tcnn
    enc, net = _reference_configs()
    with pytest.raises(ValueError, match="n_output_dims"):
        tcnn.NetworkWithInputEncoding(n_input_dims=3, n_output_dims=17, encoding_config=enc, network_config=net)
    with pytest.raises(ValueError, match="n_input_dims"):
        tcnn.NetworkWithInputEncoding(n_input_dims=4, n_output_dims=12, encoding_config=enc, network_config=net)


def test_transforms_round_trip_on_cpu():
    from pytorch3d.transforms import matrix_to_quaternion, quaternion_to_matrix
    g = torch.Generator().manual_seed(0)
    q = torch.randn(512, 4, generator=g, dtype=torch.float64)
    q = q / q.norm(dim=-1, keepdim=True)
    q = torch.where(q[:, :1] < 0, -q, q)
    R = quaternion_to_matrix(q)
    assert R.device.type == "cpu" and R.dtype == torch.float64 and R.shape == (512, 3, 3)
    assert torch.allclose(R @ R.transpose(-1, -2), torch.eye(3, dtype=torch.float64).expand(512, 3, 3), atol=1e-12)
    assert torch.allclose(torch.linalg.det(R), torch.ones(512, dtype=torch.float64), atol=1e-12)
    assert torch.allclose(matrix_to_quaternion(R), q, atol=1e-12)
    # the reference's call shape: a single numpy rotation through torch.from_numpy, then [None] and squeeze
    import numpy as np
    Rn = quaternion_to_matrix(torch.tensor([0.9, 0.1, -0.3, 0.2], dtype=torch.float64)).numpy()
    qn = matrix_to_quaternion(torch.from_numpy(Rn))
    assert qn.shape == (4,)
    assert np.allclose(quaternion_to_matrix(qn[None]).squeeze().numpy(), Rn, atol=1e-12)
    # half-turns (w = 0): every closed form but one divides by ~0
    for axis in torch.eye(3, dtype=torch.float64):
        qa = torch.cat([torch.zeros(1, dtype=torch.float64), axis])
        assert torch.allclose(quaternion_to_matrix(matrix_to_quaternion(quaternion_to_matrix(qa))), quaternion_to_matrix(qa), atol=1e-12)
