"""GPU: batched furthest-point sampling (gp_furthest_point_sampling_batched) and the pointops / simple_knn / tinycudann shims against
the library entry points they wrap."""
import math

import numpy as np
import pytest
import torch

from host_checkers import fps_host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _single(xyz, m):
    from gaussianprediction_amd import _lib
    import ctypes as C
    idx = torch.empty(m, dtype=torch.int32, device=DEV)
    tmp = torch.empty(xyz.shape[0], device=DEV)
    _lib.check(_lib.lib().gp_furthest_point_sampling(C.c_int64(xyz.shape[0]), _lib.ptr(xyz), C.c_int64(m), _lib.ptr(idx), _lib.ptr(tmp),
                                                      _lib.stream_ptr(xyz.device)), "gp_furthest_point_sampling")
    return idx


def test_one_batch_is_the_single_batch_kernel():
    from gaussianprediction_amd.knn_ops import furthest_point_sampling_batched
    rng = np.random.default_rng(0)
    xyz = torch.tensor(rng.normal(size=(30_000, 3)).astype(np.float32), device=DEV)
    xyz[100] = xyz[7]                                           # duplicates: the tie rule decides
    got = furthest_point_sampling_batched(xyz, torch.tensor([30_000], dtype=torch.int32), torch.tensor([300], dtype=torch.int32))
    assert torch.equal(got, _single(xyz, 300))
    assert torch.equal(got.cpu().to(torch.int64), fps_host(xyz, 300))


def test_ragged_batches_equal_single_calls():
    import pointops_cuda
    rng = np.random.default_rng(1)
    n_b, m_b = [5000, 700, 12_000], [50, 7, 120]
    xyz = torch.tensor(rng.normal(size=(sum(n_b), 3)).astype(np.float32), device=DEV)
    off = torch.tensor(np.cumsum(n_b), dtype=torch.int32, device=DEV)
    noff = torch.tensor(np.cumsum(m_b), dtype=torch.int32, device=DEV)
    idx = torch.zeros(sum(m_b), dtype=torch.int32, device=DEV)
    tmp = torch.full((sum(n_b),), 1e10, device=DEV)
    pointops_cuda.furthestsampling_cuda(3, max(n_b), xyz, off, noff, tmp, idx)     # (the reference's call, utils/fps.py:84)
    s0 = q0 = 0
    for nb, mb in zip(n_b, m_b):
        part = xyz[s0:s0 + nb].contiguous()
        want = _single(part, mb) + s0
        assert torch.equal(idx[q0:q0 + mb], want)
        assert torch.equal(idx[q0:q0 + mb].cpu().to(torch.int64), fps_host(part, mb) + s0)
        s0, q0 = s0 + nb, q0 + mb


def test_dist_cuda2_shim():
    from simple_knn._C import distCUDA2
    from gaussianprediction_amd.weights_ops import dist_cuda2
    rng = np.random.default_rng(2)
    p = torch.tensor(rng.normal(size=(5000, 3)).astype(np.float32), device=DEV)
    assert torch.equal(distCUDA2(p), dist_cuda2(p))


def test_tinycudann_shim_is_the_weights_model():
    import tinycudann as tcnn
    from gaussianprediction_amd.weights_ops import WeightsModel
    b = math.exp(math.log(2048 / 16) / 15)
    net = tcnn.NetworkWithInputEncoding(
        n_input_dims=3, n_output_dims=12,
        encoding_config={"otype": "Grid", "type": "Hash", "n_levels": 16, "n_features_per_level": 4, "log2_hashmap_size": 19,
                         "base_resolution": 16, "per_level_scale": b, "interpolation": "Linear"},
        network_config={"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2})
    ref = WeightsModel(12, seed=1337)
    assert isinstance(net, WeightsModel)
    assert torch.equal(net.params, ref.params)
    x = torch.rand(4096, 3, device=DEV) * 2 - 1
    out, want = net(x), ref(x)
    assert torch.equal(out, want)
    out.square().sum().backward()
    want.square().sum().backward()
    # (the table gradient is accumulated with float atomics: the same kernels give the same sum only up to the order of the adds)
    err = (net.params.grad - ref.params.grad).abs().max() / ref.params.grad.abs().max()
    assert err < 1e-5, err
    assert len(list(net.parameters())) == 1
