"""Voxel-grid downsampling on the device (include/gp_voxel.h, voxel_ops) against the numpy restatement tests/voxel_ref.py, bit for
bit: every size at which the sort or the scan takes another path, with and without colours and normals; points exactly on voxel
boundaries, negative coordinates, duplicates; one voxel holding every point, every point in its own voxel, keys of one, two and three
sorts; the reference's loop; determinism, the voxel indices, the PLY tool against the host path's file; the refusals.  There are no
tolerances.  A test that ends in a device error is the last one of this module to launch anything."""
import contextlib

import numpy as np
import pytest
import torch

import voxel_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_DEVICE_ERROR = []
_WANT = {}


@pytest.fixture(autouse=True)
def _nothing_is_launched_after_a_device_error():
    if _DEVICE_ERROR:
        pytest.fail(f"not run: an earlier test of this module ended in a device error ({_DEVICE_ERROR[0]})")
    yield


@contextlib.contextmanager
def device_work():
    """Everything that launches runs inside: the device has finished when the block ends, and an error that is not a failed
    comparison keeps the rest of the module from launching."""
    try:
        yield
        torch.cuda.synchronize()
    except AssertionError:
        raise
    except Exception as e:
        _DEVICE_ERROR.append(f"{type(e).__name__}: {e}")
        raise


@pytest.fixture(scope="module")
def V():
    from gaussianprediction_amd import voxel_ops
    return voxel_ops


def same(a, b):
    """Bit-equal arrays (or both None): the bytes."""
    if a is None or b is None:
        return a is None and b is None
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def to_device(*arrays, dtype=None):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype=dtype) for a in arrays)


def want_of(key, points, voxel_size, colors, normals):
    """The restatement's answer, computed once per case and never written to."""
    if key not in _WANT:
        _WANT[key] = ref.down_sample(points, voxel_size, colors, normals)
        for a in _WANT[key]:
            if a is not None:
                a.setflags(write=False)
    return _WANT[key]


def check(V, key, points, voxel_size, colors, normals, dtype=None):
    want = want_of(key, points, voxel_size, colors, normals)
    with device_work():
        pts, col, nrm = to_device(points, colors, normals, dtype=dtype)
        got = V.voxel_down_sample(pts, voxel_size, col, nrm, return_index=True)
    assert len(got) == 4 and tuple(got[0].shape) == want[0].shape, (tuple(got[0].shape), want[0].shape)
    assert got[3].dtype == torch.int32 and same(got[3], want[3])
    for g, w in zip(got[:3], want[:3]):
        assert (g is None or g.dtype == torch.float64) and same(g, w)
    return got, want


@pytest.mark.parametrize("attrs", ref.ATTRS)
@pytest.mark.parametrize("n", ref.SIZES)
def test_every_size_regime_equals_the_restatement(V, n, attrs):
    pts, col, nrm, vs = ref.size_case(n, attrs)
    _, want = check(V, ("size", n, attrs), pts, vs, col, nrm)
    assert n < 1000 or 1 < len(want[0]) < n


def test_float32_input_widens_exactly(V):
    pts, col, nrm, vs = ref.size_case(5000, "xyz+colors+normals")            # (the points are float32 values already)
    nrm = nrm.astype(np.float32).astype(np.float64)
    col = col.astype(np.float32).astype(np.float64)
    check(V, ("f32", 5000), pts, vs, col, nrm, dtype=torch.float32)


@pytest.mark.parametrize("name", list(ref.special_cases()))
def test_boundaries_and_degenerate_clouds(V, name):
    pts, col, nrm, vs = ref.special_cases()[name]
    from gaussianprediction_amd import _lib
    _lib.profile_enable(2)
    try:
        _, want = check(V, ("special", name), pts, vs, col, nrm)
        launches = {k: v[0] for k, v in _lib.profile_collect().items()}
    finally:
        _lib.profile_enable(0)
    m, top = len(want[0]), want[3].max(axis=0)
    assert {"one_voxel": m == 1 and len(pts) == 5000, "own_voxel": m == len(pts), "wide_x": top[0] > 65535 and 255 < top[1] < 65536,
            "wide_xyz": (top > 65535).all(), "wide_far": (top > 2 ** 22).all()}.get(name, True)
    sorts = {"wide_xyz": 2, "wide_far": 3}.get(name, 1)                   # the key's chunks of at most 32 bits
    assert launches == {"voxel_bounds": 1, "voxel_index": 1, "voxel_sort": sorts, "voxel_heads_scan": 1, "voxel_mean": 1}


def test_the_loop_takes_the_eleven_passes(V):
    pts = ref.loop_cloud()
    want_cloud, want_passes = ref.until(pts, max_points=500)
    assert [c for _, c in want_passes] == ref.LOOP_COUNTS
    with device_work():
        cloud, passes = V.downsample_until(to_device(pts, dtype=torch.float32)[0], max_points=500)
    assert passes == want_passes and passes[4][0] == 0.060000000000000005
    assert same(cloud[0], want_cloud[0]) and cloud[0].shape[0] == 451 and cloud[1] is None and cloud[2] is None
    with device_work():
        small, none = V.downsample_until(to_device(pts[:400])[0], max_points=500)
    assert none == [] and same(small[0], pts[:400])


def test_the_loop_carries_colours_and_normals_unquantised(V):
    pts, col, nrm = ref.surface(3000, 21, "xyz+colors+normals")
    want_cloud, want_passes = ref.until(pts, col, nrm, max_points=1000, voxel_size=0.03, step=0.02)
    with device_work():
        cloud, passes = V.downsample_until(*to_device(pts, col, nrm), max_points=1000, voxel_size=0.03, step=0.02)
    assert passes == want_passes and len(passes) > 1
    assert all(same(g, w) for g, w in zip(cloud, want_cloud))


def test_two_calls_are_bit_identical_and_the_index_is_optional(V):
    pts, col, nrm, vs = ref.size_case(70001, "xyz+colors+normals")
    with device_work():
        dev = to_device(pts, col, nrm)
        a = V.voxel_down_sample(dev[0], vs, dev[1], dev[2], return_index=True)
        b = V.voxel_down_sample(dev[0], vs, dev[1], dev[2], return_index=True)
        c = V.voxel_down_sample(dev[0], vs, dev[1], dev[2])
        d = V.voxel_down_sample(dev[0], vs, normals=dev[2])
    assert all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y) for x, y in zip(a, b))
    assert len(c) == 3 and all(same(x, y.cpu().numpy()) for x, y in zip(c, a[:3]))
    assert d[1] is None and same(d[0], a[0].cpu().numpy()) and same(d[2], a[2].cpu().numpy())
    want = want_of(("size", 70001, "xyz+colors+normals"), pts, vs, col, nrm)
    assert same(a[3], want[3]) and same(a[0], want[0])


def test_empty_cloud(V):
    with device_work():
        e = torch.empty(0, 3, dtype=torch.float32, device=DEV)
        out = V.voxel_down_sample(e, 0.02, colors=e, return_index=True)
    assert [None if t is None else (tuple(t.shape), t.dtype) for t in out] == [((0, 3), torch.float64), ((0, 3), torch.float64), None, ((0, 3), torch.int32)]


def test_downsample_ply_equals_the_host_paths_file(V, tmp_path):
    from gaussianprediction_amd import io_formats
    pts, col, nrm = ref.surface(4000, 33, "xyz+colors+normals")
    src, dev_out, host_out = tmp_path / "points3D.ply", tmp_path / "device" / "points3D_downsample.ply", tmp_path / "host.ply"
    io_formats.save_point_cloud_ply(src, pts, col, nrm)
    with device_work():
        passes = V.downsample_ply(src, dev_out, device=DEV, max_points=700)
    cloud, host_passes = V._loop(lambda *a: V.host_pass(*a), V.read_point_cloud_ply(src), 700, 0.02, 0.01)
    io_formats.save_point_cloud_ply(host_out, *cloud)
    assert passes == host_passes and len(passes) > 2 and passes[-1][1] <= 700
    assert open(dev_out, "rb").read() == open(host_out, "rb").read()
    v = io_formats.read_ply_vertices(dev_out)
    assert list(v.dtype.names) == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"] and len(v) == passes[-1][1]


def test_refusals_raise_and_nothing_is_launched_past_the_bounds_pass(V):
    from gaussianprediction_amd import _lib
    pts = ref.surface(3000, 5)[0]
    for bad in (float("nan"), float("inf")):
        p = pts.copy()
        p[2999, 2] = bad
        _lib.profile_enable(2)
        try:
            with device_work():
                dev = to_device(p)[0]
                with pytest.raises(RuntimeError, match="not finite"):
                    V.voxel_down_sample(dev, 0.02)
            launches = {k: v[0] for k, v in _lib.profile_collect().items()}
        finally:
            _lib.profile_enable(0)
        assert launches == {"voxel_bounds": 1}
    with device_work():
        far = to_device(np.array([[0.0, 0.0, 0.0], [1.0, 3.0e6, 0.0]]))[0]
        with pytest.raises(RuntimeError, match="voxel_size is too small"):
            V.voxel_down_sample(far, 1e-3)
        assert V.voxel_down_sample(far, 2e-3)[0].shape[0] == 2
        with pytest.raises(RuntimeError, match="<= 0"):
            V.voxel_down_sample(far, 0.0)
        with pytest.raises(RuntimeError, match=r"colors must be \[2, 3\]"):
            V.voxel_down_sample(far, 0.02, colors=torch.zeros(3, 3, device=DEV))
