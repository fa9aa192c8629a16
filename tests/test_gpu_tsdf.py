"""TSDF fusion and mesh extraction on the device against the numpy restatement tests/tsdf_ref.py on every case of tests/tsdf_cases.py:
bit for bit for tsdf, weight, color, counts, vertices, colors and faces; every entry twice with equal bytes; 16 views in one call
against 16 calls of one view; the facts of closed surfaces on the device's own output; a sphere of Gaussians fused from seven cameras
and written by render_meshes; the refusals.

Measured on an MI355X: see DESIGN section 26."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tsdf_cases as cases
import tsdf_ref as ref
from test_tsdf_host import check_closed_surface

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = np.float32
IT = 50000


def same(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_volume(vol):
    """A TsdfVolume holding a tsdf_ref volume's arrays."""
    from gaussianprediction_amd import tsdf_ops as TO
    v = TO.TsdfVolume(vol.origin, vol.voxel, (vol.nx, vol.ny, vol.nz), trunc=vol.trunc, color=vol.color is not None, device=DEV)
    v.tsdf.copy_(dev(vol.tsdf).view_as(v.tsdf))
    v.weight.copy_(dev(vol.weight).view_as(v.weight))
    if vol.color is not None:
        v.color.copy_(dev(vol.color).view_as(v.color))
    return v


def device_views(views):
    from gaussianprediction_amd import tsdf_ops as TO
    return [TO.View(dev(np.asarray(v.vm, F).reshape(4, 4)), v.tanfovx, v.tanfovy) for v in views]


def volume_equals(v, want):
    t, w, c = want
    return same(v.tsdf.reshape(-1), t) and same(v.weight.reshape(-1), w) and ((v.color is None and c is None) or same(v.color.reshape(3, -1), c))


# ---- every case against the restatement, and twice ----
@pytest.mark.parametrize("name", list(cases.EXTRACT))
def test_extraction_equals_the_restatement_and_itself(name):
    from gaussianprediction_amd import tsdf_ops as TO
    vol, iso, min_weight = cases.EXTRACT[name]
    counts, vertices, colors, faces = cases.extracted(name)
    v = device_volume(vol)
    mesh = v.extract(iso, min_weight)
    assert isinstance(mesh, TO.Mesh) and mesh.vertices.dtype == torch.float32 and mesh.faces.dtype == torch.int32
    assert tuple(mesh.vertices.shape) == (int(counts[0]), 3) and tuple(mesh.faces.shape) == (int(counts[1]), 3)
    assert same(mesh.vertices, vertices) and same(mesh.faces, faces)
    assert (mesh.colors is None and colors is None) or same(mesh.colors, colors)
    again = v.extract(iso, min_weight)
    assert torch.equal(again.vertices.view(torch.int32), mesh.vertices.view(torch.int32)) and torch.equal(again.faces, mesh.faces)
    assert same(v.tsdf.reshape(-1), vol.tsdf) and same(v.weight.reshape(-1), vol.weight)         # the volume is read only


@pytest.mark.parametrize("name", list(cases.INTEGRATE))
def test_integration_equals_the_restatement_and_itself(name):
    c, want = cases.INTEGRATE[name], cases.integrated(name)
    views = device_views(c.views)
    depth, valid, image = dev(c.depth), dev(c.valid), dev(c.image)
    kw = dict(image=image, weight=c.view_weight, weight_max=c.weight_max, z_min=c.z_min)
    v = device_volume(c.vol)
    assert v.integrate(depth, valid, views, **kw) is v          # (a 17-view list goes as 16 + 1)
    assert volume_equals(v, want), name
    twice = device_volume(c.vol).integrate(depth, None if valid is None else valid != 0, views, **kw)
    assert torch.equal(twice.tsdf.view(torch.int32), v.tsdf.view(torch.int32)) and torch.equal(twice.weight.view(torch.int32), v.weight.view(torch.int32))
    one = device_volume(c.vol)                                   # V views in one call equal V calls of one view, byte for byte
    for k in range(len(views)):
        one.integrate(depth[k], None if valid is None else valid[k], views[k], image=None if image is None else image[k], weight=c.view_weight,
                      weight_max=c.weight_max, z_min=c.z_min)
    assert volume_equals(one, want), name
    v.reset()
    assert not v.tsdf.any() and not v.weight.any() and (v.color is None or not v.color.any())


@pytest.mark.parametrize("name, euler", [("33_sphere", 2), ("33_ellipsoid", 2), ("33_torus", 0)])
def test_closed_surfaces_on_the_device(name, euler):
    vol, iso, min_weight = cases.EXTRACT[name]
    mesh = device_volume(vol).extract(iso, min_weight)
    vertices, faces = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    check_closed_surface(vertices, faces, euler)
    if name == "33_sphere":
        s = cases.SPHERE
        dist = np.abs(np.linalg.norm(vertices.astype(np.float64) - np.array(s.c), axis=1) - s.r)
        assert dist.max() <= np.sqrt(3) * vol.voxel


def test_integrate_then_extract_a_plane_on_the_device():
    from gaussianprediction_amd import tsdf_ops as TO
    d = float(F(1.53))
    v = TO.TsdfVolume((-0.25, -0.25, 1.0), 0.0625, (9, 9, 17), trunc=0.25, device=DEV)
    view = device_views([cases.plain_view(0.0, 0.5, 0.5)])[0]
    v.integrate(torch.full((32, 32), d, device=DEV), None, view, image=torch.full((3, 32, 32), 0.5, device=DEV))
    mesh = v.extract()
    assert mesh.vertices.shape[0] > 100 and float((mesh.vertices[:, 2].double() - d).abs().max()) <= 2 * 2.0 ** -24       # test_tsdf_host.py's bound
    assert float((mesh.colors - 0.5).abs().max()) == 0.0
    vol = ref.volume(9, 9, 17, (-0.25, -0.25, 1.0), 0.0625, 0.25)
    vol.tsdf, vol.weight, vol.color = ref.integrate(vol, np.full((1, 32, 32), d, F), None, np.full((1, 3, 32, 32), 0.5, F), [cases.plain_view(0.0, 0.5, 0.5)])
    want = ref.extract(vol)
    assert same(mesh.vertices, want[1]) and same(mesh.faces, want[3]) and same(mesh.colors, want[2])


# ---- the refusals ----
def test_the_device_refusals():
    from gaussianprediction_amd import _lib, tsdf_ops as TO
    v = TO.TsdfVolume((0, 0, 0), 0.1, (5, 4, 3), device=DEV)
    plain = TO.TsdfVolume((0, 0, 0), 0.1, (5, 4, 3), color=False, device=DEV)
    view = device_views([cases.plain_view(0.0, 0.5, 0.5)])[0]
    depth, image = torch.ones(12, 16, device=DEV), torch.zeros(3, 12, 16, device=DEV)
    nan, inf = float("nan"), float("inf")
    before = [t.clone() for t in (v.tsdf, v.weight, v.color, plain.tsdf, plain.weight)]
    for call, word in ((lambda: v.integrate(depth, None, view), "go together"), (lambda: plain.integrate(depth, None, view, image=image), "go together"),
                       (lambda: v.integrate(depth, None, [], image=image), "V must be"), (lambda: v.integrate(depth, None, view, image=image, z_min=0.0), "finite and > 0"),
                       (lambda: v.integrate(depth, None, view, image=image, weight=nan), "finite and > 0"), (lambda: v.integrate(depth, None, view, image=image, weight_max=inf), "finite and > 0"),
                       (lambda: v.integrate(depth, None, TO.View(view.world_view, nan, 0.5), image=image), "finite"),
                       (lambda: v.integrate(torch.ones(0, 16, device=DEV), None, view, image=torch.zeros(3, 0, 16, device=DEV)), "H and W"),
                       (lambda: v.extract(iso=nan), "iso"), (lambda: v.extract(iso=inf), "iso"), (lambda: v.extract(min_weight=nan), "NaN")):
        with pytest.raises(_lib.GpHipError, match=word):
            call()
    for call, word in ((lambda: v.integrate(depth.cpu(), None, view, image=image), "no CPU fallback"), (lambda: v.integrate(depth.double(), None, view, image=image), "float32"),
                       (lambda: v.integrate(depth, None, [view, view], image=image), r"\[2, H, W\]"), (lambda: v.integrate(depth, None, view, image=image[:, :11]), "image must be"),
                       (lambda: v.integrate(depth, torch.ones(12, 15, dtype=torch.bool, device=DEV), view, image=image), "bool or uint8"),
                       (lambda: v.integrate(depth, None, TO.View(view.world_view.cpu(), 0.5, 0.5), image=image), "no CPU fallback"),
                       (lambda: v.integrate(depth, None, TO.View(view.world_view[:3], 0.5, 0.5), image=image), r"\[4, 4\]")):
        with pytest.raises(RuntimeError, match=word):
            call()
    after = (v.tsdf, v.weight, v.color, plain.tsdf, plain.weight)
    assert all(torch.equal(a, b) for a, b in zip(before, after))             # nothing was launched
    empty = v.extract()
    assert empty.vertices.shape == (0, 3) and empty.faces.shape == (0, 3) and empty.colors.shape == (0, 3) and plain.extract().colors is None


# ---- end to end: a sphere of Gaussians, seven cameras around it ----
W, H, N, RADIUS, SCALE, SHIFT = 64, 48, 4000, 1.0, 0.05, 0.3
THICKNESS = 3 * SCALE        # the Gaussians are isotropic with standard deviation SCALE: their mass lies within three of it of the sphere
RESOLUTION = 32


@pytest.fixture(scope="module")
def scene():
    """A model whose forward is a stub: N isotropic Gaussians on the sphere of radius RADIUS about (SHIFT * t, 0, 0) (a Fibonacci
    lattice: about 0.056 apart, one standard deviation), nearly opaque."""
    from test_gpu_render import build
    from gaussianprediction_amd.cameras import orbit_cameras
    pc = build(N=N, K=20, W=W, H=H)[0]
    assert pc.get_xyz.shape[0] == N
    k = np.arange(N) + 0.5
    phi, theta = np.arccos(1 - 2 * k / N), np.pi * (1 + 5 ** 0.5) * k
    base = torch.from_numpy((RADIUS * np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], axis=1)).astype(F)).to(DEV)
    rot = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=DEV).repeat(N, 1)
    scales = torch.full((N, 3), SCALE, device=DEV)
    opacity = torch.full((N, 1), 0.95, device=DEV)
    shift = torch.tensor([SHIFT, 0.0, 0.0], device=DEV)

    def forward(t, iteration, *a, raw_activations=False, **kw):
        pc._forward_raw = False
        xyz = base + shift * t.to(DEV, torch.float32).reshape(-1)[:1]
        pc._last_xyz_t = xyz
        return xyz, rot, scales, opacity

    pc.forward = forward
    cams = orbit_cameras(7, 4.0, 0.6911, W, H, device=DEV)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    return SimpleNamespace(pc=pc, cams=cams, pipe=pipe, bg=torch.zeros(3, device=DEV))


def test_fuse_gives_the_sphere(scene):
    from gaussianprediction_amd import tsdf_ops as TO
    for t in (0.0, 0.5):
        mesh = TO.fuse(scene.cams, scene.pc, scene.pipe, IT, time=t, resolution=RESOLUTION)
        voxel = 2 * RADIUS / RESOLUTION              # the bounds are the Gaussians' own, inside the sphere's box: the voxel is at most this
        trunc = 4 * voxel
        nv, nf = mesh.vertices.shape[0], mesh.faces.shape[0]
        centre = torch.tensor([SHIFT * t, 0.0, 0.0], device=DEV)
        dist = ((mesh.vertices - centre).double().norm(dim=1) - RADIUS).abs()
        print("time", t, "vertices", nv, "faces", nf, "largest | |v - c| - r |", float(dist.max()), "mean", float(dist.mean()), "bound", trunc + THICKNESS)
        assert nv > 1000 and nf > 1000 and mesh.colors.shape == (nv, 3) and int(mesh.faces.min()) == 0 and int(mesh.faces.max()) == nv - 1
        assert float(dist.max()) <= trunc + THICKNESS
        assert bool(torch.isfinite(mesh.colors).all()) and float(mesh.colors.std()) > 0.01
        again = TO.fuse([{"cam": c} for c in scene.cams], scene.pc, scene.pipe, IT, time=t, resolution=RESOLUTION)
        assert torch.equal(again.vertices.view(torch.int32), mesh.vertices.view(torch.int32)) and torch.equal(again.faces, mesh.faces)
        assert torch.equal(again.colors.view(torch.int32), mesh.colors.view(torch.int32))
    plain = TO.fuse(scene.cams[:3], scene.pc, scene.pipe, IT, time=0.0, bounds=((-1.3, -1.3, -1.3), (1.3, 1.3, 1.3)), voxel_size=0.1, color=False)
    assert plain.colors is None and plain.vertices.shape[0] > 100


def test_render_meshes_writes_one_ply_per_time(scene, tmp_path):
    from gaussianprediction_amd import eval_render as ER, io_formats, tsdf_ops as TO
    root = str(tmp_path / "scene" / "model")
    out_dir, stats = ER.render_meshes(root, "test", IT, [{"cam": c} for c in scene.cams], scene.pc, scene.pipe, scene.bg, times=[0.25, 0.75], resolution=RESOLUTION)
    top = os.path.dirname(out_dir)
    assert out_dir == os.path.join(root, "eval", "test", f"ours_{IT}", "meshes") and sorted(os.listdir(top)) == ["meshes"]
    assert sorted(os.listdir(out_dir)) == ["00000.ply", "00001.ply"]
    assert stats["frames"] == 2 and stats["seconds"] > 0 and len(stats["vertices"]) == len(stats["faces"]) == 2
    first = [open(os.path.join(out_dir, f), "rb").read() for f in sorted(os.listdir(out_dir))]
    for i, t in enumerate((0.25, 0.75)):
        mesh = TO.fuse(scene.cams, scene.pc, scene.pipe, IT, time=t, resolution=RESOLUTION, background=scene.bg)
        vertices, faces, colors = io_formats.read_mesh_ply(os.path.join(out_dir, f"{i:05d}.ply"))
        assert (stats["vertices"][i], stats["faces"][i]) == (len(vertices), len(faces)) == (mesh.vertices.shape[0], mesh.faces.shape[0])
        assert same(mesh.vertices, vertices) and same(mesh.faces, faces) and same(io_formats.color_to_uint8(mesh.colors.cpu().numpy()), colors)
    out_dir2, _ = ER.render_meshes(str(tmp_path / "again"), "test", IT, scene.cams, scene.pc, scene.pipe, scene.bg, times=[0.25, 0.75], resolution=RESOLUTION)
    assert [open(os.path.join(out_dir2, f), "rb").read() for f in sorted(os.listdir(out_dir2))] == first          # two runs give byte-equal files
    # by default the times are the distinct times of the views, in their order
    out_dir3, stats3 = ER.render_meshes(str(tmp_path / "own"), "own", IT, [scene.cams[0], scene.cams[3], scene.cams[0]], scene.pc, scene.pipe, scene.bg, resolution=16)
    assert sorted(os.listdir(out_dir3)) == ["00000.ply", "00001.ply"] and stats3["frames"] == 2
    assert math.isclose(float(np.asarray(scene.cams[3].time).reshape(-1)[0]), 0.5)
    want = TO.fuse([scene.cams[0], scene.cams[3], scene.cams[0]], scene.pc, scene.pipe, IT, time=0.5, resolution=16, background=scene.bg)
    assert same(want.vertices, io_formats.read_mesh_ply(os.path.join(out_dir3, "00001.ply"))[0])
