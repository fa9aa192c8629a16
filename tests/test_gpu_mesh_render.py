"""The triangle rasterizer on the device against the numpy restatement tests/mesh_render_ref.py on every case and cull mode of
tests/mesh_render_cases.py: bit for bit for the counts, the coverage, the face, depth and valid planes and the barycentrics; every
call twice with equal bytes; the inputs unchanged; the facts of closed surfaces on the device's own output; interpolate, normals and
shade bit for bit; render_mesh in its four modes; a sphere of Gaussians through render_mesh_views with the comparison against its
own depth renders.

Measured on an MI355X: see DESIGN section 29."""
import os

import numpy as np
import pytest
import torch

import mesh_render_cases as cases
import mesh_render_ref as ref
import png_cases as P
from test_gpu_tsdf import IT, RESOLUTION, scene  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = np.float32


def same(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    if a.dtype == np.bool_:
        a = a.view(np.uint8)
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def device_case(c):
    from gaussianprediction_amd.tsdf_ops import Mesh, View
    return Mesh(dev(c.vertices), dev(c.faces), None), View(dev(np.asarray(c.view.vm, F).reshape(4, 4)), c.view.tanfovx, c.view.tanfovy), dev(c.attributes)


def planes(r):
    return [r.coverage, r.face, r.depth, r.valid, r.bary]


def stats_of(counts):
    from gaussianprediction_amd import mesh_render as MR
    return dict(zip(MR.STAT_NAMES, (int(v) for v in counts[:7])))


@pytest.mark.parametrize("name, cull", cases.RUNS)
def test_every_case_equals_the_restatement_and_itself(name, cull):
    from gaussianprediction_amd import mesh_render as MR
    c, want = cases.CASES[name], cases.result(name, cull)
    mesh, view, attributes = device_case(c)
    got = MR.rasterize(mesh, view, z_near=c.z_near, cull=cull, counts=True, size=(c.H, c.W))
    print(name, cull, got.stats)
    assert got.stats == stats_of(want.counts)
    assert [t.dtype for t in planes(got)] == [torch.int32, torch.int32, torch.float32, torch.bool, torch.float32] and all(t.is_contiguous() for t in planes(got))
    for k, (g, w) in enumerate(zip(planes(got), cases.planes(want)[1:])):
        assert same(g, w), (name, cull, k)
    again = MR.rasterize(mesh, view, z_near=c.z_near, cull=cull, counts=True, size=(c.H, c.W))          # run to run
    assert again.stats == got.stats and all(bytes_equal(a, b) for a, b in zip(planes(got), planes(again)))
    plain = MR.rasterize(mesh, view, z_near=c.z_near, cull=cull, size=(c.H, c.W))
    assert plain.coverage is None and plain._stats is None and all(bytes_equal(a, b) for a, b in zip(planes(got)[1:], planes(plain)[1:]))
    assert same(mesh.vertices, c.vertices) and same(mesh.faces, c.faces) and same(view.world_view, np.asarray(c.view.vm, F).reshape(4, 4))      # the inputs are read only


@pytest.mark.parametrize("name", cases.CLOSED)
def test_closed_surfaces_on_the_device(name):
    from gaussianprediction_amd import mesh_render as MR
    c = cases.CASES[name]
    mesh, view, _ = device_case(c)
    none, back, front = (MR.rasterize(mesh, view, cull=cull, counts=True, size=(c.H, c.W)) for cull in ("none", "back", "front"))
    values = set(torch.unique(none.coverage).tolist())
    assert all(v % 2 == 0 for v in values) and bool(none.valid.any())
    if not name.startswith("torus"):
        assert values == {0, 2}
    assert bytes_equal(back.depth, none.depth) and bytes_equal(back.valid, none.valid)
    assert bytes_equal(front.valid, none.valid) and bool((front.depth[none.valid] > none.depth[none.valid]).all())
    order = torch.from_numpy(np.random.default_rng(5).permutation(len(c.faces))).to(DEV)
    mixed = MR.rasterize(type(mesh)(mesh.vertices, mesh.faces[order].contiguous(), None), view, counts=True, size=(c.H, c.W))
    assert bytes_equal(mixed.depth, none.depth) and bytes_equal(mixed.coverage, none.coverage) and torch.equal(order[mixed.face[mixed.valid].long()].int(), none.face[none.valid])


@pytest.mark.parametrize("name", cases.PICTURES)
def test_interpolate_normals_and_shade_equal_the_restatement(name):
    from gaussianprediction_amd import mesh_render as MR
    c = cases.CASES[name]
    colour, n, nvalid, shaded = cases.pictures(name)
    mesh, view, attributes = device_case(c)
    r = MR.rasterize(mesh, view, z_near=c.z_near, size=(c.H, c.W))
    got_colour = MR.interpolate(r, attributes, background=cases.BACKGROUND)
    got_n, got_nvalid = MR.normals(r, mesh, view, size=(c.H, c.W))
    got_shaded = MR.shade(got_colour[:3], (got_n, got_nvalid), r, view, ambient=cases.AMBIENT, background=cases.SHADE_BACKGROUND, size=(c.H, c.W))
    assert same(got_colour, colour) and same(got_n, n) and same(got_nvalid, nvalid) and same(got_shaded, shaded)
    assert got_nvalid.dtype == torch.bool and got_colour.shape == (4, c.H, c.W) and int(nvalid.sum()) > 0
    one = MR.interpolate(r, attributes[:, 1:2].contiguous(), background=cases.BACKGROUND[1])
    assert bytes_equal(one[0], got_colour[1])                    # a column alone is that column
    again = MR.shade(got_colour[:3], (got_n, got_nvalid), r, view, ambient=cases.AMBIENT, background=cases.SHADE_BACKGROUND, size=(c.H, c.W))
    assert bytes_equal(again, got_shaded) and same(attributes, c.attributes)
    # the normals face the camera, have unit length, and the shade is between the ambient share and the colour
    length = got_n.double().pow(2).sum(0).sqrt()[got_nvalid]
    assert float((length - 1).abs().max()) < 1e-6
    lit = got_shaded[:, got_nvalid] / got_colour[:3][:, got_nvalid].clamp_min(1e-20)
    assert float(lit.min()) >= cases.AMBIENT - 1e-6 and float(lit.max()) <= 1 + 1e-6


def test_render_mesh_in_its_four_modes():
    from gaussianprediction_amd import depth_ops as DO, mesh_render as MR
    from gaussianprediction_amd.tsdf_ops import Mesh
    c = cases.CASES["sphere_0"]
    mesh, view, attributes = device_case(c)
    coloured = Mesh(mesh.vertices, mesh.faces, attributes[:, :3].contiguous())
    r = MR.rasterize(mesh, view, size=(c.H, c.W))
    bg = (0.25, 0.5, 0.75)
    want_bg = torch.tensor(bg, device=DEV).reshape(3, 1).expand(3, int((~r.valid).sum()))
    for mode in MR.MODES:
        for m in (mesh, coloured):
            image = MR.render_mesh(m, view, mode=mode, background=bg, size=(c.H, c.W))
            assert image.shape == (3, c.H, c.W) and image.dtype == torch.float32 and image.is_contiguous() and bool(torch.isfinite(image).all())
            assert torch.equal(image[:, ~r.valid], want_bg), mode
            assert bytes_equal(image, MR.render_mesh(m, view, mode=mode, background=bg, size=(c.H, c.W), raster=r))
    n = MR.normals(r, mesh, view, size=(c.H, c.W))
    grey = MR.render_mesh(mesh, view, mode="color", size=(c.H, c.W))
    assert float((grey[:, r.valid] - MR.GREY).abs().max()) < 1e-6          # a mesh without colours is grey
    assert bytes_equal(MR.render_mesh(mesh, view, mode="shaded", size=(c.H, c.W)), MR.shade(grey, n, r, view, size=(c.H, c.W)))
    assert bytes_equal(MR.render_mesh(mesh, view, mode="normals", size=(c.H, c.W)), DO.normals_image(*n))
    assert bytes_equal(MR.render_mesh(mesh, view, mode="depth", size=(c.H, c.W), near=3.0, far=5.0, depth_mode="depth"), DO.colorize(r.depth, r.valid, "depth", 3.0, 5.0))
    assert bytes_equal(MR.render_mesh(coloured, view, mode="color", size=(c.H, c.W)), MR.interpolate(r, coloured.colors))


def test_the_device_refusals():
    from gaussianprediction_amd import _lib, mesh_render as MR
    from gaussianprediction_amd.tsdf_ops import Mesh
    c = cases.CASES["diagonal"]
    mesh, view, attributes = device_case(c)
    r = MR.rasterize(mesh, view, size=(c.H, c.W))
    for fn, word in ((lambda: MR.rasterize(mesh, view), "pass size"), (lambda: MR.rasterize(Mesh(mesh.vertices.cpu(), mesh.faces, None), view, size=(8, 8)), "no CPU fallback"),
                     (lambda: MR.rasterize(mesh, type(view)(view.world_view.cpu(), 0.5, 0.5), size=(8, 8)), "no CPU fallback"),
                     (lambda: MR.interpolate(r, attributes.cpu()), "no CPU fallback"), (lambda: MR.interpolate(r, attributes[:2]), "attributes"),
                     (lambda: MR.interpolate(r, attributes, background=(0, 0)), "background"), (lambda: MR.normals(r, mesh, view, size=(8, 8)), "the raster is"),
                     (lambda: MR.shade(torch.zeros(3, 8, 8, device=DEV), torch.zeros(3, c.H, c.W, device=DEV), r, view, size=(c.H, c.W)), "color")):
        with pytest.raises(RuntimeError, match=word):
            fn()
    for fn, word in ((lambda: MR.rasterize(mesh, view, size=(0, 8)), "> 0"), (lambda: MR.rasterize(mesh, view, size=(8, 16385)), "16384"),
                     (lambda: MR.rasterize(mesh, type(view)(view.world_view, float("inf"), 0.5), size=(8, 8)), "finite"),
                     (lambda: MR.interpolate(r, torch.zeros(4, 9, device=DEV)), "C must be 1 .. 8")):
        with pytest.raises(_lib.GpHipError, match=word):
            fn()


def test_render_mesh_views_of_a_sphere_of_gaussians(scene, tmp_path):  # noqa: F811
    from gaussianprediction_amd import depth_ops as DO, eval_render as ER, jpeg_decode, mesh_render as MR, png_decode, tsdf_ops as TO
    import math
    from types import SimpleNamespace
    views = [scene.cams[0], scene.cams[3], scene.cams[0]]
    root = str(tmp_path / "scene" / "model")
    out_dir, stats = ER.render_mesh_views(root, "test", IT, [{"cam": v} for v in views], scene.pc, scene.pipe, scene.bg, compare=True, video=True, resolution=RESOLUTION)
    assert out_dir == os.path.join(root, "eval", "test", f"ours_{IT}", "mesh_views") and sorted(os.listdir(out_dir)) == ["00000.png", "00001.png", "00002.png"]
    assert stats["frames"] == 3 and stats["seconds"] > 0 and len(stats["agreement"]) == 3 and stats["video"] == os.path.join(os.path.dirname(out_dir), "scene_mesh_views.avi")
    assert len(jpeg_decode.avi_frames(open(stats["video"], "rb").read(), "v.avi")[2]) == 3
    meshes = {}
    for i, cam in enumerate(views):
        t = float(np.asarray(cam.time, dtype=F).reshape(-1)[0])
        if t not in meshes:
            meshes[t] = TO.fuse(views, scene.pc, scene.pipe, IT, time=t, resolution=RESOLUTION, background=scene.bg)
        mesh = meshes[t]
        H, W = int(cam.image_height), int(cam.image_width)
        v = SimpleNamespace(vm=cam.world_view_transform.cpu().numpy().reshape(16), tanfovx=math.tan(float(cam.FoVx) * 0.5), tanfovy=math.tan(float(cam.FoVy) * 0.5))
        vertices, faces, colors = (a.cpu().numpy() for a in mesh)
        r = ref.rasterize(vertices, faces, v, W, H)
        colour = ref.interpolate(r, faces, colors, (0, 0, 0))
        n, nvalid = ref.normals(r, vertices, faces, v)
        want = ref.shade(colour, n, nvalid, r.depth, v)
        got = MR.render_mesh(mesh, cam)
        assert same(got, want) and int(nvalid.sum()) > 200                     # the device's picture of the device-fused mesh, bit for bit
        raster = MR.rasterize(mesh, cam)
        assert same(raster.depth, r.depth) and same(raster.face, r.face) and same(raster.bary, r.bary)
        file = png_decode.decode_files([os.path.join(out_dir, f"{i:05d}.png")], device=DEV)[0]
        assert tuple(file.shape) == (3, H, W) and same(file, P.quantise(want))
        row = stats["agreement"][i]
        print("view", i, "time", t, "faces", len(faces), {k: row[k] for k in ("count", "abs_rel", "rmse", "delta1", "iou", "pixels")})
        assert set(row) == set(DO.METRIC_NAMES) | {"iou", "pixels"} and row["pixels"] == H * W and row["count"] > 200
        assert all(math.isfinite(row[k]) for k in row) and 0 < row["iou"] <= 1
        again = MR.agreement(raster, DO.render_depth(cam, scene.pc, scene.pipe, IT, time=t))
        assert again == row
    # meshes of the caller's: the same files; a time that is missing is an error
    given_dir, given = ER.render_mesh_views(str(tmp_path / "given" / "model"), "test", IT, views, scene.pc, scene.pipe, scene.bg, meshes=meshes, mode="normals")
    assert "agreement" not in given and "video" not in given and sorted(os.listdir(given_dir)) == ["00000.png", "00001.png", "00002.png"]
    want = P.quantise(MR.render_mesh(meshes[float(np.asarray(views[1].time, dtype=F).reshape(-1)[0])], views[1], mode="normals").cpu().numpy())
    assert same(png_decode.decode_files([os.path.join(given_dir, "00001.png")], device=DEV)[0], want)
    with pytest.raises(KeyError, match="no mesh for time"):
        ER.render_mesh_views(str(tmp_path / "none" / "model"), "test", IT, views, scene.pc, scene.pipe, scene.bg, meshes={7.0: meshes[0.0] if 0.0 in meshes else mesh})
