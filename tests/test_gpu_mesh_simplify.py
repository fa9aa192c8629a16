"""Mesh simplification on the device against the numpy restatement tests/mesh_simplify_ref.py on every case and option set of
tests/mesh_simplify_cases.py: bit for bit for the vertices, faces, maps, counts, colours and attributes; every call twice with equal
bytes; the inputs unchanged; the properties of any result; applied twice equals once; the status word; the refusals; a sphere of
Gaussians through render_meshes with and without welding and clustering.

Measured on an MI355X: see DESIGN section 28."""
import os

import numpy as np
import pytest
import torch

import mesh_simplify_cases as cases
import tsdf_ref
from test_gpu_tsdf import IT, RESOLUTION, scene  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = np.float32


def same(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_mesh(m, faces=None):
    from gaussianprediction_amd.tsdf_ops import Mesh
    return Mesh(dev(m.vertices), dev(m.faces if faces is None else faces), dev(m.colors))


def call(mesh, options, attributes=()):
    from gaussianprediction_amd import mesh_simplify as MZ
    options = dict(options)
    voxel = options.pop("voxel_size")
    if voxel is None:
        return MZ.weld(mesh, attributes=attributes, **options)
    return MZ.simplify(mesh, voxel, attributes=attributes, **options)


def tensors(got):
    return [got.mesh.vertices, got.mesh.faces, got.vertex_map, got.face_index, got.vertex_counts, got.mesh.colors, *got.attributes]


def bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_case_equals_the_restatement_and_itself(name):
    m = cases.CASES[name]
    mesh, attribute = device_mesh(m), dev(m.attribute)
    for run in cases.runs_of(name):
        options, want = cases.RUNS[name][run], cases.result(name, run)
        got = call(mesh, options, (attribute,))
        print(name, run, got.stats)
        assert got.stats == want.stats and want.status == 0
        assert [t.dtype for t in tensors(got)] == [torch.float32] + [torch.int32] * 4 + [torch.float32] * 2 and all(t.is_contiguous() for t in tensors(got))
        assert len(got.attributes) == 1 and all(same(g, w) for g, w in zip(tensors(got), cases.parts(want))), (name, run)
        again = call(mesh, options, (attribute,))                # run to run
        assert again.stats == got.stats and all(bytes_equal(a, b) for a, b in zip(tensors(got), tensors(again)))
        v, f, vm, vc = (t.cpu().numpy() for t in (got.mesh.vertices, got.mesh.faces, got.vertex_map, got.vertex_counts))
        cases.check_properties(m, options, v, f, vm, vc)
        if options["voxel_size"] is None or (options.get("contraction") == "first" and options.get("bounds") is not None):          # applied twice equals once
            twice = call(got.mesh, options, got.attributes)
            assert all(bytes_equal(a, b) for a, b in zip((*twice.mesh, *twice.attributes), (*got.mesh, *got.attributes))), (name, run)
            assert twice.stats["collapsed"] == twice.stats["duplicates"] == 0 and bool((twice.vertex_counts == 1).all())
    plain = call(type(mesh)(mesh.vertices, mesh.faces, None), cases.RUNS[name][0])
    assert plain.mesh.colors is None and plain.attributes == () and same(plain.mesh.vertices, cases.result(name, 0).vertices)
    assert same(mesh.vertices, m.vertices) and same(mesh.faces, m.faces) and same(mesh.colors, m.colors) and same(attribute, m.attribute)      # the inputs are read only


def test_the_two_sphere_volume_and_the_volume_with_samples_on_its_iso():
    from gaussianprediction_amd import mesh_simplify as MZ
    m = cases.CASES["two_spheres"]
    mesh = device_mesh(m)
    for voxel, (nv2, nf2, collapsed, duplicates) in cases.TWO_SPHERES.items():
        got = MZ.simplify(mesh, voxel)
        assert (got.mesh.vertices.shape[0], got.mesh.faces.shape[0], got.stats["collapsed"], got.stats["duplicates"], got.stats["unreferenced"]) == (nv2, nf2, collapsed, duplicates, 0)
    facts = tsdf_ref.mesh_facts(got.mesh.vertices.cpu().numpy(), got.mesh.faces.cpu().numpy())
    assert facts["edge_uses"] == {2} and facts["euler"] == 4
    w = MZ.weld(mesh)                                            # nothing to merge, nothing unreferenced: the mesh in equal bytes
    assert same(w.mesh.vertices, m.vertices) and same(w.mesh.faces, m.faces) and same(w.mesh.colors, m.colors) and bool((w.vertex_counts == 1).all())
    e = cases.CASES["equal_iso"]
    w = MZ.weld(device_mesh(e), drop_zero_area=True)
    v, f = w.mesh.vertices.cpu().numpy(), w.mesh.faces.cpu().numpy()
    assert len(v) < len(e.vertices) and len(np.unique((v + F(0)).view(np.uint32), axis=0)) == len(v)
    assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])).all()
    before, after = tsdf_ref.mesh_facts(e.vertices, e.faces)["volume"], tsdf_ref.mesh_facts(v, f)["volume"]
    assert abs(after - before) <= 1e-9 * abs(before) and before != 0


@pytest.mark.parametrize("case, face, corner, value", cases.BAD)
def test_a_face_index_out_of_range_raises_at_the_read(case, face, corner, value):
    from gaussianprediction_amd import _lib, mesh_simplify as MZ
    m = cases.mesh_cases.CASES[case]
    mesh = device_mesh(m, cases.bad_faces(case, face, corner, value))
    with pytest.raises(_lib.GpHipError, match="outside"):
        MZ.weld(mesh)
    with pytest.raises(_lib.GpHipError, match="outside"):
        MZ.simplify(mesh, 0.5, drop_zero_area=True)
    assert MZ.weld(device_mesh(m)).mesh.faces.shape[0] <= len(m.faces)          # the next call is clean


def test_the_status_word_of_the_grid_and_the_device_refusals():
    from gaussianprediction_amd import _lib, mesh_simplify as MZ
    from gaussianprediction_amd.tsdf_ops import Mesh
    m = cases.CASES["one_triangle"]
    mesh = device_mesh(m)
    assert MZ.simplify(mesh, 0.5, bounds=((0, 0, 0), (1, 1, 1))).mesh.faces.shape[0] == 1
    with pytest.raises(_lib.GpHipError, match="outside the bounds"):
        MZ.simplify(mesh, 0.5, bounds=((0, 0, 0), (0.25, 1, 1)))
    for bad in ([np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]):
        v = m.vertices.copy()
        v[1] = bad
        broken = Mesh(dev(v), mesh.faces, None)
        with pytest.raises(_lib.GpHipError, match="not finite"):
            MZ.simplify(broken, 0.5)                             # found by the bounds
        with pytest.raises(_lib.GpHipError, match="not finite"):
            MZ.simplify(broken, 0.5, bounds=((0, 0, 0), (1, 1, 1)))          # found by the keys
        assert MZ.weld(broken).mesh.vertices.shape[0] == 3       # welding compares bits
    for fn, word in ((lambda: MZ.simplify(mesh, 0.0), "finite and > 0"), (lambda: MZ.simplify(mesh, 1e-7), "voxel_size is too small"),
                     (lambda: MZ.simplify(mesh, 0.5, contraction="median"), "contraction must be"), (lambda: MZ.simplify(mesh, 0.5, bounds=((0, 2, 0), (1, 1, 1))), "min <= max")):
        with pytest.raises(_lib.GpHipError, match=word):
            fn()
    for fn, word in ((lambda: MZ.weld(Mesh(mesh.vertices.cpu(), mesh.faces, None)), "no CPU fallback"), (lambda: MZ.weld(mesh, attributes=(torch.zeros(3, 2),)), "no CPU fallback"),
                     (lambda: MZ.weld(mesh, attributes=(mesh.vertices[:2],)), "attributes"), (lambda: MZ.weld(Mesh(mesh.vertices, mesh.faces, mesh.colors[:2])), "colors"),
                     (lambda: MZ.simplify(Mesh(mesh.vertices.double(), mesh.faces, None), 0.5), "float32")):
        with pytest.raises(RuntimeError, match=word):
            fn()


def test_render_meshes_with_and_without_the_simplification(scene, tmp_path):  # noqa: F811
    from gaussianprediction_amd import eval_render as ER, io_formats, mesh_simplify as MZ, tsdf_ops as TO
    times = [0.25, 0.75]
    box = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
    plain_dir, plain = ER.render_meshes(str(tmp_path / "plain"), "test", IT, scene.cams, scene.pc, scene.pipe, scene.bg, times=times, resolution=RESOLUTION)
    light_dir, stats = ER.render_meshes(str(tmp_path / "light"), "test", IT, scene.cams, scene.pc, scene.pipe, scene.bg, times=times, resolution=RESOLUTION,
                                        weld=True, simplify_voxel=0.2)
    boxed_dir, boxed = ER.render_meshes(str(tmp_path / "boxed"), "test", IT, scene.cams, scene.pc, scene.pipe, scene.bg, times=times, resolution=RESOLUTION, bounds=box,
                                        simplify_voxel=0.2, simplify_contraction="first")
    assert "fused_vertices" not in plain and len(stats["fused_vertices"]) == len(stats["fused_faces"]) == 2 and "components" not in stats
    for i, t in enumerate(times):
        mesh = TO.fuse(scene.cams, scene.pc, scene.pipe, IT, time=t, resolution=RESOLUTION, background=scene.bg)
        path = str(tmp_path / "want.ply")
        io_formats.save_mesh_ply(path, mesh.vertices, mesh.faces, mesh.colors)
        assert open(path, "rb").read() == open(os.path.join(plain_dir, f"{i:05d}.ply"), "rb").read()          # the defaults: the files as they were
        want = MZ.simplify(MZ.weld(mesh).mesh, 0.2).mesh
        io_formats.save_mesh_ply(path, want.vertices, want.faces, want.colors)
        assert open(path, "rb").read() == open(os.path.join(light_dir, f"{i:05d}.ply"), "rb").read()
        assert (stats["fused_vertices"][i], stats["fused_faces"][i]) == (mesh.vertices.shape[0], mesh.faces.shape[0]) == (plain["vertices"][i], plain["faces"][i])
        assert (stats["vertices"][i], stats["faces"][i]) == (want.vertices.shape[0], want.faces.shape[0]) and 0 < stats["vertices"][i] < stats["fused_vertices"][i]
        fixed = TO.fuse(scene.cams, scene.pc, scene.pipe, IT, time=t, resolution=RESOLUTION, background=scene.bg, bounds=box)
        want = MZ.simplify(fixed, 0.2, contraction="first", bounds=box).mesh          # the caller's box is the grid's, too
        io_formats.save_mesh_ply(path, want.vertices, want.faces, want.colors)
        assert open(path, "rb").read() == open(os.path.join(boxed_dir, f"{i:05d}.ply"), "rb").read()
        assert (boxed["vertices"][i], boxed["faces"][i]) == (want.vertices.shape[0], want.faces.shape[0])
        print("time", t, "fused", stats["fused_vertices"][i], stats["fused_faces"][i], "written", stats["vertices"][i], stats["faces"][i])
