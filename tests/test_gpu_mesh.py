"""Mesh cleanup on the device against the numpy restatement tests/mesh_ref.py on every case of tests/mesh_cases.py: bit for bit for the
labels, the table, the filter's indices, faces, colours and attributes and the normals; every entry twice with equal bytes; the
result whatever the rounds granted per read; the rounds of the path case under its cap; the two-sphere volume from
TsdfVolume.extract; face indices out of range; a sphere of Gaussians through render_meshes with and without the cleanup.

Measured on an MI355X: see DESIGN section 27."""
import os

import numpy as np
import pytest
import torch

import mesh_cases as cases
import mesh_ref as ref
import tsdf_ref
from test_gpu_tsdf import IT, RESOLUTION, device_volume, scene  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = np.float32


def same(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_mesh(m):
    from gaussianprediction_amd.tsdf_ops import Mesh
    return Mesh(dev(m.vertices), dev(m.faces), dev(m.colors))


def check_components(got, want):
    _, vertex_label, face_label, labels, vertex_counts, face_counts = want
    assert all(t.dtype == torch.int32 for t in got[:5])
    assert same(got.vertex_label, vertex_label) and same(got.face_label, face_label)
    assert same(got.labels, labels) and same(got.vertex_counts, vertex_counts) and same(got.face_counts, face_counts)


def check_filtered(got, want):
    status, vertices, faces, vertex_index, face_index, rows = want
    assert same(got.mesh.vertices, vertices) and same(got.mesh.faces, faces) and same(got.vertex_index, vertex_index) and same(got.face_index, face_index)
    assert same(got.mesh.colors, rows[0]) and len(got.attributes) == 1 and same(got.attributes[0], rows[1])


def bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


@pytest.mark.parametrize("name", list(cases.CASES))
def test_components_equal_the_restatement_whatever_the_rounds_granted(name):
    from gaussianprediction_amd import mesh_ops as MO
    m = cases.CASES[name]
    faces, nv = dev(m.faces), len(m.vertices)
    got = MO.connected_components(faces, nv)
    print(name, "rounds", got.rounds, "components", int(got.labels.shape[0]))
    check_components(got, cases.components(name))
    for per in (1, 2, 64):                                       # one round per read, two, and far more than needed
        again = MO.connected_components(faces, nv, rounds_per_read=per)
        check_components(again, cases.components(name))
        assert 1 <= again.rounds <= max(got.rounds, cases.STRIP_CAP)          # (the rounds are the device's own: stale loads may cost one)
    if name == "strip":
        assert got.rounds <= cases.STRIP_CAP == 60              # a scheme bound by the diameter needs about 2048
    assert same(faces, m.faces)                                  # the mesh is read only


@pytest.mark.parametrize("name", list(cases.CASES))
def test_filter_and_normals_equal_the_restatement_and_themselves(name):
    from gaussianprediction_amd import mesh_ops as MO
    m = cases.CASES[name]
    mesh, attribute = device_mesh(m), dev(m.attribute)
    comps = MO.connected_components(mesh.faces, len(m.vertices))
    for min_triangles, keep_largest in cases.filters_of(name):
        got = MO.filter_components(mesh, min_triangles, keep_largest, components=comps, attributes=(attribute,))
        check_filtered(got, cases.filtered(name, min_triangles, keep_largest))
        again = MO.filter_components(mesh, min_triangles, keep_largest, attributes=(attribute,))          # its own components; run to run
        assert all(bytes_equal(a, b) for a, b in zip((*got.mesh, got.vertex_index, got.face_index, *got.attributes),
                                                      (*again.mesh, again.vertex_index, again.face_index, *again.attributes)))
        cleaned, normals = MO.clean(mesh, min_triangles, keep_largest, normals=True)
        assert bytes_equal(cleaned.vertices, got.mesh.vertices) and bytes_equal(cleaned.faces, got.mesh.faces) and bytes_equal(cleaned.colors, got.mesh.colors)
        want = cases.filtered(name, min_triangles, keep_largest)
        assert same(normals, ref.vertex_normals(want[1], want[2]))
    plain = MO.filter_components(type(mesh)(mesh.vertices, mesh.faces, None), components=comps)
    assert plain.mesh.colors is None and plain.attributes == () and same(plain.mesh.vertices, cases.filtered(name, None, None)[1])
    normals = MO.vertex_normals(mesh.vertices, mesh.faces)
    assert normals.dtype == torch.float32 and same(normals, cases.normals(name)) and bool(torch.isfinite(normals).all())
    assert bytes_equal(MO.vertex_normals(mesh.vertices, mesh.faces), normals)
    assert same(mesh.vertices, m.vertices) and same(mesh.faces, m.faces)


def test_the_two_sphere_volume_from_extract():
    from gaussianprediction_amd import mesh_ops as MO
    mesh = device_volume(cases.two_sphere_volume()).extract()
    assert tuple(mesh.vertices.shape) == (3932, 3) and tuple(mesh.faces.shape) == (7856, 3) and mesh.colors is None
    comps = MO.connected_components(mesh.faces, 3932)
    assert comps.labels.tolist() == [0, 1382] and comps.vertex_counts.tolist() == [3630, 302] and comps.face_counts.tolist() == [7256, 600]
    kept, normals = MO.clean(mesh, keep_largest=1, normals=True)
    vertices, faces = kept.vertices.cpu().numpy(), kept.faces.cpu().numpy()
    facts = tsdf_ref.mesh_facts(vertices, faces)
    assert (facts["V"], facts["F"]) == (3630, 7256) and facts["edge_uses"] == {2} and facts["euler"] == 2 and facts["unreferenced"] == 0 and facts["volume"] > 0
    assert bool(((normals.double() * (kept.vertices.double() - torch.tensor(cases.TWO_SPHERES.c0, device=DEV, dtype=torch.float64))).sum(dim=1) > 0).all())
    assert same(normals, ref.vertex_normals(vertices, faces))


@pytest.mark.parametrize("case, face, corner, value", cases.BAD)
def test_a_face_index_out_of_range_is_skipped_and_raises(case, face, corner, value):
    from gaussianprediction_amd import _lib, mesh_ops as MO
    from gaussianprediction_amd.tsdf_ops import Mesh
    m = cases.CASES[case]
    nv, faces = len(m.vertices), cases.bad_faces(case, face, corner, value)
    with pytest.raises(_lib.GpHipError, match="outside"):
        MO.connected_components(dev(faces), nv)
    with pytest.raises(_lib.GpHipError, match="outside"):
        MO.clean(Mesh(dev(m.vertices), dev(faces), None), keep_largest=1)
    good = MO.connected_components(dev(m.faces), nv)
    with pytest.raises(_lib.GpHipError, match="outside"):       # the filter checks the faces it is handed, too
        MO.filter_components(Mesh(dev(m.vertices), dev(faces), None), components=good)
    state = torch.zeros(4, dtype=torch.int32, device=DEV)
    normals = MO.vertex_normals(dev(m.vertices), dev(faces), state=state)
    assert state.tolist() == [1, 0, 0, 0] and same(normals, ref.vertex_normals(m.vertices, faces))      # the face contributes nothing


def test_the_device_refusals():
    from gaussianprediction_amd import _lib, mesh_ops as MO
    from gaussianprediction_amd.tsdf_ops import Mesh
    m = cases.CASES["two_disjoint"]
    mesh = device_mesh(m)
    for call, word in ((lambda: MO.connected_components(mesh.faces, 2 ** 31), "nv must be below"), (lambda: MO.connected_components(mesh.faces, -1), ">= 0"),
                       (lambda: MO.connected_components(mesh.faces, 6, rounds_per_read=0), "rounds_per_read"), (lambda: MO.filter_components(mesh, min_triangles=-1), "min_triangles"),
                       (lambda: MO.filter_components(mesh, keep_largest=2 ** 31), "keep_largest")):
        with pytest.raises(_lib.GpHipError, match=word):
            call()
    for call, word in ((lambda: MO.connected_components(mesh.faces.cpu(), 6), "no CPU fallback"), (lambda: MO.vertex_normals(mesh.vertices.cpu(), mesh.faces), "no CPU fallback"),
                       (lambda: MO.filter_components(mesh, attributes=(torch.zeros(6, 2),)), "no CPU fallback"), (lambda: MO.filter_components(mesh, attributes=(mesh.vertices[:5],)), "attributes"),
                       (lambda: MO.filter_components(Mesh(mesh.vertices, mesh.faces, mesh.colors[:4])), "colors"), (lambda: MO.vertex_normals(mesh.vertices.double(), mesh.faces), "float32"),
                       (lambda: MO.filter_components(mesh, components=MO.connected_components(mesh.faces[1:], 3)), "not those of this mesh")):
        with pytest.raises(RuntimeError, match=word):
            call()


def test_render_meshes_with_and_without_the_cleanup(scene, tmp_path):  # noqa: F811
    from gaussianprediction_amd import eval_render as ER, io_formats, mesh_ops as MO, tsdf_ops as TO
    times = [0.25, 0.75]
    plain_dir, plain = ER.render_meshes(str(tmp_path / "plain"), "test", IT, scene.cams, scene.pc, scene.pipe, scene.bg, times=times, resolution=RESOLUTION)
    clean_dir, stats = ER.render_meshes(str(tmp_path / "clean"), "test", IT, scene.cams, scene.pc, scene.pipe, scene.bg, times=times, resolution=RESOLUTION,
                                        keep_largest=1, normals=True)
    assert "components" not in plain and len(stats["components"]) == 2 and min(stats["components"]) >= 1
    for i, t in enumerate(times):
        mesh = TO.fuse(scene.cams, scene.pc, scene.pipe, IT, time=t, resolution=RESOLUTION, background=scene.bg)
        path = str(tmp_path / "want.ply")
        io_formats.save_mesh_ply(path, mesh.vertices, mesh.faces, mesh.colors)
        assert open(path, "rb").read() == open(os.path.join(plain_dir, f"{i:05d}.ply"), "rb").read()          # the defaults: the files as they were
        kept, normals = MO.clean(mesh, keep_largest=1, normals=True)
        vertices, faces, colors, held = io_formats.read_mesh_ply(os.path.join(clean_dir, f"{i:05d}.ply"), normals=True)
        assert same(kept.vertices, vertices) and same(kept.faces, faces) and same(normals, held) and same(io_formats.color_to_uint8(kept.colors.cpu().numpy()), colors)
        assert (stats["vertices"][i], stats["faces"][i]) == (len(vertices), len(faces)) and len(vertices) <= mesh.vertices.shape[0]
        assert stats["components"][i] == int(MO.connected_components(mesh.faces, mesh.vertices.shape[0]).labels.shape[0])
        outward = (normals.double() * (kept.vertices.double() - torch.tensor([0.3 * t, 0.0, 0.0], device=DEV, dtype=torch.float64))).sum(dim=1)
        print("time", t, "components", stats["components"][i], "kept", len(vertices), "of", mesh.vertices.shape[0], "outward normals", float((outward > 0).double().mean()))
