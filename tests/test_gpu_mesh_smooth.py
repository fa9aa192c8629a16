"""Mesh topology and smoothing on the device against the numpy restatement tests/mesh_smooth_ref.py on every case and option set of
tests/mesh_smooth_cases.py: bit for bit for the edges, counts, adjacency, flags, smoothed rows and umbrella (a NaN the arithmetic made: a NaN in the
same place); every call twice with equal bytes; the inputs unchanged; topology= against the call without it; the status word; the refusals; dtypes and contiguity; the
fused sphere of Gaussians: its edges against the restatement (which finds holes where DESIGN section 26 says watertight: section
32), smoother after Taubin, smaller after Laplacian; render_meshes with and without the new arguments.

Measured on an MI355X: see DESIGN section 32."""
import json
import os

import numpy as np
import pytest
import torch

import mesh_smooth_cases as cases
import mesh_smooth_ref as ref
from test_gpu_tsdf import IT, RESOLUTION, scene  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = np.float32


def same(a, b, strict=False):
    """Equal bytes; where the arithmetic made a NaN, a NaN in the same place (IEEE 754 states neither the sign nor the payload of a
    NaN result, and the host's and the device's differ: gp_mesh_smooth.h section 6)."""
    a, b = (np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t) for t in (a, b))
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == F and not strict and np.isnan(b).any():
        nan = np.isnan(b)
        return np.array_equal(np.isnan(a), nan) and np.where(nan, F(0), a).tobytes() == np.where(nan, F(0), b).tobytes()
    return a.tobytes() == b.tobytes()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def topology_tensors(t):
    return [t.edge, t.face_count, t.wind, t.offsets, t.neighbors, t.vertex_flags]


def smoothed_tensors(s):
    return [s.mesh.vertices, *s.attributes]


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_case_equals_the_restatement_and_itself(name):
    from gaussianprediction_amd import mesh_smooth as MT
    from gaussianprediction_amd.tsdf_ops import Mesh
    m, want = cases.CASES[name], cases.topology(name)
    nv = len(m.vertices)
    faces, vertices, rows = dev(m.faces), dev(m.vertices), [dev(r) for r in m.rows]
    colors = dev(m.rows[1][:, :3])
    topo = MT.edges(faces, nv)
    print(name, topo.stats)
    assert topo.stats == want.stats and want.status == 0 and all(same(g, w) for g, w in zip(topology_tensors(topo), ref.parts(want)))
    assert [t.dtype for t in topology_tensors(topo)] == [torch.int32] * 5 + [torch.uint8] and all(t.is_contiguous() for t in topology_tensors(topo))
    again = MT.edges(faces, nv)                                  # run to run
    assert again.stats == topo.stats and all(bytes_equal(a, b) for a, b in zip(topology_tensors(topo), topology_tensors(again)))
    t = {k: v.cpu().numpy() for k, v in zip(MT.Edges._fields, topology_tensors(topo))}
    cases.check_properties(nv, len(m.faces), t["edge"], t["face_count"], t["wind"], t["offsets"], t["neighbors"], t["vertex_flags"], topo.stats)
    for r, w in zip([vertices] + rows, cases.umbrella(name)):
        u = MT.umbrella(r, topo)
        assert u.dtype == torch.float32 and u.is_contiguous() and same(u, w) and bytes_equal(u, MT.umbrella(r, topo))
    mesh = Mesh(vertices, faces, colors)
    for run in cases.runs_of(name):
        options = cases.RUNS[name][run]
        got = MT.smooth(mesh, attributes=rows, topology=topo, **options)
        assert all(same(g, w) for g, w in zip(smoothed_tensors(got), cases.smoothed(name, run))), (name, run)
        assert all(t.dtype == torch.float32 and t.is_contiguous() for t in smoothed_tensors(got)) and got.mesh.faces is faces and got.topology is topo
        assert bytes_equal(got.mesh.colors, colors)              # colors=False: they pass through
        assert got.stats["steps"] == options["iterations"] * (2 if options["method"] == "taubin" else 1)
        assert int(got.stats["pinned"]) == ref.pinned_count(want, options["boundary"])
        twice = MT.smooth(mesh, attributes=rows, **options)      # run to run, and without topology=: the same bytes
        assert all(bytes_equal(a, b) for a, b in zip(smoothed_tensors(got), smoothed_tensors(twice)))
        assert all(bytes_equal(a, b) for a, b in zip(topology_tensors(topo), topology_tensors(twice.topology)))
    tinted = MT.smooth(mesh, colors=True, topology=topo, **cases.RUNS[name][-1])
    assert tinted.attributes == () and same(tinted.mesh.colors, cases.smoothed(name, len(cases.RUNS[name]) - 1)[2][:, :3])          # the colours take the same steps
    plain = MT.smooth(Mesh(vertices, faces, None), topology=topo, **cases.RUNS[name][0])
    assert plain.mesh.colors is None and same(plain.mesh.vertices, cases.smoothed(name, 0)[0])
    assert same(vertices, m.vertices, True) and same(faces, m.faces) and same(colors, m.rows[1][:, :3], True) and all(same(r, w, True) for r, w in zip(rows, m.rows))      # the inputs are read only
    assert all(same(g, w) for g, w in zip(topology_tensors(topo), ref.parts(want)))


def test_exact_results_that_need_no_restatement():
    from gaussianprediction_amd import mesh_smooth as MT
    from gaussianprediction_amd.tsdf_ops import Mesh
    v, f = cases.OCTAHEDRON
    mesh = Mesh(dev(v), dev(f), None)
    for n in (1, 2, 5, 30):
        assert same(MT.smooth(mesh, n, "laplacian", lambda_=0.5).mesh.vertices, v * F(2.0 ** -n))
    tri = cases.CASES["one_triangle"]
    mesh = Mesh(dev(tri.vertices), dev(tri.faces), None)
    for method in ("laplacian", "taubin"):
        held = MT.smooth(mesh, 5, method, boundary="fixed")
        assert same(held.mesh.vertices, tri.vertices) and int(held.stats["pinned"]) == 3 and not same(MT.smooth(mesh, 5, method, boundary="free").mesh.vertices, tri.vertices)
    for name in ("not_finite", "hub", "cube_soup"):
        m = cases.CASES[name]
        got = MT.smooth(Mesh(dev(m.vertices), dev(m.faces), None), 0, attributes=[dev(r) for r in m.rows])
        assert same(got.mesh.vertices, m.vertices, strict=True) and all(same(g, w, strict=True) for g, w in zip(got.attributes, m.rows)) and got.stats["steps"] == 0          # a NaN that is copied keeps its bits


@pytest.mark.parametrize("case, face, corner, value", cases.BAD)
def test_a_face_index_out_of_range_raises_at_the_read(case, face, corner, value):
    from gaussianprediction_amd import _lib, mesh_smooth as MT
    from gaussianprediction_amd.tsdf_ops import Mesh
    m = cases.CASES[case]
    bad = dev(cases.bad_faces(case, face, corner, value))
    with pytest.raises(_lib.GpHipError, match="outside"):
        MT.edges(bad, len(m.vertices))
    with pytest.raises(_lib.GpHipError, match="outside"):
        MT.smooth(Mesh(dev(m.vertices), bad, None), 1)
    assert MT.edges(dev(m.faces), len(m.vertices)).stats == cases.topology(case).stats          # the next call is clean


def test_the_refusals_dtypes_and_contiguity():
    from gaussianprediction_amd import _lib, mesh_smooth as MT
    from gaussianprediction_amd.tsdf_ops import Mesh
    m = cases.CASES["octahedron"]
    vertices, faces = dev(m.vertices), dev(m.faces)
    mesh, topo = Mesh(vertices, faces, None), MT.edges(faces, 6)
    for fn, word in ((lambda: MT.smooth(mesh, lambda_=float("nan")), "must be finite"), (lambda: MT.smooth(mesh, mu=float("-inf")), "must be finite"),
                     (lambda: MT.smooth(mesh, iterations=10001), "iterations must be"), (lambda: MT.smooth(mesh, iterations=-1), "iterations must be"),
                     (lambda: MT.smooth(mesh, method="cotangent"), "method must be"), (lambda: MT.smooth(mesh, boundary="sliding"), "boundary must be")):
        with pytest.raises(_lib.GpHipError, match=word):
            fn()
    l = MT.lib()                                                 # the library words the same refusals itself
    scratch = torch.empty(1024, dtype=torch.uint8, device=DEV)
    out = torch.empty(6, 3, device=DEV)
    for kw, word in ((dict(method=5), "method must be"), (dict(boundary=5), "boundary must be"), (dict(iterations=10001), "iterations must be"), (dict(lambda_=float("nan")), "must be finite")):
        a = dict(dict(method=MT.TAUBIN, boundary=MT.FIXED, iterations=1, lambda_=0.5, mu=-0.53), **kw)
        rc = l.gp_mesh_smooth_steps(vertices, 6, 3, topo.offsets, topo.neighbors, 24, topo.vertex_flags, a["method"], a["boundary"], a["iterations"], a["lambda_"], a["mu"], scratch, out, None,
                                    _lib.stream_ptr(vertices.device))
        assert rc == 1 and word in _lib.last_error() and MT.check_options("taubin" if "method" not in kw else "x", "fixed" if "boundary" not in kw else "x", a["iterations"], a["lambda_"], a["mu"]) in _lib.last_error()
    cpu = Mesh(vertices.cpu(), faces, None)
    for fn, word in ((lambda: MT.edges(faces.cpu(), 6), "no CPU fallback"), (lambda: MT.smooth(cpu), "no CPU fallback"), (lambda: MT.smooth(mesh, attributes=(torch.zeros(6, 2),)), "no CPU fallback"),
                     (lambda: MT.umbrella(vertices.cpu(), topo), "no CPU fallback"), (lambda: MT.smooth(mesh, topology=topo._replace(offsets=topo.offsets.cpu())), "no CPU fallback"),
                     (lambda: MT.smooth(mesh, attributes=(vertices[:2],)), "attributes"), (lambda: MT.smooth(Mesh(vertices, faces, vertices[:2])), "colors"),
                     (lambda: MT.smooth(Mesh(vertices.double(), faces, None)), "float32"), (lambda: MT.edges(faces.long(), 6), "int32"),
                     (lambda: MT.smooth(mesh, topology=topo._replace(offsets=topo.offsets[:-1])), "offsets"), (lambda: MT.smooth(mesh, topology=topo._replace(vertex_flags=topo.vertex_flags.int())), "vertex_flags"),
                     (lambda: MT.smooth(mesh, topology=(1, 2)), "must be an Edges"), (lambda: MT.umbrella(vertices, topo._replace(neighbors=topo.neighbors.long())), "neighbors")):
        with pytest.raises(RuntimeError, match=word):
            fn()
    # views that are not contiguous are read as what they show
    wide = torch.zeros(6, 6, device=DEV)
    wide[:, ::2] = vertices
    faces_t = faces.t().contiguous().t()
    assert not wide[:, ::2].is_contiguous() and not faces_t.is_contiguous()
    got = MT.smooth(Mesh(wide[:, ::2], faces_t, None), 3)
    assert bytes_equal(got.mesh.vertices, MT.smooth(mesh, 3, topology=topo).mesh.vertices) and bytes_equal(MT.edges(faces_t, 6).edge, topo.edge)
    # a list that is not one of this mesh leaves its vertex unchanged, and nothing is read out of bounds
    wrong = topo._replace(neighbors=topo.neighbors + 3)
    moved = MT.smooth(mesh, 1, "laplacian", boundary="free", topology=wrong).mesh.vertices.cpu().numpy()
    names_outside = np.array([(topo.neighbors.cpu().numpy()[4 * v:4 * v + 4] + 3 >= 6).any() for v in range(6)])
    assert names_outside.any() and same(moved[names_outside], m.vertices[names_outside])


def _fused(scene, time=0.25):  # noqa: F811
    from gaussianprediction_amd import tsdf_ops as TO
    return TO.fuse(scene.cams, scene.pc, scene.pipe, IT, time=time, resolution=RESOLUTION, background=scene.bg)


def test_the_fused_sphere_equals_the_restatement_is_smoother_after_taubin_and_smaller_after_laplacian(scene):  # noqa: F811
    from gaussianprediction_amd import mesh_simplify as MZ, mesh_smooth as MT
    mesh = _fused(scene)
    v, f = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    topo, want = MT.edges(mesh.faces, len(v)), ref.edges(f, len(v))
    print("fused sphere", len(v), len(f), topo.stats)
    assert topo.stats == want.stats and all(same(g, w) for g, w in zip(topology_tensors(topo), ref.parts(want)))
    # DESIGN section 26 says "watertight": that holds where every cell around the surface was observed.  The restatement finds boundary
    # edges on this mesh (seven cameras on one orbit leave cells below min_weight: section 32 records it), so what is asserted is what
    # the restatement gives, and that what is there is a manifold, consistently wound surface with holes
    welded = MT.edges(MZ.weld(mesh).mesh.faces, MZ.weld(mesh).mesh.vertices.shape[0])
    print("welded", welded.stats)
    assert topo.stats["boundary"] == want.stats["boundary"] and topo.stats["nonmanifold"] == 0 and topo.stats["inconsistent"] == 0 and topo.stats["degenerate"] == 0
    assert int((topo.vertex_flags & 1).sum()) == int((want.vertex_flags & 1).sum()) and (topo.stats["boundary"] == 0) == topo.stats["watertight"]
    taubin = MT.smooth(mesh, 10, "taubin", topology=topo)
    laplacian = MT.smooth(mesh, 10, "laplacian", topology=topo)
    assert same(taubin.mesh.vertices, ref.smooth(v, want, 10, "taubin", one_step=ref.step_vectorised)) and bytes_equal(taubin.mesh.colors, mesh.colors)
    assert same(laplacian.mesh.vertices, ref.smooth(v, want, 10, "laplacian", one_step=ref.step_vectorised)) and laplacian.mesh.faces is mesh.faces
    length = lambda m: float(MT.umbrella(m.vertices, topo).double().norm(dim=1).mean())          # noqa: E731
    rough = [length(mesh), length(taubin.mesh), length(laplacian.mesh)]
    volume = [ref.enclosed_volume(m.vertices.cpu().numpy(), f) for m in (mesh, taubin.mesh, laplacian.mesh)]
    print("mean umbrella length", rough, "enclosed volume", volume)
    assert rough[1] < rough[0]                                   # ten Taubin iterations take roughness out
    assert volume[2] < volume[1]                                 # Laplacian shrinks, Taubin far less


def test_render_meshes_with_and_without_the_smoothing(scene, tmp_path):  # noqa: F811
    from gaussianprediction_amd import eval_render as ER, io_formats, mesh_ops, mesh_smooth as MT
    times = [0.25, 0.75]
    common = dict(times=times, resolution=RESOLUTION)
    plain_dir, plain = ER.render_meshes(str(tmp_path / "plain"), "test", IT, scene.cams, scene.pc, scene.pipe, scene.bg, **common)
    named_dir, named = ER.render_meshes(str(tmp_path / "named"), "test", IT, scene.cams, scene.pc, scene.pipe, scene.bg, smooth=0, smooth_method="taubin", smooth_boundary="fixed",
                                        topology_report=False, **common)
    soft_dir, soft = ER.render_meshes(str(tmp_path / "soft"), "test", IT, scene.cams, scene.pc, scene.pipe, scene.bg, smooth=5, normals=True, topology_report=True, **common)
    assert "topology" not in plain and "topology" not in named and sorted(os.listdir(plain_dir)) == sorted(os.listdir(named_dir)) == ["00000.ply", "00001.ply"]
    rows = json.load(open(os.path.join(soft_dir, "mesh_topology.json")))
    assert rows == soft["topology"] and len(rows) == 2 and sorted(os.listdir(soft_dir)) == ["00000.ply", "00001.ply", "mesh_topology.json"]
    for i, t in enumerate(times):
        file = f"{i:05d}.ply"
        assert open(os.path.join(plain_dir, file), "rb").read() == open(os.path.join(named_dir, file), "rb").read()          # the defaults: the files as they were
        mesh = _fused(scene, t)
        path = str(tmp_path / "want.ply")
        io_formats.save_mesh_ply(path, mesh.vertices, mesh.faces, mesh.colors)
        assert open(path, "rb").read() == open(os.path.join(plain_dir, file), "rb").read()
        mesh = mesh_ops.filter_components(mesh, components=mesh_ops.connected_components(mesh.faces, mesh.vertices.shape[0])).mesh          # normals=True goes through the cleanup
        topo = MT.edges(mesh.faces, mesh.vertices.shape[0])
        want = MT.smooth(mesh, 5, topology=topo).mesh
        got = io_formats.read_mesh_ply(os.path.join(soft_dir, file), normals=True)
        assert same(np.asarray(got[0], F), want.vertices) and np.array_equal(np.asarray(got[1]), mesh.faces.cpu().numpy()) and not same(np.asarray(got[0], F), mesh.vertices)
        assert same(np.asarray(got[-1], F), mesh_ops.vertex_normals(want.vertices, want.faces))          # the normals of the smoothed surface
        assert rows[i] == dict(topo.stats, frame=i, time=t) and rows[i]["nonmanifold"] == 0 and rows[i]["edges"] > 1000
        assert (soft["vertices"][i], soft["faces"][i]) == (want.vertices.shape[0], want.faces.shape[0])
