"""The topology of a triangle mesh and Laplacian / Taubin smoothing on the device (csrc/gp_mesh_smooth.h,
csrc/mesh_smooth_kernels.hip).

edges builds what no other module here knows: the unique undirected edges of a mesh in ascending order, the faces on each and
their winding, every vertex's neighbours in CSR form, the boundary and non-manifold vertices, and the counts a report needs
(boundary, non-manifold and inconsistently wound edges, the Euler characteristic).  smooth runs Jacobi steps p + s (mean of the
neighbours - p) over those lists, in float64 with the neighbours summed in ascending index, on the positions and on any per-vertex
rows: a marching-tetrahedra mesh carries the staircase of its lattice, and Taubin's lambda | mu pair takes it out without the
shrinkage of plain Laplacian steps.  Everything has a stated order: two runs give equal bytes.  The header states every definition
in full, tests/mesh_smooth_ref.py restates them in numpy and the tests pin that.

HIP only: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple

import torch

from . import _lib
from .mesh_ops import _faces, _rows
from .tsdf_ops import Mesh

GP_MESH_SMOOTH_ABI_VERSION = 1    # csrc/gp_mesh_smooth.h
LAPLACIAN, TAUBIN = 0, 1
FREE, FIXED = 0, 1
MAX_ITERATIONS = 10000
FLAG_BOUNDARY, FLAG_NONMANIFOLD, FLAG_ISOLATED = 1, 2, 4
STATUS, EDGES, BOUNDARY, NONMANIFOLD, INCONSISTENT, DEGENERATE, VERTICES, FACES, COUNT_WORDS = 0, 1, 2, 3, 4, 5, 6, 7, 8
HEADER = "../gaussianprediction_amd/csrc/gp_mesh_smooth.h"      # relative to include/: the header is not one of include/ 
METHODS = {"laplacian": LAPLACIAN, "taubin": TAUBIN}
BOUNDARIES = {"free": FREE, "fixed": FIXED}
COUNT_NAMES = ("status", "edges", "boundary", "nonmanifold", "inconsistent", "degenerate", "vertices", "faces")


def _prototypes():
    i32, i64, f64, P = C.c_int32, C.c_int64, C.c_double, _lib.Ptr
    return {   # name: (restype, argtypes), as csrc/gp_mesh_smooth.h declares them (tests/test_mesh_smooth_host.py compares the two)
        "gp_mesh_smooth_abi_version": (i32, []),
        "gp_mesh_smooth_scratch_bytes": (i64, [i64, i64]),
        "gp_mesh_smooth_edges_plan": (i32, [P, i64, i64, P, P, P]),
        "gp_mesh_smooth_edges_apply": (i32, [i64, i64, i64, P, P, P, P, P, P, P, P]),
        "gp_mesh_smooth_rows_bytes": (i64, [i64, i32]),
        "gp_mesh_smooth_steps": (i32, [P, i64, i32, P, P, i64, P, i32, i32, i32, f64, f64, P, P, P, P]),
        "gp_mesh_smooth_umbrella": (i32, [P, i64, i32, P, P, i64, P, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi(HEADER, "gp_mesh_smooth_abi_version", GP_MESH_SMOOTH_ABI_VERSION, PROTOTYPES, register=False)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)

# edge [E, 2]: the pairs (lo, hi), ascending; face_count, wind [E]; offsets [Nv + 1], neighbors [2E]: the adjacency in CSR form,
# every list ascending, all int32 on the device; vertex_flags [Nv] uint8 (1: on a boundary edge, 2: on a non-manifold edge, 4: degree
# 0); stats: the eight counts by name (COUNT_NAMES), "euler" and "watertight"
Edges = namedtuple("Edges", "edge face_count wind offsets neighbors vertex_flags stats")
# mesh: the smoothed tsdf_ops.Mesh (the faces are the input's tensor); attributes: the tensors handed in, smoothed alike; topology:
# the Edges used; stats: {"steps": launches per array, "pinned": a one-element int32 tensor on the device, the vertices held}
Smoothed = namedtuple("Smoothed", "mesh attributes topology stats")


def check_sizes(n_vertices, n_faces):
    """The library's refusal of the sizes, as it words it (None: accepted)."""
    from .mesh_ops import check_sizes as base
    why = base(n_vertices, n_faces)
    if why is None and 6 * int(n_faces) >= 2 ** 31:
        why = "6*nf must be below 2^31"
    return why


def check_options(method, boundary, iterations, lambda_, mu):
    """The library's refusal of smooth's options, as it words it (None: accepted)."""
    if method not in METHODS:
        return "method must be \"laplacian\" or \"taubin\""
    if boundary not in BOUNDARIES:
        return "boundary must be \"fixed\" or \"free\""
    if isinstance(iterations, bool) or not isinstance(iterations, int) or not 0 <= iterations <= MAX_ITERATIONS:
        return "iterations must be 0 .. 10000"
    if not math.isfinite(float(lambda_)) or not math.isfinite(float(mu)):
        return "lambda_ and mu must be finite"
    return None


def _room(n, *shape, dtype, device):          # (an empty tensor has no pointer to hand over: one row at the least, cut by the caller)
    return torch.empty(max(n, 1), *shape, dtype=dtype, device=device)


def edges(faces, n_vertices):
    """Edges(edge, face_count, wind, offsets, neighbors, vertex_flags, stats) of faces [Nf, 3] int32 over n_vertices vertices.  A face
    (a, b, c) gives the half-edges a->b, b->c, c->a; one with equal ends is dropped and counted ("degenerate").  edge: the unique
    pairs (lo, hi), lo < hi, in ascending lexicographic order; face_count: the half-edges on each (a duplicated face counts twice);
    wind: those running lo->hi minus those running hi->lo, 0 on a consistently oriented interior edge.  The neighbours of vertex v
    are neighbors[offsets[v]:offsets[v + 1]], each once, ascending.  stats: "edges", "boundary" (face_count 1), "nonmanifold" (> 2),
    "inconsistent" (face_count 2, wind != 0), "degenerate", "vertices" (of degree > 0), "faces" (kept), "euler" = vertices - edges +
    faces and "watertight" = no boundary, non-manifold or inconsistent edge and at least one edge.  One read: the eight counts.  A
    face index outside [0, n_vertices) raises GpHipError at that read."""
    what = "edges"
    nv = int(n_vertices)
    faces = _faces(what, faces, nv)
    nf, dev = faces.shape[0], faces.device
    why = check_sizes(nv, nf)
    if why:
        raise _lib.GpHipError(f"{what}: {why} (nv = {nv}, nf = {nf})")
    counts = torch.empty(COUNT_WORDS, dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        st = _lib.stream_ptr(dev)
        scratch = _lib.scratch(lib().gp_mesh_smooth_scratch_bytes, nv, nf, device=dev)
        _lib.check(lib().gp_mesh_smooth_edges_plan(faces, nv, nf, scratch, counts, st), "gp_mesh_smooth_edges_plan")
        read = [int(v) for v in counts.tolist()]              # (the one read of the counts)
        if read[STATUS]:
            raise _lib.GpHipError(f"{what}: a face index lies outside [0, {nv})")
        ne = read[EDGES]
        i32 = dict(dtype=torch.int32, device=dev)
        edge, face_count, wind, neighbors = _room(ne, 2, **i32), _room(ne, **i32), _room(ne, **i32), _room(2 * ne, **i32)
        offsets, flags = torch.empty(nv + 1, **i32), _room(nv, dtype=torch.uint8, device=dev)
        _lib.check(lib().gp_mesh_smooth_edges_apply(nv, nf, ne, scratch, edge, face_count, wind, offsets, neighbors, flags, st), "gp_mesh_smooth_edges_apply")
    stats = dict(zip(COUNT_NAMES[1:], read[1:]))
    stats["euler"] = read[VERTICES] - ne + read[FACES]
    stats["watertight"] = read[BOUNDARY] == 0 and read[NONMANIFOLD] == 0 and read[INCONSISTENT] == 0 and ne > 0
    return Edges(edge[:ne], face_count[:ne], wind[:ne], offsets, neighbors[:2 * ne], flags[:nv], stats)


def _topology(what, topology, nv, dev):
    if not isinstance(topology, Edges):
        raise RuntimeError(f"{what}: topology must be an Edges")
    offsets, neighbors, flags = topology.offsets, topology.neighbors, topology.vertex_flags
    for name, t, dtype, n in (("offsets", offsets, torch.int32, nv + 1), ("neighbors", neighbors, torch.int32, None), ("vertex_flags", flags, torch.uint8, nv)):
        if not torch.is_tensor(t) or t.dtype != dtype or t.dim() != 1 or (n is not None and t.shape[0] != n):
            raise RuntimeError(f"{what}: topology.{name} must be a [{'2E' if n is None else n}] {str(dtype).split('.')[-1]} tensor")
        if not t.is_cuda:
            raise RuntimeError(f"{what}: topology.{name} is on {t.device} -- HIP kernels only (no CPU fallback)")
        if t.device != dev:
            raise RuntimeError(f"{what}: topology.{name} is on {t.device}, the rows on {dev}")
    return offsets.contiguous(), neighbors.contiguous(), flags.contiguous()


def umbrella(rows, topology):
    """[Nv, k] float32: per vertex and column the mean of the neighbours' values minus the vertex's own -- the float64 sum over the
    neighbours in ascending index from +0.0, divided by the degree, minus double(value), rounded to float32 once; 0 where the degree
    is 0.  The length of its rows on the positions is the roughness smoothing takes out.  Nothing is read."""
    what = "umbrella"
    if not torch.is_tensor(rows) or rows.dim() != 2:
        raise RuntimeError(f"{what}: rows must be an [Nv, k] float32 tensor")
    if not rows.is_cuda:
        raise RuntimeError(f"{what}: rows is on {rows.device} -- HIP kernels only (no CPU fallback)")
    nv, dev = rows.shape[0], rows.device
    rows = _rows(what, "rows", rows, nv, dev)
    offsets, neighbors, _ = _topology(what, topology, nv, dev)
    out = _room(nv, rows.shape[1], dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        _lib.check(lib().gp_mesh_smooth_umbrella(rows, nv, rows.shape[1], offsets, neighbors, neighbors.shape[0], out, _lib.stream_ptr(dev)), "gp_mesh_smooth_umbrella")
    return out[:nv]


def smooth(mesh, iterations=10, method="taubin", lambda_=0.5, mu=-0.53, boundary="fixed", colors=False, attributes=(), topology=None):
    """Smoothed(mesh, attributes, topology, stats): the vertices of `mesh` (a tsdf_ops.Mesh) after `iterations` of smoothing.  One
    step with factor s replaces every vertex p by p + s (m - p), m the mean of its neighbours -- per column in float64: the sum over
    the neighbours in ascending index from +0.0, one IEEE division by the degree, the difference, the product, the sum, one rounding
    to float32 -- all vertices at once (a step never reads what it writes).  method "laplacian": `iterations` steps with lambda_;
    "taubin": per iteration one step with lambda_ and one with mu (2 * iterations launches), the convention and the defaults of
    Open3D's filter_smooth_taubin.  boundary "fixed": the ends of boundary and non-manifold edges keep their bits; "free": none is
    held.  A vertex without neighbours keeps its bits; the faces are the input's.  colors=True and attributes ([Nv, k] float32
    tensors) go through the same steps; otherwise the colours pass through as they are.  iterations=0 returns the input's bytes.
    topology: an Edges of this mesh from an earlier call -- then nothing is read; without it the one read of edges.  Refused with
    GpHipError, worded by the library: lambda_ or mu not finite, iterations outside [0, 10000], an unknown method or boundary.
    Parity with Open3D to the bit is unpinned: Open3D is not a dependency of this project and sums over an unordered_set, whose
    order is not stated; the pinned definition is tests/mesh_smooth_ref.py."""
    what = "smooth"
    why = check_options(method, boundary, iterations, lambda_, mu)
    if why:
        raise _lib.GpHipError(f"{what}: {why} (iterations = {iterations!r}, lambda_ = {lambda_!r}, mu = {mu!r})")
    vertices, faces, tint = mesh
    if not torch.is_tensor(vertices) or vertices.dim() != 2:
        raise RuntimeError(f"{what}: vertices must be an [Nv, 3] float32 tensor")
    nv = vertices.shape[0]
    checked = _faces(what, faces, nv)
    dev = checked.device
    vertices = _rows(what, "vertices", vertices, nv, dev, 3)
    tint = None if tint is None else _rows(what, "colors", tint, nv, dev, 3)
    attributes = tuple(_rows(what, f"attributes[{k}]", a, nv, dev) for k, a in enumerate(attributes))
    if topology is None:
        topology = edges(checked, nv)
    offsets, neighbors, flags = _topology(what, topology, nv, dev)
    pinned = torch.empty(1, dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        st = _lib.stream_ptr(dev)
        held = [None]

        def run(t, count=None):
            k = t.shape[1]
            out = _room(nv, k, dtype=torch.float32, device=dev)
            if held[0] is None or held[0][0] != k:            # (the two buffers of a width, shared by the arrays of that width)
                held[0] = (k, _lib.scratch(lib().gp_mesh_smooth_rows_bytes, nv, k, device=dev))
            _lib.check(lib().gp_mesh_smooth_steps(t, nv, k, offsets, neighbors, neighbors.shape[0], flags, METHODS[method], BOUNDARIES[boundary], iterations,
                                                  float(lambda_), float(mu), held[0][1], out, count, st), "gp_mesh_smooth_steps")
            return out[:nv]

        moved = run(vertices, pinned)
        if colors and tint is not None:
            tint = run(tint)
        followed = tuple(run(a) for a in attributes)
    steps = iterations * (2 if method == "taubin" else 1)
    return Smoothed(Mesh(moved, faces, tint), followed, topology, {"steps": steps, "pinned": pinned})
