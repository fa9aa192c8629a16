"""Cleanup of a triangle mesh on the device (csrc/gp_mesh.h, csrc/mesh_kernels.hip): connected components, removal of small
components ("floaters"), area-weighted vertex normals.

tsdf_ops ends at the extracted mesh.  A mesh fused from a trained scene carries one small closed shell per stray blob that two views
agree on, and no normals.  connected_components labels every vertex with the smallest vertex index of its component (two triangles
that share only a vertex are connected), filter_components keeps the components asked for and renumbers what is left in its old
order, vertex_normals sums the face vectors of every vertex in a fixed order; clean does the three in a row.  Everything is integers
or float32 in a stated order of operations: two runs give equal bytes.  The header states every definition in full,
tests/mesh_ref.py restates them in numpy and the tests pin that.

HIP only: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import torch

from . import _lib
from .tsdf_ops import Mesh

GP_MESH_ABI_VERSION = 1             # csrc/gp_mesh.h
TILE, HOPS, MAX_ROUNDS = 1024, 4, 64
STATUS, CONVERGED, COUNT, ROUNDS, STATE_WORDS = 0, 1, 2, 3, 4
ROUNDS_PER_READ = 12                # the rounds enqueued before the state is read
HEADER = "../gaussianprediction_amd/csrc/gp_mesh.h"      # relative to include/: the header is not one of include/ 


def _prototypes():
    i32, i64, P = C.c_int32, C.c_int64, _lib.Ptr
    return {   # name: (restype, argtypes), as csrc/gp_mesh.h declares them (tests/test_mesh_host.py compares the two)
        "gp_mesh_abi_version": (i32, []),
        "gp_mesh_scratch_bytes": (i64, [i64, i64]),
        "gp_mesh_components": (i32, [P, i64, i64, i32, i32, P, P, P, P, P, P]),
        "gp_mesh_filter_plan": (i32, [P, i64, i64, P, P, P, i64, i32, i32, P, P, P]),
        "gp_mesh_filter_apply": (i32, [P, i64, i64, P, P, P, P, P]),
        "gp_mesh_gather_rows": (i32, [P, i64, i32, P, P, P]),
        "gp_mesh_vertex_normals": (i32, [P, P, i64, i64, P, P, P, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi(HEADER, "gp_mesh_abi_version", GP_MESH_ABI_VERSION, PROTOTYPES, register=False)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)

# vertex_label [Nv], face_label [Nf], and the table in ascending label: labels, vertex_counts, face_counts [C], all int32 on the
# device; rounds: how many hook / jump / settle rounds ran (a Python int)
Components = namedtuple("Components", "vertex_label face_label labels vertex_counts face_counts rounds")
# mesh: the kept part; vertex_index [Nv'], face_index [Nf']: the old ids, int32; attributes: the tensors handed in, following the vertices
Filtered = namedtuple("Filtered", "mesh vertex_index face_index attributes")


def check_sizes(n_vertices, n_faces):
    """The library's refusal of the sizes, as it words it (None: accepted)."""
    nv, nf = int(n_vertices), int(n_faces)
    if nv < 0 or nf < 0:
        return "nv and nf must be >= 0"
    if nv >= 2 ** 31:
        return "nv must be below 2^31"
    if 3 * nf >= 2 ** 31:
        return "3*nf must be below 2^31"
    return None


def _faces(what, faces, n_vertices):
    if not torch.is_tensor(faces) or faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError(f"{what}: faces must be an [Nf, 3] int32 tensor")
    if not faces.is_cuda:
        raise RuntimeError(f"{what}: faces is on {faces.device} -- HIP kernels only (no CPU fallback)")
    why = check_sizes(n_vertices, faces.shape[0])
    if why:
        raise _lib.GpHipError(f"{what}: {why} (nv = {int(n_vertices)}, nf = {faces.shape[0]})")
    return faces.detach().contiguous()


def _rows(what, name, t, n, device, k=None):
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != n or (k is not None and t.shape[1] != k):
        raise RuntimeError(f"{what}: {name} must be a [{n}, {'k' if k is None else k}] float32 tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{what}: {name} is on {t.device} -- HIP kernels only (no CPU fallback)")
    if t.device != device:
        raise RuntimeError(f"{what}: {name} is on {t.device}, the faces on {device}")
    if not 1 <= t.shape[1] <= 1024:
        raise _lib.GpHipError(f"{what}: {name} must have 1 .. 1024 columns")
    return t.detach().contiguous()


def _count(what, name, v):
    if v is None:
        return -1
    v = int(v)
    if not 0 <= v < 2 ** 31:
        raise _lib.GpHipError(f"{what}: {name} must be 0 .. 2^31 - 1 ({name} = {v})")
    return v


def connected_components(faces, n_vertices, rounds_per_read=ROUNDS_PER_READ):
    """Components of the graph whose nodes are the vertices 0 .. n_vertices - 1, with an edge between any two indices of one face
    (triangles sharing only a vertex are connected; this is not Open3D's edge adjacency).  vertex_label: the smallest vertex index of
    the vertex's component; face_label: vertex_label[faces[f, 0]]; labels, vertex_counts, face_counts: the table in ascending label
    (views of one [3, Nv] tensor).  A vertex no face names is a component of its own with face count 0; degenerate faces are ordinary.

    Rounds and reads: a round is three launches (hook by atomicMin, jump up to 4 pointers, settle); `rounds_per_read` of them (12) are
    enqueued at once, a round behind a converged one returns at once, then the table is built and FOUR words are read -- status,
    converged, C, rounds: one read per 12 rounds.  DESIGN section 27's mesh of 0.9 M vertices converged in 3 rounds (one read), a
    path of 4098 vertices under a seeded numbering in 5, against a cap of 4 ceil(log2 Nv) + 8.  The result does not depend on
    rounds_per_read; an enqueued round costs about 0.2 ms there whether it works or not, so a smaller value trades reads for time.
    A face index outside [0, n_vertices) raises GpHipError at that read."""
    what = "connected_components"
    faces = _faces(what, faces, n_vertices)
    nv, nf, dev = int(n_vertices), faces.shape[0], faces.device
    per = int(rounds_per_read)
    if not 1 <= per <= MAX_ROUNDS:
        raise _lib.GpHipError(f"{what}: rounds_per_read must be 1 .. {MAX_ROUNDS} (rounds_per_read = {per})")
    vertex_label = torch.empty(nv, dtype=torch.int32, device=dev)
    face_label = torch.empty(nf, dtype=torch.int32, device=dev)
    table = torch.empty(3, nv, dtype=torch.int32, device=dev)
    state = torch.empty(STATE_WORDS, dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        scratch = _lib.scratch(lib().gp_mesh_scratch_bytes, nv, nf, device=dev)
        first = 1
        while True:
            _lib.check(lib().gp_mesh_components(faces, nv, nf, per, first, vertex_label, face_label, table, scratch, state, _lib.stream_ptr(dev)),
                       "gp_mesh_components")
            status, converged, count, rounds = (int(v) for v in state.tolist())          # (the read of this batch)
            if status:
                raise _lib.GpHipError(f"{what}: a face index lies outside [0, {nv})")
            if converged:
                break
            first = 0
    return Components(vertex_label, face_label, table[0, :count], table[1, :count], table[2, :count], rounds)


def filter_components(mesh, min_triangles=None, keep_largest=None, components=None, attributes=()):
    """Filtered(mesh, vertex_index, face_index, attributes): the part of `mesh` (a tsdf_ops.Mesh) whose components have at least one
    face, at least min_triangles faces where given, and are among the keep_largest components with the most faces where given (ties
    to the smaller label).  With neither, only unreferenced vertices leave.  Kept vertices and faces stay in ascending old index (an
    ordered compaction: ballot ranks and tile scans, no atomics: two runs give equal bytes and a closed surface stays closed), the
    faces are renumbered; mesh.colors and every [Nv, k] float32 tensor of `attributes` follow the vertices.  vertex_index and
    face_index are the old ids, int32.  One read: the two new sizes (with the status word); where `components` (the Components of
    this mesh) is not given, the reads of connected_components come first."""
    what = "filter_components"
    vertices, faces, colors = mesh
    if not torch.is_tensor(vertices) or vertices.dim() != 2:
        raise RuntimeError(f"{what}: vertices must be an [Nv, 3] float32 tensor")
    nv = vertices.shape[0]
    faces = _faces(what, faces, nv)
    nf, dev = faces.shape[0], faces.device
    vertices = _rows(what, "vertices", vertices, nv, dev, 3)
    colors = None if colors is None else _rows(what, "colors", colors, nv, dev, 3)
    attributes = tuple(_rows(what, f"attributes[{k}]", a, nv, dev) for k, a in enumerate(attributes))
    min_triangles, keep_largest = _count(what, "min_triangles", min_triangles), _count(what, "keep_largest", keep_largest)
    if components is None:
        components = connected_components(faces, nv)
    ncomp = components.labels.shape[0]
    if components.vertex_label.shape[0] != nv or components.vertex_label.device != dev or ncomp > nv:
        raise RuntimeError(f"{what}: components are not those of this mesh")
    counts = torch.empty(3, dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        st = _lib.stream_ptr(dev)
        scratch = _lib.scratch(lib().gp_mesh_scratch_bytes, nv, nf, device=dev)
        _lib.check(lib().gp_mesh_filter_plan(faces, nv, nf, components.vertex_label.contiguous(), components.labels.contiguous(),
                                             components.face_counts.contiguous(), ncomp, min_triangles, keep_largest, scratch, counts, st), "gp_mesh_filter_plan")
        status, nv2, nf2 = (int(v) for v in counts.tolist())          # (the one read)
        if status:
            raise _lib.GpHipError(f"{what}: a face index or a label lies outside [0, {nv})")
        vertex_index = torch.empty(nv2, dtype=torch.int32, device=dev)
        face_index = torch.empty(nf2, dtype=torch.int32, device=dev)
        faces_out = torch.empty(nf2, 3, dtype=torch.int32, device=dev)
        if nv2 > 0:                                       # (a kept vertex lies in a kept component, which has a face: nf2 > 0 as well)
            _lib.check(lib().gp_mesh_filter_apply(faces, nv, nf, scratch, vertex_index, face_index, faces_out, st), "gp_mesh_filter_apply")

        def follow(t):
            out = torch.empty(nv2, t.shape[1], dtype=torch.float32, device=dev)
            if nv2 > 0:
                _lib.check(lib().gp_mesh_gather_rows(t, nv, t.shape[1], scratch, out, st), "gp_mesh_gather_rows")
            return out

        kept = Mesh(follow(vertices), faces_out, None if colors is None else follow(colors))
        return Filtered(kept, vertex_index, face_index, tuple(follow(a) for a in attributes))


def vertex_normals(vertices, faces, state=None):
    """[Nv, 3] float32: per vertex the sum of the face vectors (b - a) x (c - a) of its incidences -- area-weighted, pointing out of
    the surface with the winding of TsdfVolume.extract -- added one after the other in ascending 3 f + corner, divided by its length
    sqrtf((x*x + y*y) + z*z) where that is finite and > 0, else (0, 0, 0), never NaN.  The lists come from a stable radix sort of
    (vertex, 3 f + corner) pairs, no float atomics: the result is the same to the bit in every run.  Faces with an index outside
    [0, Nv) contribute nothing (and raise word 0 of `state`, a [4] int32 tensor, where one is handed in).  Nothing is read."""
    what = "vertex_normals"
    if not torch.is_tensor(vertices) or vertices.dim() != 2:
        raise RuntimeError(f"{what}: vertices must be an [Nv, 3] float32 tensor")
    nv = vertices.shape[0]
    faces = _faces(what, faces, nv)
    nf, dev = faces.shape[0], faces.device
    vertices = _rows(what, "vertices", vertices, nv, dev, 3)
    normals = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        scratch = _lib.scratch(lib().gp_mesh_scratch_bytes, nv, nf, device=dev)
        _lib.check(lib().gp_mesh_vertex_normals(vertices, faces, nv, nf, scratch, normals, state, _lib.stream_ptr(dev)), "gp_mesh_vertex_normals")
    return normals


def clean(mesh, min_triangles=None, keep_largest=None, normals=False):
    """connected_components, filter_components and (normals=True) vertex_normals of what is left: the filtered Mesh, or (Mesh,
    normals).  Reads: those of connected_components (one, as a rule) and the one of filter_components."""
    filtered = filter_components(mesh, min_triangles=min_triangles, keep_largest=keep_largest)
    if not normals:
        return filtered.mesh
    return filtered.mesh, vertex_normals(filtered.mesh.vertices, filtered.mesh.faces)
