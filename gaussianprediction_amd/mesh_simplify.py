"""Simplification of a triangle mesh on the device (csrc/gp_mesh_simplify.h, csrc/mesh_simplify_kernels.hip): welding of bit-equal
vertices and vertex clustering on a grid.

tsdf_ops' extraction puts the crossing vertices of several lattice edges on one grid point wherever a sample equals iso, and keeps
the zero-area triangles this gives; a mesh fused at 256^3 has close to a million vertices.  weld merges the vertices whose positions
have equal bits (-0.0 as +0.0), simplify the vertices of one grid cell; both contract every cluster to one vertex, carry the faces
over, drop what collapsed or doubled, and renumber in a stated order -- clusters in ascending order of their smallest member,
faces in their old order -- so that two runs give equal bytes and a mesh with nothing to merge comes back unchanged.  The header
states every definition in full, tests/mesh_simplify_ref.py restates them in numpy and the tests pin that.

HIP only: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple

import torch

from . import _lib
from .mesh_ops import _faces, _rows
from .tsdf_ops import Mesh

GP_MESH_SIMPLIFY_ABI_VERSION = 1    # csrc/gp_mesh_simplify.h
WELD, GRID = 0, 1
FIRST, AVERAGE = 0, 1
MAX_DIM = 2 ** 21
STATUS, VERTICES, FACES, CLUSTERS, COLLAPSED, ZERO_AREA, DUPLICATES, COUNT_WORDS = 0, 1, 2, 3, 4, 5, 6, 8
RECORD_WORDS = 8
HEADER = "../gaussianprediction_amd/csrc/gp_mesh_simplify.h"      # relative to include/: the header is not one of include/ 
CONTRACTIONS = {"first": FIRST, "average": AVERAGE}


def _prototypes():
    i32, i64, f64, P = C.c_int32, C.c_int64, C.c_double, _lib.Ptr
    return {   # name: (restype, argtypes), as csrc/gp_mesh_simplify.h declares them (tests/test_mesh_simplify_host.py compares the two)
        "gp_mesh_simplify_abi_version": (i32, []),
        "gp_mesh_simplify_scratch_bytes": (i64, [i64, i64]),
        "gp_mesh_simplify_bounds": (i32, [P, i64, P, P, P]),
        "gp_mesh_simplify_plan": (i32, [P, P, i64, i64, i32, f64, P, i32, i32, i32, i32, P, P, P]),
        "gp_mesh_simplify_apply": (i32, [P, i64, i64, P, P, P, P, P, P, P]),
        "gp_mesh_simplify_rows": (i32, [P, i64, i64, i32, i32, P, P, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi(HEADER, "gp_mesh_simplify_abi_version", GP_MESH_SIMPLIFY_ABI_VERSION, PROTOTYPES, register=False)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)

# mesh: the simplified tsdf_ops.Mesh; vertex_map [Nv]: the new vertex of every old one, -1 where its cluster was dropped; face_index
# [Nf']: the old ids of the kept faces; vertex_counts [Nv']: the members of every new vertex, all int32 on the device; attributes: the
# tensors handed in, contracted like the positions; stats: {"clusters", "collapsed", "zero_area", "duplicates", "unreferenced"}
Simplified = namedtuple("Simplified", "mesh vertex_map face_index vertex_counts attributes stats")


def check_voxel(voxel_size, bounds=None):
    """The library's refusal of a voxel size (and, where given, of the box ((x0, y0, z0), (x1, y1, z1)) with it), as it words it
    (None: accepted)."""
    voxel = float(voxel_size)
    if not math.isfinite(voxel) or not voxel > 0:
        return "voxel_size must be finite and > 0"
    if bounds is None:
        return None
    lo, hi = [float(v) for v in bounds[0]], [float(v) for v in bounds[1]]
    if len(lo) != 3 or len(hi) != 3 or not all(math.isfinite(v) for v in lo + hi) or any(a > b for a, b in zip(lo, hi)):
        return "bounds must be finite with min <= max"
    for a, b in zip(lo, hi):
        origin = a - voxel / 2
        if not math.floor((b + voxel / 2 - origin) / voxel) + 1.0 <= MAX_DIM:
            return "voxel_size is too small"
    return None


def _run(what, mesh, mode, voxel_size, contraction, bounds, drop_zero_area, drop_duplicates, keep_unreferenced, attributes):
    if contraction not in CONTRACTIONS:
        raise _lib.GpHipError(f"{what}: contraction must be \"average\" or \"first\" (contraction = {contraction!r})")
    how = FIRST if mode == WELD else CONTRACTIONS[contraction]
    voxel = 0.0
    if mode == GRID:
        voxel = float(voxel_size)
        why = check_voxel(voxel, bounds)
        if why:
            raise _lib.GpHipError(f"{what}: {why} (voxel_size = {voxel:g})")
    vertices, faces, colors = mesh
    if not torch.is_tensor(vertices) or vertices.dim() != 2:
        raise RuntimeError(f"{what}: vertices must be an [Nv, 3] float32 tensor")
    nv = vertices.shape[0]
    faces = _faces(what, faces, nv)
    nf, dev = faces.shape[0], faces.device
    vertices = _rows(what, "vertices", vertices, nv, dev, 3)
    colors = None if colors is None else _rows(what, "colors", colors, nv, dev, 3)
    attributes = tuple(_rows(what, f"attributes[{k}]", a, nv, dev) for k, a in enumerate(attributes))
    counts = torch.empty(COUNT_WORDS, dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        st = _lib.stream_ptr(dev)
        scratch = _lib.scratch(lib().gp_mesh_simplify_scratch_bytes, nv, nf, device=dev)
        box = (C.c_double * 6)()
        if mode == GRID and bounds is not None:
            box[:] = [float(v) for v in bounds[0]] + [float(v) for v in bounds[1]]
        elif mode == GRID and nv > 0:
            record = torch.empty(RECORD_WORDS, dtype=torch.float64, device=dev)
            _lib.check(lib().gp_mesh_simplify_bounds(vertices, nv, scratch, record, st), "gp_mesh_simplify_bounds")
            found = record.tolist()                           # (the read of the bounds)
            if found[6] != 0:
                raise _lib.GpHipError(f"{what}: a coordinate is not finite")
            box[:] = found[:6]
            why = check_voxel(voxel, (found[:3], found[3:6]))
            if why:
                raise _lib.GpHipError(f"{what}: {why} (voxel_size = {voxel:g})")
        _lib.check(lib().gp_mesh_simplify_plan(vertices, faces, nv, nf, mode, voxel, box, how, int(bool(drop_zero_area)), int(bool(drop_duplicates)),
                                               int(bool(keep_unreferenced)), scratch, counts, st), "gp_mesh_simplify_plan")
        read = [int(v) for v in counts.tolist()]              # (the one read of the counts)
        if read[STATUS]:
            raise _lib.GpHipError(f"{what}: a face index lies outside [0, {nv}), or a vertex outside the bounds (a coordinate that is not finite among them)")
        nv2, nf2 = read[VERTICES], read[FACES]

        def room(n, *shape, dtype):                           # (an empty tensor has no pointer to hand over: one row at the least, cut below)
            return torch.empty(max(n, 1), *shape, dtype=dtype, device=dev)

        vertices_out, faces_out = room(nv2, 3, dtype=torch.float32), room(nf2, 3, dtype=torch.int32)
        vertex_map, face_index, vertex_counts = room(nv, dtype=torch.int32), room(nf2, dtype=torch.int32), room(nv2, dtype=torch.int32)
        if nv > 0:
            _lib.check(lib().gp_mesh_simplify_apply(faces, nv, nf, scratch, vertices_out, faces_out, vertex_map, face_index, vertex_counts, st), "gp_mesh_simplify_apply")
        vertices_out, faces_out, vertex_map, face_index, vertex_counts = vertices_out[:nv2], faces_out[:nf2], vertex_map[:nv], face_index[:nf2], vertex_counts[:nv2]

        def follow(t):
            out = room(nv2, t.shape[1], dtype=torch.float32)
            if nv > 0:
                _lib.check(lib().gp_mesh_simplify_rows(t, nv, nf, t.shape[1], how, scratch, out, st), "gp_mesh_simplify_rows")
            return out[:nv2]

        stats = {"clusters": read[CLUSTERS], "collapsed": read[COLLAPSED], "zero_area": read[ZERO_AREA], "duplicates": read[DUPLICATES],
                 "unreferenced": read[CLUSTERS] - nv2}
        kept = Mesh(vertices_out, faces_out, None if colors is None else follow(colors))
        return Simplified(kept, vertex_map, face_index, vertex_counts, tuple(follow(a) for a in attributes), stats)


def weld(mesh, drop_zero_area=False, drop_duplicates=True, keep_unreferenced=False, attributes=()):
    """Simplified(mesh, vertex_map, face_index, vertex_counts, attributes, stats): `mesh` (a tsdf_ops.Mesh) with the vertices of
    bit-equal positions (-0.0 as +0.0; NaNs of equal bits weld) merged into the one of the smallest index, whose position, colour and
    attribute rows stay as they are.  Faces two of whose corners merged are dropped; with drop_zero_area also those whose face
    vector (b - a) x (c - a) is zero in all three components; with drop_duplicates all but the first of the faces that name the same
    three vertices in the same winding (any rotation).  Unless keep_unreferenced, a vertex no kept face names is dropped and
    vertex_map holds -1 for it.  What stays keeps its order: a mesh with nothing to merge and no unreferenced vertex comes back in
    equal bytes.  One read: the eight counts (with the status word).  A face index outside [0, Nv) raises GpHipError at that read."""
    return _run("weld", mesh, WELD, None, "first", None, drop_zero_area, drop_duplicates, keep_unreferenced, attributes)


def simplify(mesh, voxel_size, contraction="average", bounds=None, drop_zero_area=False, drop_duplicates=True, keep_unreferenced=False, attributes=()):
    """Vertex clustering: the vertices of one cell of a grid of side voxel_size become one vertex -- contraction "average": per column
    the float64 sum over the cell's vertices in ascending index, over their count, rounded to float32 once; "first": the vertex of
    the smallest index -- colours and attribute rows alike; the faces as in weld.  The grid: origin = min - voxel_size / 2, cell =
    floor((p - origin) / voxel_size) in float64; min and max are the exact bounds of the vertices, or `bounds` ((x0, y0, z0), (x1,
    y1, z1)) where given: a sequence that hands in one box shares one grid.  A vertex outside such a box, a coordinate that is not
    finite and a face index outside [0, Nv) raise GpHipError; more than 2^21 cells along an axis are refused ("voxel_size is too
    small").  Two reads: the bounds' record, then the eight counts; one read with `bounds` given.  Returns Simplified as weld does;
    vertex_counts are the vertices of every cell."""
    return _run("simplify", mesh, GRID, voxel_size, contraction, bounds, drop_zero_area, drop_duplicates, keep_unreferenced, attributes)
