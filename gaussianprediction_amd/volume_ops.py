"""Signed-distance volumes on the device (csrc/gp_volume.h, csrc/volume_kernels.hip): a bounding-volume tree over the triangles of a
mesh that answers surface_ops' exact closest-point query ANYWHERE in space -- the uniform grid pays for every empty ring between a
query and the surface, the tree skips empty space a box at a time --, the signed distance of a mesh on the lattice of a
tsdf_ops.TsdfVolume, a volumetric IoU between two meshes, and remesh, which makes a closed surface from that lattice with the
marching tetrahedra that are already there.

The result of a query is defined without the tree: gp_surface.h's lexicographic minimum over the usable faces of (float64 distance,
face number), computed with the same functions.  MeshTree.query gives the bytes SurfaceGrid.query gives, SignedTree.query the bytes
SignedGrid.query gives; the tree only decides what it costs.  The header states the skipping rule and its proof in full,
tests/volume_ref.py restates the definitions in numpy and the tests pin that, bit for bit.

HIP only: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
import math
import struct

import torch

from . import _lib
from . import mesh_smooth as MS
from . import sdf_ops as D
from . import tsdf_ops as T
from .geometry_ops import _Words, _cloud, _mesh
from .surface_ops import PointSurface

GP_VOLUME_ABI_VERSION = 1         # csrc/gp_volume.h
LEAF, STACK = 2, 32
STAT_WORDS, LATTICE_WORDS, COUNT_WORDS = 8, 16, 6
STAT_NAMES = ("excluded_faces", "excluded_queries", "nodes", "candidates", "max_stack", "levels", "leaves", "status")
LATTICE_NAMES = STAT_NAMES + ("face", "edge", "vertex", "inside", "outside", "undetermined", "excluded", "sign_status")
COUNT_NAMES = ("inside_a", "inside_b", "both", "either", "undetermined", "points")
HEADER = "../gaussianprediction_amd/csrc/gp_volume.h"          # relative to include/: the header is not one of include/ 


def _prototypes():
    i32, i64, f32, P = C.c_int32, C.c_int64, C.c_float, _lib.Ptr
    return {   # name: (restype, argtypes), as csrc/gp_volume.h declares them (tests/test_volume_host.py compares the two)
        "gp_volume_abi_version": (i32, []),
        "gp_volume_tree_scratch_bytes": (i64, [i64]),
        "gp_volume_tree": (i32, [P, P, i64, i64, P, P]),
        "gp_volume_query": (i32, [P, i64, P, i64, P, P, P, P, P, P, P]),
        "gp_volume_lattice": (i32, [P, P, P, i64, i64, P, P, i64, P, f32, f32, f32, f32, i32, i32, i32, P, P, P]),
        "gp_volume_compare": (i32, [P, P, i64, P, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi(HEADER, "gp_volume_abi_version", GP_VOLUME_ABI_VERSION, PROTOTYPES, register=False)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)


def _f32(x):
    return struct.unpack("<f", struct.pack("<f", float(x)))[0]


# ---- refusals that need no device, as the library words them (None: accepted) ----
def check_lattice(origin, voxel, dims):
    vals = [float(v) for v in origin] + [float(voxel)]
    if not all(abs(v) < float("inf") for v in vals):
        return "origin and voxel must be finite"
    if not vals[3] > 0:
        return "voxel must be > 0"
    nx, ny, nz = (int(v) for v in dims)
    if nx < 1 or ny < 1 or nz < 1:
        return "nx, ny and nz must be >= 1"
    if nx * ny * nz >= 2 ** 31:
        return "nx*ny*nz must be below 2^31"
    return None


class MeshTree:
    """A bounding-volume tree over the triangles of `mesh` (a tsdf_ops.Mesh, or any (vertices [Nv, 3] float32, faces [Nf, 3] int32,
    ...)), built once and queried often: the records sorted along a 30-bit Morton curve of their boxes' centres by one stable radix
    sort, two consecutive records a leaf, the boxes level by level above them.  Every size is a function of the number of faces: the
    build reads nothing.  Memory: 96 bytes a face for the records in both orders, 32 bytes a face for the boxes, 16 for the sort."""

    def __init__(self, mesh):
        what = "MeshTree"
        self.vertices, self.faces, nv = _mesh(what, mesh)
        dev, nf = self.faces.device, self.faces.shape[0]
        with _lib.on_device(dev):
            self._scratch = _lib.scratch(lib().gp_volume_tree_scratch_bytes, nf, device=dev)
            _lib.check(lib().gp_volume_tree(self.vertices, self.faces, nv, nf, self._scratch, _lib.stream_ptr(dev)), "gp_volume_tree")

    def query(self, queries):
        """surface_ops.PointSurface(dist2, face, region, closest, bary, stats) of queries [nq, 3] float32, byte-equal to
        SurfaceGrid(mesh).query(queries) for every input: the lexicographic minimum over the usable faces of (d, face).  A lane walks
        the tree with a stack, the nearer child first, and skips a box only where every face in it is strictly farther than the best
        so far (csrc/gp_volume.h has the proof).  stats: {"excluded_faces", "excluded_queries", "nodes" (boxes tested), "candidates"
        (records tested), "max_stack", "levels", "leaves", "status"} -- read when first asked for, the only read.  Nothing is read."""
        what = "MeshTree.query"
        dev = self.faces.device
        queries = _cloud(what, "queries", queries, dev)
        nq = queries.shape[0]
        dist2 = torch.empty(nq, dtype=torch.float32, device=dev)
        face = torch.empty(nq, dtype=torch.int32, device=dev)
        region = torch.empty(nq, dtype=torch.int32, device=dev)
        closest = torch.empty(nq, 3, dtype=torch.float32, device=dev)
        bary = torch.empty(nq, 2, dtype=torch.float32, device=dev)
        words = torch.empty(STAT_WORDS, dtype=torch.int64, device=dev)
        with _lib.on_device(dev):
            _lib.check(lib().gp_volume_query(queries, nq, self._scratch, self.faces.shape[0], dist2, face, region, closest, bary, words, _lib.stream_ptr(dev)),
                       "gp_volume_query")
        out = PointSurface(dist2, face, region, closest, bary, words)
        out._names = STAT_NAMES
        return out


class SdfVolume(_Words):
    """The signed distance of a mesh on a lattice: sdf [nz, ny, nx] float32 on the device (negative inside a watertight mesh wound
    outward; +inf where the mesh has no usable face), origin (three floats), voxel_size, dims = (nx, ny, nz): point (i, j, k) lies at
    fma(i, voxel_size, origin) in float32, the lattice of a tsdf_ops.TsdfVolume of the same origin, voxel_size and dims.  stats: the
    walk's words and the sign's ({"nodes", "candidates", "max_stack", "levels", "leaves", "status", "face", "edge", "vertex", "inside",
    "outside", "undetermined", "excluded", "sign_status", ...}) -- read when first asked for, the only read."""
    __slots__ = ("sdf", "origin", "voxel_size", "dims")

    def __init__(self, sdf, origin, voxel_size, dims, words):
        self.sdf, self.origin, self.voxel_size, self.dims = sdf, tuple(origin), float(voxel_size), tuple(dims)
        self._words, self._names, self._stats = words, LATTICE_NAMES, None

    def inside(self):
        """[nz, ny, nx] bool on the device: sdf < 0.  Nothing is read."""
        return self.sdf < 0

    def to_tsdf(self, trunc=None):
        """A colourless tsdf_ops.TsdfVolume on the same lattice: tsdf = clamp(sdf / trunc, -1, 1) in float32 (trunc: 4 * voxel_size by
        default), weight 1 where sdf is finite and 0 elsewhere.  Its extract() is the surface sdf = 0.  Nothing is read."""
        volume = T.TsdfVolume(self.origin, self.voxel_size, self.dims, trunc=trunc, color=False, device=self.sdf.device)
        # the float32 quotient, rounded once: a float64 division of two float32 values rounded again to float32 is the correctly rounded
        # float32 division (53 >= 2 * 24 + 2 bits), and a tensor divisor keeps torch from multiplying by a reciprocal instead
        trunc = torch.full((), _f32(volume.trunc), dtype=torch.float64, device=self.sdf.device)
        volume.tsdf = torch.clamp((self.sdf.to(torch.float64) / trunc).to(torch.float32), -1.0, 1.0).contiguous()
        volume.weight = torch.isfinite(self.sdf).to(torch.float32).contiguous()
        return volume


class SignedTree:
    """A MeshTree over `mesh` and the sdf_ops.Pseudonormals of the same mesh.  topology: the mesh_smooth.Edges of this mesh from an
    earlier call; without it the one read of mesh_smooth.edges -- the only read of the build.  .tree, .normals."""

    def __init__(self, mesh, topology=None):
        self.tree = MeshTree(mesh)
        self.normals = D.pseudonormals((self.tree.vertices, self.tree.faces), topology)

    def query(self, queries):
        """sdf_ops.SignedSurface(sdf, sign, kind, element, surface, stats) of queries [nq, 3] float32, byte-equal to
        SignedGrid(mesh).query(queries): the tree's closest point, then sdf_ops' sign pass on it.  Nothing is read."""
        what = "SignedTree.query"
        tree = self.tree
        queries = _cloud(what, "queries", queries, tree.faces.device)
        return D._sign(what, queries, tree.query(queries), tree.vertices, tree.faces, self.normals)

    def contains(self, queries):
        """[nq] bool on the device: query(queries).sign < 0 -- sdf_ops.contains' answer and its caveats (it means "inside" only on a
        watertight mesh wound outward), at the tree's cost: a query deep inside is no slower than one near the surface.  Nothing is
        read."""
        return self.query(queries).sign < 0

    def lattice(self, origin, voxel_size, dims):
        """SdfVolume of the lattice origin + (i, j, k) * voxel_size, dims = (nx, ny, nz) points: a lane per point computes the point
        (one float32 fma a coordinate, as a TsdfVolume's), walks the tree and signs the float32-rounded result as query does; 4 bytes
        are written a point, no query tensor and no PointSurface is made.  Equal to query() on the materialised points.  Nothing is
        read."""
        what = "SignedTree.lattice"
        origin, dims = [_f32(v) for v in origin], [int(v) for v in dims]
        if len(origin) != 3 or len(dims) != 3:
            raise RuntimeError(f"{what}: origin and dims must hold three numbers each")
        voxel = _f32(voxel_size)
        why = check_lattice(origin, voxel, dims)
        if why:
            raise _lib.GpHipError(f"{what}: {why} (origin = {origin}, voxel_size = {voxel}, dims = {dims})")
        tree, normals = self.tree, self.normals
        dev, nv, nf, ne = tree.faces.device, tree.vertices.shape[0], tree.faces.shape[0], normals.edge_normal.shape[0]
        nx, ny, nz = dims
        sdf = torch.empty(nz, ny, nx, dtype=torch.float32, device=dev)
        words = torch.empty(LATTICE_WORDS, dtype=torch.int64, device=dev)
        with _lib.on_device(dev):
            _lib.check(lib().gp_volume_lattice(tree._scratch, tree.vertices, tree.faces, nv, nf, normals.face_edges, normals.edge_normal, ne, normals.vertex_normal,
                                               origin[0], origin[1], origin[2], voxel, nx, ny, nz, sdf, words, _lib.stream_ptr(dev)), "gp_volume_lattice")
        return SdfVolume(sdf, origin, voxel, dims, words)


def lattice_rule(lo, hi, voxel_size=None, resolution=128, margin=2):
    """lattice_for's rule on the bounds lo, hi (three floats each): see there.  No device."""
    what = "lattice_for"
    resolution, margin = int(resolution), int(margin)
    if margin < 0:
        raise _lib.GpHipError(f"{what}: margin must be >= 0 (margin = {margin})")
    lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    if not all(abs(v) < float("inf") for v in lo + hi):
        raise _lib.GpHipError(f"{what}: the meshes have no vertex with finite coordinates")
    ext = [h - l for l, h in zip(lo, hi)]
    if voxel_size is None:
        cells = resolution - 2 * margin - 2
        if cells < 1:
            raise _lib.GpHipError(f"{what}: resolution must be above 2 * margin + 2 (resolution = {resolution}, margin = {margin})")
        voxel = _f32(max(ext) / cells)
        if not voxel > 0:
            raise _lib.GpHipError(f"{what}: the meshes have no extent: pass voxel_size")
    else:
        voxel = _f32(voxel_size)
        if not 0 < voxel < float("inf"):
            raise _lib.GpHipError(f"{what}: voxel_size must be finite and > 0 (voxel_size = {voxel_size})")
    origin = tuple(_f32(l - (margin + 0.5) * voxel) for l in lo)
    dims = tuple(int(math.ceil(e / voxel)) + 2 * margin + 2 for e in ext)
    why = check_lattice(origin, voxel, dims)
    if why:
        raise _lib.GpHipError(f"{what}: {why} (origin = {origin}, voxel_size = {voxel}, dims = {dims})")
    return origin, voxel, dims


def lattice_for(meshes, voxel_size=None, resolution=128, margin=2):
    """(origin, voxel_size, dims) of a lattice around `meshes` (one mesh or a list of them).  The rule, with lo and hi the bounds of
    all vertices with finite coordinates and E the largest of hi - lo, in float64 unless said otherwise:
        voxel_size = float32(voxel_size), or float32(E / (resolution - 2 * margin - 2)) where none is given;
        origin_k = float32(lo_k - (margin + 0.5) * voxel_size);      dims_k = ceil((hi_k - lo_k) / voxel_size) + 2 * margin + 2
    -- the lattice reaches `margin` and a half voxels beyond the bounds on every side, the longest axis holds `resolution` points (one
    more where the division rounds up), and no lattice plane coincides with a face of the bounding box: an axis-aligned surface does
    not fall on lattice points, where its distance would be 0 and its sign undetermined.  ONE read of 24 bytes (the bounds)."""
    what = "lattice_for"
    if isinstance(meshes, (list, tuple)) and len(meshes) and isinstance(meshes[0], (list, tuple)):
        meshes = list(meshes)
    else:
        meshes = [meshes]
    parts = [_mesh(what, m)[0] for m in meshes]
    dev = parts[0].device
    if any(p.device != dev for p in parts):
        raise RuntimeError(f"{what}: the meshes are on different devices")
    v = torch.cat(parts)
    ok = torch.isfinite(v).all(dim=1, keepdim=True)
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=dev)
    lo = torch.where(ok, v, inf).amin(dim=0) if v.shape[0] else inf.expand(3)
    hi = torch.where(ok, v, -inf).amax(dim=0) if v.shape[0] else (-inf).expand(3)
    bounds = torch.cat([lo, hi]).tolist()                                 # (the one read: 24 bytes)
    return lattice_rule(bounds[:3], bounds[3:], voxel_size, resolution, margin)


def sdf_volume(mesh, voxel_size=None, resolution=128, margin=2, origin=None, dims=None):
    """SdfVolume of `mesh` on the lattice lattice_for(mesh, voxel_size, resolution, margin) chooses, or on (origin, voxel_size, dims)
    where origin and dims are given (then voxel_size must be too, and the 24-byte read is not made).  The other read: mesh_smooth.edges'."""
    what = "sdf_volume"
    if (origin is None) != (dims is None):
        raise _lib.GpHipError(f"{what}: origin and dims go together (both or neither)")
    if origin is not None and voxel_size is None:
        raise _lib.GpHipError(f"{what}: origin and dims need a voxel_size")
    _mesh(what, mesh)
    if origin is None:
        origin, voxel_size, dims = lattice_for(mesh, voxel_size, resolution, margin)
    return SignedTree(mesh).lattice(origin, voxel_size, dims)


def compare(sdf_a, sdf_b):
    """[6] int64 on the device: how many points are inside a (a finite value < 0), inside b, inside both, inside either, undetermined
    (a value that is not finite in either volume: such a point counts in none of the four), and the number of points.  Integers only:
    equal bytes from two runs.  Nothing is read."""
    what = "compare"
    for name, t in (("sdf_a", sdf_a), ("sdf_b", sdf_b)):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise RuntimeError(f"{what}: {name} must be a float32 tensor")
        if not t.is_cuda or t.device != sdf_a.device:
            raise RuntimeError(f"{what}: {name} is on {t.device} -- HIP kernels only (no CPU fallback)")
    if sdf_a.shape != sdf_b.shape:
        raise RuntimeError(f"{what}: sdf_a and sdf_b must have the same shape")
    n = sdf_a.numel()
    if n >= 2 ** 31:
        raise _lib.GpHipError(f"{what}: the volumes must hold fewer than 2^31 points")
    dev = sdf_a.device
    a, b = sdf_a.detach().contiguous(), sdf_b.detach().contiguous()
    counts = torch.empty(COUNT_WORDS, dtype=torch.int64, device=dev)
    with _lib.on_device(dev):
        _lib.check(lib().gp_volume_compare(a if n else None, b if n else None, n, counts, _lib.stream_ptr(dev)), "gp_volume_compare")
    return counts


def volume_iou(mesh_a, mesh_b, voxel_size=None, resolution=128):
    """The volumetric IoU of two meshes: both signed on ONE lattice around their joint bounds (lattice_for([mesh_a, mesh_b], ...)),
    the points inside each counted in integers.  {"iou" (intersection / union of the counts; NaN where no point is inside either),
    "volume_a", "volume_b", "intersection", "union" (counts times voxel_size^3), "undetermined" (points without a finite distance in
    either volume, counted nowhere else), "points", "voxel_size", "oriented" (both meshes are watertight and wound outward, as
    sdf_ops.signed_surface_distance defines it: only then "inside" means inside)}.  A point ON a surface is not inside.
    The reads: one of 24 bytes for the bounds, the two of mesh_smooth.edges for the topologies, then ONE for the counts and the
    tables' words."""
    what = "volume_iou"
    _mesh(what, mesh_a), _mesh(what, mesh_b)
    origin, voxel, dims = lattice_for([mesh_a, mesh_b], voxel_size, resolution)
    ta, tb = SignedTree(mesh_a), SignedTree(mesh_b)
    counts = compare(ta.lattice(origin, voxel, dims).sdf, tb.lattice(origin, voxel, dims).sdf)
    pending = [t.normals.stats._pending for t in (ta, tb)]
    values = torch.cat([counts.to(torch.float64)] + [torch.cat([p[0], p[1].to(torch.float64)]) for p in pending]).tolist()          # (the one read)
    tables = [values[COUNT_WORDS + k * (1 + D.COUNT_WORDS):COUNT_WORDS + (k + 1) * (1 + D.COUNT_WORDS)] for k in range(2)]
    for name, t in (("mesh_a", tables[0]), ("mesh_b", tables[1])):
        if int(t[1]):
            raise _lib.GpHipError(f"{what}: {name}: a face index lies outside the vertices")
    inside_a, inside_b, both, either, undetermined, points = (int(v) for v in values[:COUNT_WORDS])
    cell = voxel ** 3
    return {"iou": both / either if either else float("nan"), "volume_a": inside_a * cell, "volume_b": inside_b * cell, "intersection": both * cell, "union": either * cell,
            "undetermined": undetermined, "points": points, "voxel_size": voxel,
            "oriented": all(bool(t.normals.topology.stats["watertight"]) for t in (ta, tb)) and all(t[0] > 0 for t in tables)}


def remesh(mesh, voxel_size=None, resolution=128, trunc=None):
    """sdf_volume(mesh, voxel_size, resolution).to_tsdf(trunc).extract(): a tsdf_ops.Mesh of the surface sdf = 0 by the marching
    tetrahedra of tsdf_ops -- closed wherever the sign of the lattice is that of a solid, with triangles no larger than a cell.  On a
    watertight mesh wound outward the result is watertight and wound outward, within a cell's diagonal of the input; on an open sheet
    the sign is only the side the normals face and the result closes around that half space up to the lattice's rim.  The reads:
    lattice_for's, mesh_smooth.edges' and extract's."""
    return sdf_volume(mesh, voxel_size, resolution).to_tsdf(trunc).extract()
