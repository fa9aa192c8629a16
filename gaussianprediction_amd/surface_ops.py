"""The exact distance from a point to a mesh surface on the device (csrc/gp_surface.h, csrc/surface_kernels.hip): for every query the
closest point on the nearest triangle -- its squared distance, face, Voronoi region, position and barycentrics -- found on a uniform
grid over the triangles; and the metrics of geometry_ops with no sampling floor on the reference side: surface_distance measures the
samples of each mesh against the OTHER MESH'S SURFACE, so a mesh against itself is 0 up to float32 rounding of the samples.

The result is defined without the grid: the lexicographic minimum over the usable faces of (float64 distance, face number), the
distance of a face being the minimum over its interior candidate and its three edge candidates.  The grid only decides what it costs.
The header states the definition and the proof of the stopping rule in full, tests/surface_ref.py restates the definition in numpy
and the tests pin that, bit for bit.

HIP only: CPU tensors raise."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from . import geometry_ops as G
from .geometry_ops import THRESHOLDS, _Words, _cloud, _mesh, _thresholds, check_cell

GP_SURFACE_ABI_VERSION = 1          # csrc/gp_surface.h
WIDE_CELLS, MAX_WIDE_CELLS = 64, 64
STAT_WORDS, REFUSED_CAPACITY = 12, 1
STAT_NAMES = ("excluded_faces", "excluded_queries", "candidates", "max_ring", "dim_x", "dim_y", "dim_z", "swept", "pairs", "wide", "status")
HEADER = "../gaussianprediction_amd/csrc/gp_surface.h"         # relative to include/: the header is not one of include/ 


def _prototypes():
    i32, i64, f32, P = C.c_int32, C.c_int64, C.c_float, _lib.Ptr
    return {   # name: (restype, argtypes), as csrc/gp_surface.h declares them (tests/test_surface_host.py compares the two)
        "gp_surface_abi_version": (i32, []),
        "gp_surface_scratch_bytes": (i64, [i64, f32]),
        "gp_surface_grid_count": (i32, [P, P, i64, i64, f32, i32, P, P, P]),
        "gp_surface_grid_fill": (i32, [i64, f32, i32, P, P, i64, P]),
        "gp_surface_grid_query": (i32, [P, i64, P, P, i64, f32, P, P, P, P, P, P, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi(HEADER, "gp_surface_abi_version", GP_SURFACE_ABI_VERSION, PROTOTYPES, register=False)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)


class PointSurface(_Words):
    """dist2 [nq] float32, face [nq] int32, region [nq] int32 (0 the interior, 1 .. 3 the edges (a, b), (b, c), (c, a)), closest [nq, 3]
    float32 and bary [nq, 2] float32 on the device; stats: {"excluded_faces", "excluded_queries", "candidates", "max_ring", "dim_x",
    "dim_y", "dim_z", "swept", "pairs", "wide", "status"} -- read when first asked for, the only read of the device that a query makes.
    geometry_ops.interpolate(result, mesh, attributes) carries vertex attributes to the closest points."""
    __slots__ = ("dist2", "face", "region", "closest", "bary")

    def __init__(self, dist2, face, region, closest, bary, words):
        self.dist2, self.face, self.region, self.closest, self.bary = dist2, face, region, closest, bary
        self._words, self._names, self._stats = words, STAT_NAMES, None

    def __iter__(self):
        return iter((self.dist2, self.face, self.region, self.closest, self.bary))


class SurfaceGrid:
    """The grid over the triangles of `mesh` (a tsdf_ops.Mesh, or any (vertices [Nv, 3] float32, faces [Nf, 3] int32, ...)), built once
    and queried often.  cell: the side of a cell, or None for the automatic rule, round(sqrt(usable faces) / 4) cells along the longest axis;
    wide_cells: a face whose box of cells holds more goes to the wide list every query tests first (DESIGN section 31 measured both).
    No result of query depends on either.
    The build makes ONE 16-byte read of the device, between its counting and its filling entry: the number of (cell, face) pairs
    depends on the data, and the pair array is sized by it.  Memory: 52 bytes a face, 4 bytes a pair, 8 bytes a cell the grid may
    choose (an explicit cell: all 2^24, 128 MiB, as NearestGrid)."""

    def __init__(self, mesh, cell=None, *, wide_cells=WIDE_CELLS):
        what = "SurfaceGrid"
        why = check_cell(cell)
        if why:
            raise _lib.GpHipError(f"{what}: {why}")
        wide_cells = int(wide_cells)
        if not 1 <= wide_cells <= MAX_WIDE_CELLS:
            raise _lib.GpHipError(f"{what}: wide_cells must be 1 .. {MAX_WIDE_CELLS} (wide_cells = {wide_cells})")
        self.vertices, self.faces, nv = _mesh(what, mesh)
        self.cell, self.wide_cells = 0.0 if cell is None else float(cell), wide_cells
        dev, nf = self.faces.device, self.faces.shape[0]
        sizes = torch.empty(2, dtype=torch.int64, device=dev)
        with _lib.on_device(dev):
            self._scratch = _lib.scratch(lib().gp_surface_scratch_bytes, nf, self.cell, device=dev)
            st = _lib.stream_ptr(dev)
            _lib.check(lib().gp_surface_grid_count(self.vertices, self.faces, nv, nf, self.cell, wide_cells, self._scratch, sizes, st), "gp_surface_grid_count")
            self.pairs, self.wide = (int(v) for v in sizes.tolist())          # (the one read: 16 bytes)
            self._pairs = torch.empty(max(self.pairs, 1), dtype=torch.int32, device=dev)
            _lib.check(lib().gp_surface_grid_fill(nf, self.cell, wide_cells, self._scratch, self._pairs, self.pairs, st), "gp_surface_grid_fill")

    def query(self, queries):
        """PointSurface(dist2, face, region, closest, bary, stats) of queries [nq, 3] float32: for every query the lexicographic minimum
        over the usable faces of (d, face), d the float64 squared distance to the closest point of the face, rounded once to float32;
        (+inf, -1, 0, NaN, 0) for a query with a non-finite coordinate, or where no face is usable.  Nothing is read."""
        what = "SurfaceGrid.query"
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
            _lib.check(lib().gp_surface_grid_query(queries, nq, self._scratch, self._pairs, self.faces.shape[0], self.cell, dist2, face, region, closest, bary, words,
                                                   _lib.stream_ptr(dev)), "gp_surface_grid_query")
        return PointSurface(dist2, face, region, closest, bary, words)


def point_mesh_distance(queries, mesh, cell=None):
    """SurfaceGrid(mesh, cell).query(queries): the one-shot form (the grid's ONE 16-byte sizing read, then nothing)."""
    return SurfaceGrid(mesh, cell).query(queries)


def surface_distance(mesh_a, mesh_b, n=100000, seed=0, thresholds=THRESHOLDS, cell=None):
    """geometry_ops.mesh_distance with each mesh's n surface samples (seeded as mesh_distance seeds them: `seed`, and seed + 1 mod 2^64
    for mesh_b) measured against the OTHER MESH'S SURFACE, not against its samples: accuracy, completeness and Hausdorff have no
    sampling floor, and a mesh against itself gives 0 up to the float32 rounding of the samples.  The same row dict as mesh_distance,
    plus "surface": True.  The table and the two sampling refusals come in ONE read, after the two 16-byte sizing reads of the grids;
    a mesh without area raises after it."""
    what = "surface_distance"
    t = _thresholds(what, thresholds)
    sa, sb = G.sample_surface(mesh_a, n, seed), G.sample_surface(mesh_b, n, (int(seed) + 1) % 2 ** 64)
    ab = SurfaceGrid(mesh_b, cell).query(sa.points)
    ba = SurfaceGrid(mesh_a, cell).query(sb.points)
    table = G.metrics_table(ab.dist2, ba.dist2, t)
    status = torch.stack([sa._words[G.STATUS], sb._words[G.STATUS]]).to(torch.float64)
    values = torch.cat([table, status]).tolist()                          # (the one read)
    for name, s in (("mesh_a", values[-2]), ("mesh_b", values[-1])):
        if s:
            raise _lib.GpHipError(f"{what}: {name} " + ("has no area to sample" if int(s) == G.REFUSED_EMPTY else f"cannot tell n = {int(n)} samples apart (n exceeds its total weight)"))
    out = G._row(values[:G.COLUMNS], t)
    out["n"] = int(n)
    out["surface"] = True
    return out
