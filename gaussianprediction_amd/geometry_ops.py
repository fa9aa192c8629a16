"""Geometry metrics on the device (csrc/gp_geometry.h, csrc/geometry_kernels.hip): area-weighted, stratified, counter-based samples
of a mesh surface; an exact nearest neighbour on a uniform grid; and accuracy, completeness, Chamfer distance, precision, recall and
F-score at thresholds and the Hausdorff distance of two clouds or two meshes -- the DTU / Tanks-and-Temples protocol -- from ONE
read of a float64 table.

The nearest neighbour is defined without the grid: the lexicographic minimum of (distance, index) with knn_kernels.hip's own
float32 distance, so for finite inputs it equals knn_ops.knn_points(K=1) bit for bit, for every cell size; the grid only decides
what it costs.  The header states every definition in full, tests/geometry_ref.py restates them in numpy and the tests pin that,
bit for bit.

HIP only: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
import json
import math
import os
import re

import torch

from . import _lib
from .mesh_ops import _faces, _rows

GP_GEOMETRY_ABI_VERSION = 1         # csrc/gp_geometry.h
MAX_FACES, MAX_CHANNELS, MAX_AXIS, MAX_CELLS, MAX_THRESHOLDS, WEIGHT_BITS = 2 ** 26, 8, 1024, 2 ** 24, 8, 36
STATUS, BAD_INDEX, NON_FINITE, ZERO_WEIGHT, COUNT_WORDS = 0, 1, 2, 3, 8
REFUSED_EMPTY, REFUSED_TOO_MANY = 1, 2
SAMPLE_STAT_NAMES = ("status", "bad_index", "non_finite", "zero_weight")
STAT_WORDS = 8
STAT_NAMES = ("excluded_points", "excluded_queries", "candidates", "max_ring", "dim_x", "dim_y", "dim_z", "swept")
COLUMNS, PRECISION, RECALL, FSCORE = 37, 13, 21, 29
COLUMN_NAMES = ("count_ab", "sum_ab", "sum2_ab", "max_ab", "count_ba", "sum_ba", "sum2_ba", "max_ba", "accuracy", "completeness", "chamfer_l1", "chamfer_l2", "hausdorff")
THRESHOLDS = (0.01, 0.02, 0.05)
HEADER = "../gaussianprediction_amd/csrc/gp_geometry.h"        # relative to include/: the header is not one of include/ 


def _prototypes():
    i32, i64, u64, f32, P = C.c_int32, C.c_int64, C.c_uint64, C.c_float, _lib.Ptr
    return {   # name: (restype, argtypes), as csrc/gp_geometry.h declares them (tests/test_geometry_host.py compares the two)
        "gp_geometry_abi_version": (i32, []),
        "gp_geometry_sample_scratch_bytes": (i64, [i64]),
        "gp_geometry_grid_scratch_bytes": (i64, [i64, f32]),
        "gp_geometry_metrics_scratch_bytes": (i64, [i64, i64]),
        "gp_geometry_sample": (i32, [P, P, i64, i64, i64, u64, P, P, P, P, P, P]),
        "gp_geometry_interpolate": (i32, [P, i32, P, i64, i64, P, P, i64, P, P]),
        "gp_geometry_grid_build": (i32, [P, i64, f32, P, P]),
        "gp_geometry_grid_query": (i32, [P, i64, P, i64, f32, P, P, P, P]),
        "gp_geometry_metrics": (i32, [P, i64, P, i64, P, i32, P, P, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi(HEADER, "gp_geometry_abi_version", GP_GEOMETRY_ABI_VERSION, PROTOTYPES, register=False)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)


class _Words:
    """Device words as a dict, read when first asked for and never otherwise."""
    __slots__ = ("_words", "_names", "_stats")

    @property
    def stats(self):
        if self._stats is None:
            self._stats = dict(zip(self._names, (int(v) for v in self._words.tolist())))          # (the one read)
        return self._stats


class SurfaceSamples(_Words):
    """points [n, 3] float32, face [n] int32, bary [n, 2] float32 on the device.  stats: {"status", "bad_index", "non_finite",
    "zero_weight"} -- the ONE read of the device, made when stats is first asked for and never otherwise.  status != 0: the mesh was
    refused on the device (1: no area at all; 2: more samples than its integer weights can tell apart) and every point is NaN, every
    face -1."""
    __slots__ = ("points", "face", "bary")

    def __init__(self, points, face, bary, words):
        self.points, self.face, self.bary = points, face, bary
        self._words, self._names, self._stats = words, SAMPLE_STAT_NAMES, None

    def __iter__(self):
        return iter((self.points, self.face, self.bary))


class Nearest(_Words):
    """dist2 [nq] float32, index [nq] int32 on the device; stats: {"excluded_points", "excluded_queries", "candidates", "max_ring",
    "dim_x", "dim_y", "dim_z", "swept"} -- read when first asked for, the only read of the device."""
    __slots__ = ("dist2", "index")

    def __init__(self, dist2, index, words):
        self.dist2, self.index = dist2, index
        self._words, self._names, self._stats = words, STAT_NAMES, None

    def __iter__(self):
        return iter((self.dist2, self.index))


def check_cell(cell):
    """The library's refusal of a cell size, as it words it (None: accepted)."""
    c = 0.0 if cell is None else float(cell)
    if not (math.isfinite(c) and c >= 0):
        return "cell must be finite and >= 0 (0: the automatic rule)"
    return None


def check_thresholds(thresholds):
    t = [float(v) for v in thresholds]
    if len(t) > MAX_THRESHOLDS:
        return f"nt must be 0 .. {MAX_THRESHOLDS}"
    if any(v != v for v in t):
        return "a threshold is NaN"
    return None


def _mesh(what, mesh):
    vertices, faces = mesh[0], mesh[1]
    if not torch.is_tensor(vertices) or vertices.dim() != 2:
        raise RuntimeError(f"{what}: vertices must be an [Nv, 3] float32 tensor")
    nv = vertices.shape[0]
    faces = _faces(what, faces, nv)
    if faces.shape[0] >= MAX_FACES:
        raise _lib.GpHipError(f"{what}: nf must be below 2^26 (nf = {faces.shape[0]})")
    return _rows(what, "vertices", vertices, nv, faces.device, 3), faces, nv


def _cloud(what, name, t, device=None):
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3:
        raise RuntimeError(f"{what}: {name} must be an [N, 3] float32 tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{what}: {name} is on {t.device} -- HIP kernels only (no CPU fallback)")
    if device is not None and t.device != device:
        raise RuntimeError(f"{what}: {name} is on {t.device}, the points on {device}")
    if t.shape[0] >= 2 ** 31 - 1:
        raise _lib.GpHipError(f"{what}: {name} must hold fewer than 2^31 - 1 rows")
    return t.detach().contiguous()


def sample_surface(mesh, n, seed=0):
    """SurfaceSamples of `mesh` (a tsdf_ops.Mesh, or any (vertices [Nv, 3] float32, faces [Nf, 3] int32, ...)): n points, area-weighted
    (integer weights from float64 areas), stratified (sample i falls in the i-th of n equal parts of the total weight) and
    counter-based (splitmix64 of (seed, i, k)): the bytes depend on the arguments alone.  A face with an index out of range or a
    non-finite corner has no weight and is counted.  Nothing is read: a mesh without area is refused on the device, see
    SurfaceSamples.stats."""
    what = "sample_surface"
    n, seed = int(n), int(seed)
    if not 1 <= n < 2 ** 31:
        raise _lib.GpHipError(f"{what}: n must be 1 .. 2^31 - 1 (n = {n})")
    if not 0 <= seed < 2 ** 64:
        raise _lib.GpHipError(f"{what}: seed must be 0 .. 2^64 - 1")
    vertices, faces, nv = _mesh(what, mesh)
    dev, nf = faces.device, faces.shape[0]
    points = torch.empty(n, 3, dtype=torch.float32, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    bary = torch.empty(n, 2, dtype=torch.float32, device=dev)
    words = torch.empty(COUNT_WORDS, dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        scratch = _lib.scratch(lib().gp_geometry_sample_scratch_bytes, nf, device=dev)
        _lib.check(lib().gp_geometry_sample(vertices, faces, nv, nf, n, seed, scratch, points, face, bary, words, _lib.stream_ptr(dev)), "gp_geometry_sample")
    return SurfaceSamples(points, face, bary, words)


def interpolate(samples, mesh, attributes):
    """[n, C] float32: the rows of attributes [Nv, C] float32, 1 <= C <= 8, at the samples, through the weights the points were made
    with: ((B - A) * u1 + A) + (C - A) * u2 over the corners of every sample's face."""
    what = "interpolate"
    if not all(torch.is_tensor(getattr(samples, k, None)) for k in ("face", "bary")):
        raise RuntimeError(f"{what}: samples must be a SurfaceSamples (of sample_surface) or a surface_ops.PointSurface")
    vertices, faces, nv = _mesh(what, mesh)
    dev = faces.device
    attributes = _rows(what, "attributes", attributes, nv, dev)
    k = attributes.shape[1]
    if not 1 <= k <= MAX_CHANNELS:
        raise _lib.GpHipError(f"{what}: C must be 1 .. {MAX_CHANNELS} (C = {k})")
    n = samples.face.shape[0]
    out = torch.empty(n, k, dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        _lib.check(lib().gp_geometry_interpolate(attributes, k, faces, nv, faces.shape[0], samples.face.contiguous(), samples.bary.contiguous(), n, out,
                                                 _lib.stream_ptr(dev)), "gp_geometry_interpolate")
    return out


class NearestGrid:
    """The grid of `points` [np, 3] float32, built once (seven launches and three clears, nothing read) and queried often.  cell: the side of a cell, or
    None for the automatic rule, round(1.5 * cbrt(np)) cells along the longest axis.  No result of query depends on it.  Memory: the
    automatic rule takes about 43 bytes a point of scratch; an explicit cell takes 128 MiB more whatever the cloud (the starts of all
    2^24 cells the device may choose, cleared and scanned by the build), so cloud_distance(..., cell=...) holds that twice."""

    def __init__(self, points, cell=None):
        what = "NearestGrid"
        why = check_cell(cell)
        if why:
            raise _lib.GpHipError(f"{what}: {why}")
        self.points = _cloud(what, "points", points)
        self.cell = 0.0 if cell is None else float(cell)
        dev, n = self.points.device, self.points.shape[0]
        with _lib.on_device(dev):
            self._scratch = _lib.scratch(lib().gp_geometry_grid_scratch_bytes, n, self.cell, device=dev)
            _lib.check(lib().gp_geometry_grid_build(self.points, n, self.cell, self._scratch, _lib.stream_ptr(dev)), "gp_geometry_grid_build")

    def query(self, queries):
        """Nearest(dist2 [nq], index [nq], stats) of queries [nq, 3] float32: for every query the lexicographic minimum over the points
        with finite coordinates of (d, index), d = ((dx*dx + dy*dy) + dz*dz) in float32; (+inf, -1) for a query with a non-finite
        coordinate, or where no point is usable.  Nothing is read."""
        what = "NearestGrid.query"
        dev = self.points.device
        queries = _cloud(what, "queries", queries, dev)
        nq = queries.shape[0]
        dist2 = torch.empty(nq, dtype=torch.float32, device=dev)
        index = torch.empty(nq, dtype=torch.int32, device=dev)
        words = torch.empty(STAT_WORDS, dtype=torch.int64, device=dev)
        with _lib.on_device(dev):
            _lib.check(lib().gp_geometry_grid_query(queries, nq, self._scratch, self.points.shape[0], self.cell, dist2, index, words, _lib.stream_ptr(dev)),
                       "gp_geometry_grid_query")
        return Nearest(dist2, index, words)


def nearest(queries, points, cell=None):
    """NearestGrid(points, cell).query(queries): equal to knn_ops.knn_points(queries, points, K=1) bit for bit where everything is finite."""
    return NearestGrid(points, cell).query(queries)


def _thresholds(what, thresholds):
    t = [float(v) for v in thresholds]
    why = check_thresholds(t)
    if why:
        raise _lib.GpHipError(f"{what}: {why}")
    return t


def metrics_table(dist2_ab, dist2_ba, thresholds=THRESHOLDS):
    """[37] float64 on the device, gp_geometry.h's table, of the squared distances of a's points to b (dist2_ab) and of b's to a."""
    what = "metrics_table"
    t = _thresholds(what, thresholds)
    for name, d in (("dist2_ab", dist2_ab), ("dist2_ba", dist2_ba)):
        if not torch.is_tensor(d) or d.dtype != torch.float32 or d.dim() != 1:
            raise RuntimeError(f"{what}: {name} must be an [n] float32 tensor")
        if not d.is_cuda or d.device != dist2_ab.device:
            raise RuntimeError(f"{what}: {name} is on {d.device} -- HIP kernels only (no CPU fallback)")
    dev = dist2_ab.device
    dist2_ab, dist2_ba = dist2_ab.detach().contiguous(), dist2_ba.detach().contiguous()
    table = torch.empty(COLUMNS, dtype=torch.float64, device=dev)
    with _lib.on_device(dev):
        scratch = _lib.scratch(lib().gp_geometry_metrics_scratch_bytes, dist2_ab.shape[0], dist2_ba.shape[0], device=dev)
        _lib.check(lib().gp_geometry_metrics(dist2_ab, dist2_ab.shape[0], dist2_ba, dist2_ba.shape[0], (C.c_float * max(len(t), 1))(*t), len(t), scratch, table,
                                             _lib.stream_ptr(dev)), "gp_geometry_metrics")
    return table


def _row(values, thresholds):
    out = dict(zip(COLUMN_NAMES, values[:len(COLUMN_NAMES)]))
    out["count_ab"], out["count_ba"] = int(out["count_ab"]), int(out["count_ba"])
    out["thresholds"] = [float(t) for t in thresholds]
    for name, at in (("precision", PRECISION), ("recall", RECALL), ("fscore", FSCORE)):
        out[name] = [values[at + k] for k in range(len(thresholds))]
    return out


def cloud_distance(a, b, thresholds=THRESHOLDS, cell=None):
    """The distances of cloud a [na, 3] (the prediction) and cloud b [nb, 3] (the ground truth), a dict from ONE read of the float64
    table: accuracy = mean distance a -> b, completeness = mean b -> a, chamfer_l1 = their mean, chamfer_l2 = the sum of the two mean
    SQUARED distances, hausdorff = the largest distance of either direction, and per threshold precision (the share of a within it of
    b), recall (of b within it of a) and fscore = 2pr / (p + r), 0 where p + r = 0; the totals count_ab, sum_ab, ... beside them.
    Points with non-finite coordinates count in neither direction."""
    what = "cloud_distance"
    t = _thresholds(what, thresholds)
    a = _cloud(what, "a", a)
    b = _cloud(what, "b", b, a.device)
    ab = NearestGrid(b, cell).query(a)
    ba = NearestGrid(a, cell).query(b)
    return _row(metrics_table(ab.dist2, ba.dist2, t).tolist(), t)          # (the one read)


def mesh_distance(mesh_a, mesh_b, n=100000, seed=0, thresholds=THRESHOLDS, cell=None, surface=False):
    """cloud_distance of n surface samples of each mesh (sample_surface with `seed`, and seed + 1 mod 2^64 for mesh_b, so that a mesh against
    itself is not sample against the same sample).  ONE read: the table and the two sampling refusals together; a mesh without area
    raises after it.  surface=True: surface_ops.surface_distance instead -- the same samples against the other mesh's surface.
    surface="signed": sdf_ops.signed_surface_distance -- that row, plus the sign of every sample against the other mesh."""
    what = "mesh_distance"
    if isinstance(surface, str):
        if surface != "signed":
            raise RuntimeError(f"{what}: surface must be False, True or \"signed\"")
        from .sdf_ops import signed_surface_distance
        return signed_surface_distance(mesh_a, mesh_b, n=n, seed=seed, thresholds=thresholds, cell=cell)
    if surface:
        from .surface_ops import surface_distance
        return surface_distance(mesh_a, mesh_b, n=n, seed=seed, thresholds=thresholds, cell=cell)
    t = _thresholds(what, thresholds)
    sa, sb = sample_surface(mesh_a, n, seed), sample_surface(mesh_b, n, (int(seed) + 1) % 2 ** 64)
    ab = NearestGrid(sb.points, cell).query(sa.points)
    ba = NearestGrid(sa.points, cell).query(sb.points)
    table = metrics_table(ab.dist2, ba.dist2, t)
    status = torch.stack([sa._words[STATUS], sb._words[STATUS]]).to(torch.float64)
    values = torch.cat([table, status]).tolist()                          # (the one read)
    for name, s in (("mesh_a", values[-2]), ("mesh_b", values[-1])):
        if s:
            raise _lib.GpHipError(f"{what}: {name} " + ("has no area to sample" if int(s) == REFUSED_EMPTY else f"cannot tell n = {int(n)} samples apart (n exceeds its total weight)"))
    out = _row(values[:COLUMNS], t)
    out["n"] = int(n)
    return out


def mean_row(rows):
    """The mean of rows of cloud_distance, column by column (lists element by element; NaN where a row has one)."""
    if not rows:
        return {}
    out = {}
    for k, v in rows[0].items():
        if k in ("thresholds", "n", "name", "surface", "signed"):
            out[k] = v
        elif k == "oriented":
            out[k] = all(r[k] for r in rows)
        elif isinstance(v, list):
            out[k] = [sum(r[k][j] for r in rows) / len(rows) for j in range(len(v))]
        else:
            out[k] = sum(r[k] for r in rows) / len(rows)
    out.pop("name", None)
    return out


def evaluate_mesh_dirs(pred_dir, gt_dir, n=100000, thresholds=THRESHOLDS, seed=0, device="cuda", surface=False):
    """Pairs the %05d.ply files of two folders by name (io_formats.read_mesh_ply), one mesh_distance(pred, gt) per pair: returns
    {"rows": [one dict per pair, with its "name"], "mean": their mean, "pairs": how many} and writes it as mesh_metrics.json beside
    pred_dir.  A name only one folder has is left out and listed under "unpaired".  surface=True: every pair through
    mesh_distance(..., surface=True); surface="signed": through mesh_distance(..., surface="signed"), the signed columns with them
    ("oriented" of the mean: every pair is)."""
    from .io_formats import read_mesh_ply
    what = "evaluate_mesh_dirs"
    names = [sorted(f for f in os.listdir(d) if re.fullmatch(r"\d{5}\.ply", f)) for d in (pred_dir, gt_dir)]
    both = [f for f in names[0] if f in set(names[1])]
    if not both:
        raise RuntimeError(f"{what}: no %05d.ply name is in both {pred_dir} and {gt_dir}")

    def load(path):
        vertices, faces = read_mesh_ply(path)[:2]
        return torch.as_tensor(vertices, dtype=torch.float32).to(device), torch.as_tensor(faces, dtype=torch.int32).to(device)

    rows = []
    for f in both:
        row = mesh_distance(load(os.path.join(pred_dir, f)), load(os.path.join(gt_dir, f)), n=n, seed=seed, thresholds=thresholds, surface=surface)
        row["name"] = f
        rows.append(row)
    out = {"rows": rows, "mean": mean_row(rows), "pairs": len(rows), "unpaired": sorted(set(names[0]) ^ set(names[1]))}
    with open(os.path.join(os.path.dirname(os.path.abspath(pred_dir).rstrip(os.sep)), "mesh_metrics.json"), "w") as fp:
        json.dump(out, fp, indent=1)
    return out
