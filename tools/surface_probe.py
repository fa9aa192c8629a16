#!/usr/bin/env python
"""Time the point-to-surface distance (surface_ops) on the mesh of tools/mesh_probe.py: a 256^3 volume holding a unit sphere seen by 16
views of 800 x 800, extracted (914254 vertices, 1780644 triangles where that probe recorded it).  "Another time step" is that mesh
scaled by 1.02 and moved by 0.01 along x.

    the build          gp_surface_grid_count, the 16-byte sizing read (host clock) and gp_surface_grid_fill, each apart
    query              10^6 surface samples of the other time step's mesh; 10^6 uniform points of the cube around the mesh (fewer where a
                       10^4 pilot says the full run would take more than CUBE_BUDGET_S, and the row says so)
    the sweep          the cells along the longest axis and W, the wide threshold: build, pairs per face, wide faces, candidates per
                       query, the largest ring, swept, query time -- on this mesh and on the 64^3 one, which the 2^24 cells do not cap
    the brute force    2 * 10^4 queries under the one-cell rule, the same kernel, against the automatic rule; and the same on smaller
                       meshes (8^3 .. 64^3 volumes) to see where the grid overtakes it
    end to end         surface_distance against mesh_distance at n = 10^5, host clock, reads included

hipEvent windows, medians of 7 (3 for the rows marked so).  Informative only: no pass/fail threshold comes from here.  Prints one
table and writes it to profiles/surface_probe.txt.

    python tools/surface_probe.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from mesh_clean_probe import sphere_mesh  # noqa: E402
from mesh_probe import DEV, REPS, event_ms, host_ms, median, timed  # noqa: E402
from gaussianprediction_amd import _lib, geometry_ops as G, surface_ops as S  # noqa: E402

N = 10 ** 6
SMALL = 2 * 10 ** 4
CUBE_BUDGET_S = 5.0
SWEEP_CELLS = (32, 64, 128, 167, 256)          # 167: what round(sqrt(nf) / 4) = 334 halves to on the large mesh; 256: what round(sqrt(nf)) does
SWEEP_WIDE = (8, 27, 64)


def few(fn, reps=3):
    fn()
    return median([event_ms(fn) for _ in range(reps)])


def measure(grid, queries, budget_s=CUBE_BUDGET_S):
    """(queries used, ms, stats): all of `queries`, or the first 10^5 or 10^4 where a 10^4 pilot says a call would take more than budget_s."""
    pilot = few(lambda: grid.query(queries[:10 ** 4].contiguous()), 1)
    n = len(queries)
    while n > 10 ** 4 and pilot * (n / 10 ** 4) / 1000 > budget_s:
        n //= 10
    q = queries[:n].contiguous()
    return n, few(lambda: grid.query(q)), grid.query(q).stats


def build_parts(mesh, cell, wide):
    """(count ms, read ms on the host clock, fill ms) of one build, through the C entries."""
    vertices, faces = mesh
    nv, nf, l, st = vertices.shape[0], faces.shape[0], S.lib(), _lib.stream_ptr(DEV)
    scratch = _lib.scratch(l.gp_surface_scratch_bytes, nf, cell, device=DEV)
    sizes = torch.empty(2, dtype=torch.int64, device=DEV)
    count = lambda: _lib.check(l.gp_surface_grid_count(vertices, faces, nv, nf, cell, wide, scratch, sizes, st), "count")          # noqa: E731
    count_ms = timed(count)
    read_ms = timed(lambda: sizes.tolist(), clock=host_ms)
    pairs = torch.empty(max(int(sizes[0]), 1), dtype=torch.int32, device=DEV)
    fill_ms = timed(lambda: _lib.check(l.gp_surface_grid_fill(nf, cell, wide, scratch, pairs, int(sizes[0]), st), "fill"))
    return count_ms, read_ms, fill_ms


def main():
    lines = [f"surface probe on {torch.cuda.get_device_name(DEV)}: per call, hipEvent medians of {REPS} after one warm-up",
             f"{'entry':<150}{'ms':>12}"]

    def row(name, ms):
        lines.append(f"{name:<150}{ms:>12.3f}")
        print(lines[-1], flush=True)

    full = sphere_mesh(256)
    mesh = (full.vertices, full.faces)
    other = ((full.vertices * 1.02 + torch.tensor([0.01, 0.0, 0.0], device=DEV)).contiguous(), full.faces)
    nv, nf = mesh[0].shape[0], mesh[1].shape[0]
    extent = float((mesh[0].max(dim=0).values - mesh[0].min(dim=0).values).max())
    lines.append(f"the mesh: {nv} vertices, {nf} triangles, extent {extent:.4f}; round(sqrt(nf)) = {round(nf ** 0.5)}, the automatic rule asks round(sqrt(nf) / 4) = {round(nf ** 0.5 / 4)}")
    samples = G.sample_surface(other, N, seed=1).points
    lo, hi = mesh[0].min(dim=0).values - 0.05 * extent, mesh[0].max(dim=0).values + 0.05 * extent
    torch.manual_seed(0)
    cube = (lo + (hi - lo) * torch.rand(N, 3, device=DEV)).contiguous()

    count_ms, read_ms, fill_ms = build_parts(mesh, 0.0, S.WIDE_CELLS)
    row("the build, automatic rule: gp_surface_grid_count", count_ms)
    row("the build, automatic rule: the 16-byte sizing read (host clock)", read_ms)
    row("the build, automatic rule: gp_surface_grid_fill", fill_ms)
    row("SurfaceGrid(mesh), all of it (host clock)", timed(lambda: S.SurfaceGrid(mesh), clock=host_ms))
    grid = S.SurfaceGrid(mesh)
    row(f"query: {N} surface samples of the other time step's mesh", timed(lambda: grid.query(samples)))
    s = grid.query(samples).stats
    lines.append(f"  its stats: {s}; {s['candidates'] / N:.1f} candidates a query, {s['pairs'] / nf:.2f} pairs a face")
    n_cube, ms, s = measure(grid, cube)
    row(f"query: {n_cube} uniform points of the cube around the mesh (of {N}: what a 10^4 pilot allowed in {CUBE_BUDGET_S:g} s a call; medians of 3)", ms)
    lines.append(f"  its stats: {s}; {s['candidates'] / n_cube:.1f} candidates a query")

    lines.append("the sweep: cells along the longest axis (an explicit cell) and W; queries: the 10^6 samples, or the first 10^5 or 10^4 where a pilot says a call would take more than 2 s; medians of 3")
    small = sphere_mesh(64)
    small = (small.vertices, small.faces)
    small_samples = G.sample_surface(((small[0] * 1.02 + torch.tensor([0.01, 0.0, 0.0], device=DEV)).contiguous(), small[1]), N, seed=1).points
    for what, m, queries in ((f"{nf} faces", mesh, samples), (f"{small[1].shape[0]} faces (64^3 volume, round(sqrt(nf)) = {round(small[1].shape[0] ** 0.5)})", small, small_samples)):
        ext = float((m[0].max(dim=0).values - m[0].min(dim=0).values).max())
        for cells in SWEEP_CELLS + (round(m[1].shape[0] ** 0.5),):
            for wide in SWEEP_WIDE:
                cell = ext / cells * (1 + 1e-6)
                build = few(lambda: S.SurfaceGrid(m, cell, wide_cells=wide))
                g = S.SurfaceGrid(m, cell, wide_cells=wide)
                n, ms, s = measure(g, queries, 2.0)
                row(f"{what}, {cells} cells asked, W = {wide}: grid {s['dim_x']} x {s['dim_y']} x {s['dim_z']}, build {build:.3f} ms, {s['pairs'] / m[1].shape[0]:.2f} pairs a face, "
                    f"{s['wide']} wide, {s['candidates'] / n:.1f} candidates a query, ring {s['max_ring']}, swept {s['swept']}; query of {n}", ms)

    lines.append(f"the brute force: {SMALL} queries (samples of the other mesh) under the one-cell rule against the automatic rule; medians of 3")
    for n in (8, 16, 32, 64, 256):
        m = mesh if n == 256 else sphere_mesh(n)
        m = (m[0], m[1]) if n == 256 else (m.vertices, m.faces)
        moved = ((m[0] * 1.02 + torch.tensor([0.01, 0.0, 0.0], device=DEV)).contiguous(), m[1])
        queries = G.sample_surface(moved, SMALL, seed=1).points
        ext = float((m[0].max(dim=0).values - m[0].min(dim=0).values).max())
        one, auto = S.SurfaceGrid(m, 2 * ext), S.SurfaceGrid(m)
        a, b = one.query(queries), auto.query(queries)
        equal = all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))
        row(f"{n}^3 volume, {m[1].shape[0]} faces: one cell, the brute force on the same kernel (equal bits: {equal})", few(lambda: one.query(queries)))
        row(f"{n}^3 volume, {m[1].shape[0]} faces: the automatic rule, grid {b.stats['dim_x']} x {b.stats['dim_y']} x {b.stats['dim_z']}, {b.stats['candidates'] / SMALL:.1f} candidates a query",
            few(lambda: auto.query(queries)))

    n = 10 ** 5
    row(f"surface_distance(mesh, other, n = {n}), end to end (host clock)", timed(lambda: S.surface_distance(mesh, other, n=n), clock=host_ms))
    row(f"mesh_distance(mesh, other, n = {n}), end to end (host clock)", timed(lambda: G.mesh_distance(mesh, other, n=n), clock=host_ms))
    on, off = S.surface_distance(mesh, other, n=n), G.mesh_distance(mesh, other, n=n)
    for name, r in (("surface_distance", on), ("mesh_distance", off)):
        lines.append(f"  {name}: " + ", ".join(f"{k} {r[k]:.6f}" for k in ("accuracy", "completeness", "hausdorff")))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "surface_probe.txt"), "w") as fp:
        fp.write(text)


if __name__ == "__main__":
    main()
