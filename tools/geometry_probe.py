#!/usr/bin/env python
"""Time the geometry metrics (geometry_ops) on the mesh of tools/mesh_probe.py: a 256^3 volume holding a unit sphere seen by 16 views
of 800 x 800, extracted (914254 vertices, 1780644 triangles where that probe recorded it).

    sample_surface     10^6 samples of that mesh: areas, weights, the 64-bit scan, the binary searches
    the grid build     NearestGrid of those samples: bounds, the record, counts, scan, scatter
    query              10^6 other samples of the same mesh against it
    metrics            gp_geometry_metrics on the two dist2 arrays
    query against knn_ops.knn_points(K=1), the brute force, on the same inputs at 2 * 10^5 x 2 * 10^5
    query with R, the cells along the longest axis, at 1/4, 1/2, 1, 1.25, 1.5, 2 and 2.5 times cbrt(np), on a surface cloud (those
    samples) and on a volume cloud (10^6 uniform points of a cube, queried by 10^6 others), with the candidates per query, the
    largest ring and the queries that ended with the pass over all records

hipEvent windows, medians.  Informative only: no pass/fail threshold comes from here.  Prints one table and writes it to
profiles/geometry_probe.txt.

    python tools/geometry_probe.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from mesh_clean_probe import sphere_mesh  # noqa: E402
from mesh_probe import DEV, REPS, event_ms, median, timed  # noqa: E402
from gaussianprediction_amd import geometry_ops as G, knn_ops  # noqa: E402

N = 10 ** 6
SMALL = 2 * 10 ** 5
FACTORS = (0.25, 0.5, 1.0, 1.25, 1.5, 2.0, 2.5)          # (2.5 x 100 cells cubed is the most the 2^24 cells allow at 10^6 points)


def main():
    lines = [f"geometry probe on {torch.cuda.get_device_name(DEV)}: per call, hipEvent medians of {REPS} after one warm-up",
             f"{'entry':<118}{'ms':>10}"]

    def row(name, ms):
        lines.append(f"{name:<118}{ms:>10.3f}")

    mesh = sphere_mesh(256)
    mesh = (mesh.vertices, mesh.faces)
    nv, nf = mesh[0].shape[0], mesh[1].shape[0]
    lines.append(f"the mesh: {nv} vertices, {nf} triangles")
    row(f"sample_surface(mesh, {N})", timed(lambda: G.sample_surface(mesh, N)))
    a, b = G.sample_surface(mesh, N, seed=0), G.sample_surface(mesh, N, seed=1)
    lines.append(f"  its counts: {a.stats}")
    row(f"NearestGrid of {N} samples (the build)", timed(lambda: G.NearestGrid(a.points)))
    grid = G.NearestGrid(a.points)
    row(f"query: {N} other samples against it", timed(lambda: grid.query(b.points)))
    ab, ba = grid.query(b.points), G.NearestGrid(b.points).query(a.points)
    lines.append(f"  its stats: {ab.stats}")
    row(f"metrics_table of the two dist2 arrays ({N} each)", timed(lambda: G.metrics_table(ab.dist2, ba.dist2)))
    lines.append("  cloud_distance of the two sample sets: " + ", ".join(f"{k} {v:.6f}" for k, v in G.cloud_distance(a.points, b.points).items() if k in ("accuracy", "completeness", "hausdorff")))

    p, q = a.points[:SMALL].contiguous(), b.points[:SMALL].contiguous()
    small = G.NearestGrid(p)
    build_ms = timed(lambda: G.NearestGrid(p))
    query_ms = timed(lambda: small.query(q))
    knn = lambda: knn_ops.knn_points(q[None], p[None], K=1)          # noqa: E731
    knn()
    knn_ms = median([event_ms(knn) for _ in range(3)])
    d, i = knn()
    got = small.query(q)
    equal = bool(torch.equal(got.dist2, d.reshape(-1)) and torch.equal(got.index.long(), i.reshape(-1)))
    row(f"{SMALL} x {SMALL} surface samples: the grid build", build_ms)
    row(f"{SMALL} x {SMALL} surface samples: query", query_ms)
    row(f"{SMALL} x {SMALL} surface samples: knn_ops.knn_points(K=1), the brute force (equal bits: {equal})", knn_ms)

    torch.manual_seed(0)
    volume_p, volume_q = torch.rand(N, 3, device=DEV), torch.rand(N, 3, device=DEV)
    for what, points, queries in (("surface", a.points, b.points), ("volume", volume_p, volume_q)):
        extent = float((points.max(dim=0).values - points.min(dim=0).values).max())
        for factor in FACTORS:
            cell = extent / max(1, round(factor * round(N ** (1 / 3))))
            build = timed(lambda: G.NearestGrid(points, cell))
            g = G.NearestGrid(points, cell)
            ms = timed(lambda: g.query(queries))
            s = g.query(queries).stats
            row(f"{what} cloud, {N} x {N}, R = {factor:g} x cbrt(np): grid {s['dim_x']} x {s['dim_y']} x {s['dim_z']}, build {build:.3f} ms, "
                f"{s['candidates'] / N:.1f} candidates a query, largest ring {s['max_ring']}, swept {s['swept']}; query", ms)
        g = G.NearestGrid(points)
        s = g.query(queries).stats
        row(f"{what} cloud, {N} x {N}, the automatic rule: grid {s['dim_x']} x {s['dim_y']} x {s['dim_z']}, build {timed(lambda: G.NearestGrid(points)):.3f} ms; query", timed(lambda: g.query(queries)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "geometry_probe.txt"), "w") as fp:
        fp.write(text)


if __name__ == "__main__":
    main()
