#!/usr/bin/env python
"""Time the signed distance (sdf_ops) on the mesh of tools/mesh_probe.py: a 256^3 volume holding a unit sphere seen by 16 views of
800 x 800, extracted (914254 vertices, 1780644 triangles where that probe recorded it).  "Another time step" is that mesh scaled by
1.02 and moved by 0.01 along x, as in tools/surface_probe.py.

    the tables         mesh_smooth.edges (what they need, host clock, its read included) and gp_sdf_tables with that topology handed in
    the sign           gp_sdf_sign for 10^6 surface samples of the other time step's mesh, beside the unsigned query it follows
    the means          gp_sdf_means of those 10^6 rows
    end to end         signed_surface_distance against surface_distance at n = 10^5, host clock, reads included

hipEvent windows, medians of 7.  Informative only: no pass/fail threshold comes from here.  Every line says what bounds it, "supposed"
where no counter was read.  Prints one table and writes it to profiles/sdf_probe.txt (or to the path given as the first argument).

    python tools/sdf_probe.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from mesh_clean_probe import sphere_mesh  # noqa: E402
from mesh_probe import DEV, REPS, host_ms, timed  # noqa: E402
from gaussianprediction_amd import geometry_ops as G, mesh_smooth as MS, sdf_ops as D, surface_ops as S  # noqa: E402

N = 10 ** 6


def main():
    lines = [f"sdf probe on {torch.cuda.get_device_name(DEV)}: per call, hipEvent medians of {REPS} after one warm-up",
             f"{'entry':<170}{'ms':>12}"]

    def row(name, ms):
        lines.append(f"{name:<170}{ms:>12.3f}")
        print(lines[-1], flush=True)

    full = sphere_mesh(256)
    mesh = (full.vertices, full.faces)
    other = ((full.vertices * 1.02 + torch.tensor([0.01, 0.0, 0.0], device=DEV)).contiguous(), full.faces)
    nv, nf = mesh[0].shape[0], mesh[1].shape[0]
    topology = MS.edges(mesh[1], nv)
    ne = topology.edge.shape[0]
    lines.append(f"the mesh: {nv} vertices, {nf} triangles, {ne} edges; {topology.stats}")
    row("mesh_smooth.edges(faces, nv): the topology the tables need (host clock, its one read included) -- section 32's", timed(lambda: MS.edges(mesh[1], nv), clock=host_ms))
    row(f"pseudonormals(mesh, topology): gp_sdf_tables -- two stable sorts of {3 * nf} pairs, two walks, {3 * nf} bisections in {ne} edges; bound by the sorts' passes over memory (supposed)",
        timed(lambda: D.pseudonormals(mesh, topology)))
    normals = D.pseudonormals(mesh, topology)
    lines.append(f"  its stats: {dict(normals.stats)}")
    samples = G.sample_surface(other, N, seed=1).points
    grid = S.SurfaceGrid(mesh)
    row(f"SurfaceGrid.query: {N} surface samples of the other time step's mesh, unsigned (section 31's: the candidates' float64 tests, supposed there)", timed(lambda: grid.query(samples)))
    surface = grid.query(samples)
    row(f"gp_sdf_sign for those {N} rows: one face test in float64 and one 24-byte gather a query; bound by the latency of the dependent gathers (face -> indices -> corners -> table; supposed)",
        timed(lambda: D._sign("probe", samples, surface, mesh[0], mesh[1], normals)))
    signed = D._sign("probe", samples, surface, mesh[0], mesh[1], normals)
    lines.append(f"  its stats: {signed.stats}")
    row(f"gp_sdf_means of those {N} rows: four trees a workgroup, one lane adds {-(-N // 256)} partials a word; bound by that one lane's walk (supposed)", timed(lambda: D.means(signed.sdf, signed.sign)))
    n = 10 ** 5
    row(f"signed_surface_distance(mesh, other, n = {n}), end to end (host clock): two grids, two topologies, two tables, two queries, two signs, one read; bound by the grids' builds and queries and the two reads of edges (supposed)", timed(lambda: D.signed_surface_distance(mesh, other, n=n), clock=host_ms))
    row(f"surface_distance(mesh, other, n = {n}), end to end (host clock); bound by the grids' builds and queries (section 31; supposed)", timed(lambda: S.surface_distance(mesh, other, n=n), clock=host_ms))
    on = D.signed_surface_distance(mesh, other, n=n)
    lines.append("  signed_surface_distance: " + ", ".join(f"{k} {on[k]:.6f}" for k in ("accuracy", "completeness", "signed_accuracy", "signed_completeness", "outside_share_a", "outside_share_b"))
                 + f", oriented {on['oriented']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sdf_probe.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fp:
        fp.write(text)


if __name__ == "__main__":
    main()
