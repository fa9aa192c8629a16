#!/usr/bin/env python
"""Time the signed-distance volumes (volume_ops) on the mesh of tools/mesh_probe.py: a 256^3 volume holding a unit sphere seen by 16
views of 800 x 800, extracted (914254 vertices, 1780644 triangles where that probe recorded it).  "Another time step" is that mesh
scaled by 1.02 and moved by 0.01 along x, as in tools/surface_probe.py.

    build              MeshTree beside SurfaceGrid (host clock: the grid's build holds its 16-byte read)
    uniform            10^4 uniform points of the cube around the mesh through MeshTree.query, beside SurfaceGrid.query on the same points
    surface            10^6 surface samples of the other time step's mesh through both
    lattice            SignedTree.lattice at 64^3 and 128^3; 256^3 only where eight times the 128^3 line stays under a minute
    end_to_end         volume_iou and remesh at resolution 128, host clock, reads included
    open_sphere        remesh of the fused sphere itself, which mesh_smooth.edges finds open: its boundary edges before and after

hipEvent windows, medians of 7.  Every step runs as a child process of its own under its own time limit, one after the other; the first
that fails or runs out of time ends the run.  Informative only: no pass/fail threshold comes from here.  Every line says what bounds
it, "supposed" where no counter was read.  Prints one table and writes it to profiles/volume_probe.txt (or to the path given as the
first argument).

    python tools/volume_probe.py
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (("build", 240), ("uniform", 480), ("surface", 240), ("lattice", 480), ("end_to_end", 300), ("open_sphere", 300))      # name, seconds
N_UNIFORM, N_SURFACE = 10 ** 4, 10 ** 6


def step(name, mesh_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import torch
    from mesh_probe import DEV, REPS, event_ms, host_ms, timed
    from gaussianprediction_amd import geometry_ops as G, mesh_smooth as MS, surface_ops as S, volume_ops as V

    def row(text, ms):
        print(f"{text:<190}{ms:>12.3f}", flush=True)

    if name == "build" and not os.path.exists(mesh_path):
        from mesh_clean_probe import sphere_mesh
        full = sphere_mesh(256)
        torch.save((full.vertices.cpu(), full.faces.cpu()), mesh_path)
    vertices, faces = (t.to(DEV) for t in torch.load(mesh_path))
    mesh = (vertices, faces)
    other = ((vertices * 1.02 + torch.tensor([0.01, 0.0, 0.0], device=DEV)).contiguous(), faces)
    nv, nf = vertices.shape[0], faces.shape[0]
    if name == "build":
        print(f"volume probe on {torch.cuda.get_device_name(DEV)}: per call, hipEvent medians of {REPS} after one warm-up unless a line says host clock")
        print(f"{'entry':<190}{'ms':>12}")
        print(f"the mesh: {nv} vertices, {nf} triangles; leaf {V.LEAF}, levels {V.MeshTree(mesh).query(vertices[:1]).stats['levels']}")
        row(f"MeshTree(mesh): the records, one stable radix sort of {nf} 31-bit keys, the gather, one launch a level; no read (host clock); bound by the sort's passes (supposed)",
            timed(lambda: V.MeshTree(mesh), clock=host_ms))
        row("SurfaceGrid(mesh): section 31's build, its 16-byte read included (host clock)", timed(lambda: S.SurfaceGrid(mesh), clock=host_ms))
    elif name == "uniform":
        lo, hi = vertices.amin(dim=0), vertices.amax(dim=0)
        g = torch.Generator(device="cpu").manual_seed(34)
        points = (lo + (hi - lo) * torch.rand(N_UNIFORM, 3, generator=g).to(DEV)).contiguous()
        tree, grid = V.MeshTree(mesh), S.SurfaceGrid(mesh)
        a, b = tree.query(points), grid.query(points)
        same = all(torch.equal(x, y) for x, y in zip(a, b))
        row(f"MeshTree.query: {N_UNIFORM} uniform points of the cube around the mesh; bound by the latency of the dependent box and record loads of divergent lanes (supposed)",
            timed(lambda: tree.query(points)))
        row(f"SurfaceGrid.query on the same points, the same machine, this run (section 31's grid, unchanged): the empty rings (section 31)", timed(lambda: grid.query(points)))
        print(f"  equal bytes: {same}; tree stats {a.stats}; grid stats {b.stats}")
    elif name == "surface":
        samples = G.sample_surface(other, N_SURFACE, seed=1).points
        tree, grid = V.MeshTree(mesh), S.SurfaceGrid(mesh)
        a, b = tree.query(samples), grid.query(samples)
        same = all(torch.equal(x, y) for x, y in zip(a, b))
        row(f"MeshTree.query: {N_SURFACE} surface samples of the other time step's mesh; bound by the float64 candidate tests and the box loads (supposed)", timed(lambda: tree.query(samples)))
        row(f"SurfaceGrid.query on the same samples (section 31: the candidates' float64 tests, supposed there)", timed(lambda: grid.query(samples)))
        print(f"  equal bytes: {same}; tree stats {a.stats}; grid stats {b.stats}")
    elif name == "lattice":
        topology = MS.edges(faces, nv)
        signed = V.SignedTree(mesh, topology)
        took = 0.0
        for n in (64, 128, 256):
            if n == 256 and 8 * took >= 60e3:
                print(f"  256^3 left out: eight times the 128^3 line is {8 * took / 1e3:.1f} s")
                break
            origin, voxel, dims = V.lattice_rule(vertices.amin(dim=0).tolist(), vertices.amax(dim=0).tolist(), None, n)
            took = timed(lambda: signed.lattice(origin, voxel, dims)) if n < 256 else event_ms(lambda: signed.lattice(origin, voxel, dims))          # (256^3: one call)
            volume = signed.lattice(origin, voxel, dims)
            row(f"SignedTree.lattice {dims[0]} x {dims[1]} x {dims[2]}{' (one call)' if n == 256 else ''}: a walk and a sign a point, 4 bytes written; bound by the walks of the points far from "
                "the surface (supposed)", took)
            s = volume.stats
            print(f"  nodes {s['nodes'] / volume.sdf.numel():.1f} and candidates {s['candidates'] / volume.sdf.numel():.1f} a point; max stack {s['max_stack']}; inside {s['inside']}, "
                  f"outside {s['outside']}, undetermined {s['undetermined']}")
    elif name == "end_to_end":
        row("volume_iou(mesh, other, resolution = 128), end to end (host clock): the bounds' read, two trees, two topologies, two tables, two lattices, one read; bound by the lattices (supposed)",
            timed(lambda: V.volume_iou(mesh, other, resolution=128), clock=host_ms))
        print("  " + ", ".join(f"{k} {v}" for k, v in V.volume_iou(mesh, other, resolution=128).items()))
        row("remesh(mesh, resolution = 128), end to end (host clock): the lattice, to_tsdf, marching tetrahedra; bound by the lattice (supposed)", timed(lambda: V.remesh(mesh, resolution=128), clock=host_ms))
    elif name == "open_sphere":
        before = MS.edges(faces, nv).stats
        out = V.remesh(mesh, resolution=128)
        after = MS.edges(out.faces, out.vertices.shape[0]).stats
        print(f"  the fused sphere: {nf} triangles, boundary edges {before['boundary']}, watertight {before['watertight']}")
        print(f"  remesh(resolution = 128): {out.faces.shape[0]} triangles, boundary edges {after['boundary']}, watertight {after['watertight']}, euler {after.get('euler')}"
              " -- a finding, not an assertion: the sign of an open sheet is only the side its normals face")


def main():
    out = next((a for a in sys.argv[1:] if not a.startswith("--")), os.path.join(ROOT, "profiles", "volume_probe.txt"))
    lines = []
    with tempfile.TemporaryDirectory() as d:
        mesh_path = os.path.join(d, "mesh.pt")
        for name, seconds in STEPS:
            try:
                done = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, mesh_path], timeout=seconds, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            except subprocess.TimeoutExpired:
                lines.append(f"step {name}: no result within {seconds} s; the run ends here")
                break
            lines.append(done.stdout.rstrip("\n"))
            print(lines[-1], flush=True)
            if done.returncode != 0:
                lines.append(f"step {name}: exit status {done.returncode}; the run ends here\n{done.stderr[-2000:]}")
                break
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fp:
        fp.write(text)
    print(text if lines and lines[-1].startswith("step ") else "", end="")
    return 1 if lines and "the run ends here" in lines[-1] else 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--step":
        step(sys.argv[2], sys.argv[3])
    else:
        sys.exit(main())
