#!/usr/bin/env python
"""Time the mesh topology and the smoothing (mesh_smooth) on the mesh of tools/mesh_probe.py: a 256^3 volume holding a unit sphere
seen by 16 views of 800 x 800, extracted (914254 vertices, 1780644 triangles where that probe recorded it):

    edges        gp_mesh_smooth_edges_plan and gp_mesh_smooth_edges_apply alone (hipEvent), and edges() as a whole with its read
                 (host clock around a synchronise); the counts and the degree histogram of that mesh
    smooth       ten Taubin iterations (twenty launches) of the positions alone (hipEvent), one step alone with the bytes it moves
                 at the least, and smooth() as a whole with topology= (host clock); the roughness and the volume before and after
    numpy        the same two in the vectorised forms of tests/mesh_smooth_ref.py on the host, once each, with the bytes compared

with the copy peak recorded in profiles/ for scale.  Informative only: no pass/fail threshold comes from here.  Prints one table and
writes it to profiles/mesh_smooth_probe.txt.

    python tools/mesh_smooth_probe.py
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mesh_smooth_ref as ref  # noqa: E402
from mesh_clean_probe import sphere_mesh  # noqa: E402
from mesh_probe import DEV, REPS, host_ms, recorded_copy_peak, timed  # noqa: E402
from gaussianprediction_amd import _lib, mesh_smooth as MT  # noqa: E402


def main():
    copy_peak, where = recorded_copy_peak()
    lines = [f"mesh topology and smoothing probe on {torch.cuda.get_device_name(DEV)}: hipEvent medians of {REPS} after one warm-up unless a host clock is named",
             f"copy peak (read + written bytes): {copy_peak:.0f} GB/s, {where}",
             f"{'entry':<112}{'ms':>10}{'MB moved':>12}{'GB/s':>10}{'of peak':>9}"]

    def row(name, ms, nbytes=0):
        rate = nbytes / (ms * 1e-3) / 1e9 if nbytes else 0.0
        lines.append(f"{name:<112}{ms:>10.3f}" + (f"{nbytes / 1e6:>12.1f}{rate:>10.1f}{100 * rate / copy_peak:>8.1f}%" if nbytes else ""))

    mesh = sphere_mesh(256)
    nv, nf = mesh.vertices.shape[0], mesh.faces.shape[0]
    l, st = MT.lib(), _lib.stream_ptr(DEV)
    scratch = _lib.scratch(l.gp_mesh_smooth_scratch_bytes, nv, nf, device=DEV)
    lines.append(f"the mesh: {nv} vertices, {nf} triangles; scratch {scratch.numel() / 1e6:.1f} MB = {scratch.numel() / max(nf, 1):.1f} bytes per face")
    counts = torch.empty(MT.COUNT_WORDS, dtype=torch.int32, device=DEV)
    bits = max(1, nv.bit_length())
    passes = 2 * ((bits + 7) // 8)
    plan = lambda: _lib.check(l.gp_mesh_smooth_edges_plan(mesh.faces, nv, nf, scratch, counts, st), "plan")      # noqa: E731
    row(f"gp_mesh_smooth_edges_plan: {6 * nf} directed entries, {passes} sort passes of (key, value) words, heads, two compactions", timed(plan),
        6 * nf * 16 * passes)                                # (a pass reads and writes a key and a value at the least)
    ne = int(counts.tolist()[MT.EDGES])
    i32 = dict(dtype=torch.int32, device=DEV)
    out = [torch.empty(ne, 2, **i32), torch.empty(ne, **i32), torch.empty(ne, **i32), torch.empty(nv + 1, **i32), torch.empty(2 * ne, **i32), torch.empty(nv, dtype=torch.uint8, device=DEV)]
    apply = lambda: _lib.check(l.gp_mesh_smooth_edges_apply(nv, nf, ne, scratch, *out, st), "apply")      # noqa: E731
    row("gp_mesh_smooth_edges_apply: the heads write edges and neighbours, offsets by bisection, flags", timed(apply), 6 * nf * 14 + ne * 16 + 2 * ne * 8 + nv * 7)
    row("edges() as a whole: scratch, plan, the read of eight words, apply (host clock)", timed(lambda: MT.edges(mesh.faces, nv), host_ms))
    del scratch
    topo = MT.edges(mesh.faces, nv)
    degree = torch.diff(topo.offsets).cpu().numpy()
    lines.append("  counts: " + ", ".join(f"{k} {v}" for k, v in topo.stats.items()))
    lines.append("  degree histogram: " + ", ".join(f"{d}: {n}" for d, n in enumerate(np.bincount(degree)) if n))

    k, n2 = 3, 2 * ne
    rows_scratch = _lib.scratch(l.gp_mesh_smooth_rows_bytes, nv, k, device=DEV)
    dst = torch.empty(nv, k, device=DEV)

    def steps(iterations, method):
        return lambda: _lib.check(l.gp_mesh_smooth_steps(mesh.vertices, nv, k, topo.offsets, topo.neighbors, n2, topo.vertex_flags, method, MT.FIXED, iterations, 0.5, -0.53, rows_scratch, dst,
                                                         None, st), "steps")

    step_bytes = nv * (8 + 1) + n2 * 4 + (n2 + 2 * nv) * 4 * k          # offsets, flags, neighbours; every neighbour's row once, the vertex's own read and written
    row("gp_mesh_smooth_steps, one Laplacian step of the positions (the neighbours' rows counted as read once each)", timed(steps(1, MT.LAPLACIAN)), step_bytes)
    row("gp_mesh_smooth_steps, ten Taubin iterations of the positions: twenty launches", timed(steps(10, MT.TAUBIN)), 20 * step_bytes)
    row("smooth(10, taubin, topology=) as a whole: the positions, no read (host clock)", timed(lambda: MT.smooth(mesh, 10, topology=topo), host_ms))
    row("smooth(10, taubin) without topology=: edges() first, one read (host clock)", timed(lambda: MT.smooth(mesh, 10), host_ms))
    row("gp_mesh_smooth_umbrella of the positions", timed(lambda: MT.umbrella(mesh.vertices, topo)), step_bytes)
    smoothed = MT.smooth(mesh, 10, topology=topo)
    length = lambda m: float(MT.umbrella(m.vertices, topo).double().norm(dim=1).mean())      # noqa: E731
    f = mesh.faces.cpu().numpy()
    lines.append(f"  mean umbrella length before {length(mesh):.3e}, after {length(smoothed.mesh):.3e}; enclosed volume before "
                 f"{ref.enclosed_volume(mesh.vertices.cpu().numpy(), f):.6f}, after {ref.enclosed_volume(smoothed.mesh.vertices.cpu().numpy(), f):.6f} (the unit sphere: {4 * np.pi / 3:.6f})")

    # ---- beside the vectorised numpy restatement, the same mesh ----
    v = mesh.vertices.cpu().numpy()
    start = time.perf_counter()
    want = ref.edges_vectorised(f, nv)
    row("  edges in numpy (tests/mesh_smooth_ref.py edges_vectorised), host, once", (time.perf_counter() - start) * 1e3)
    start = time.perf_counter()
    moved = ref.smooth(v, want, 10, "taubin", one_step=ref.step_vectorised)
    row("  ten Taubin iterations in numpy (step_vectorised), host, once", (time.perf_counter() - start) * 1e3)
    got = [t.cpu().numpy() for t in (topo.edge, topo.face_count, topo.wind, topo.offsets, topo.neighbors, topo.vertex_flags)]
    equal = all(g.tobytes() == w.tobytes() for g, w in zip(got, ref.parts(want))) and topo.stats == want.stats and smoothed.mesh.vertices.cpu().numpy().tobytes() == moved.tobytes()
    lines.append(f"the device's topology and smoothed positions of that mesh and the restatement's: {'equal bytes' if equal else 'DIFFERENT'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mesh_smooth_probe.txt"), "w") as fp:
        fp.write(text)


if __name__ == "__main__":
    main()
