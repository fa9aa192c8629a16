#!/usr/bin/env python
"""Time the mesh simplification (mesh_simplify) on the mesh of tools/mesh_probe.py: a 256^3 volume holding a unit sphere seen by 16
views of 800 x 800, extracted (914254 vertices, 1780644 triangles where that probe recorded it):

    weld         gp_mesh_simplify_plan in weld mode, gp_mesh_simplify_apply + the rows of the colours alone (hipEvent), and weld() as
                 a whole with its read (host clock around a synchronise)
    simplify     at 2 and at 4 cells of the volume: gp_mesh_simplify_bounds, the plan, apply + rows alone (hipEvent), and simplify()
                 as a whole with its two reads (host clock)
    sizes        vertices, triangles and the bytes of the PLY file (positions, colours, faces) before and after each
    numpy        the same three on the mesh of a 64^3 volume in tests/mesh_simplify_ref.py, beside the device, with the bytes compared

with the copy peak recorded in profiles/ for scale.  Informative only: no pass/fail threshold comes from here.  Prints one table and
writes it to profiles/mesh_simplify_probe.txt.

    python tools/mesh_simplify_probe.py
"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import mesh_simplify_ref  # noqa: E402
from mesh_clean_probe import sphere_mesh  # noqa: E402
from mesh_probe import DEV, REPS, host_ms, recorded_copy_peak, timed  # noqa: E402
from gaussianprediction_amd import _lib, mesh_simplify as MZ  # noqa: E402


def ply_bytes(nv, nf):
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n"
              "property uchar green\nproperty uchar blue\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n" % (nv, nf))
    return len(header) + 15 * nv + 13 * nf


def main():
    copy_peak, where = recorded_copy_peak()
    lines = [f"mesh simplification probe on {torch.cuda.get_device_name(DEV)}: hipEvent medians of {REPS} after one warm-up unless a host clock is named",
             f"copy peak (read + written bytes): {copy_peak:.0f} GB/s, {where}; beside it: the extraction of this mesh 0.62 ms (profiles/mesh_probe.txt), its components "
             "2.5 ms (profiles/mesh_clean_probe.txt)",
             f"{'entry':<112}{'ms':>10}"]

    def row(name, ms):
        lines.append(f"{name:<112}{ms:>10.3f}")

    def size(what, nv, nf):
        return f"{what}: {nv} vertices, {nf} triangles, PLY {ply_bytes(nv, nf) / 1e6:.2f} MB"

    mesh = sphere_mesh(256)
    nv, nf = mesh.vertices.shape[0], mesh.faces.shape[0]
    cell = 2.6 / 255
    l, st = MZ.lib(), _lib.stream_ptr(DEV)
    scratch = _lib.scratch(l.gp_mesh_simplify_scratch_bytes, nv, nf, device=DEV)
    lines.append(size("the mesh", nv, nf) + f"; scratch {scratch.numel() / 1e6:.1f} MB = {scratch.numel() / max(nv + nf, 1):.1f} bytes per vertex-or-face")
    counts = torch.empty(MZ.COUNT_WORDS, dtype=torch.int32, device=DEV)
    record = torch.empty(MZ.RECORD_WORDS, dtype=torch.float64, device=DEV)
    box = (C.c_double * 6)()

    def entries(name, mode, voxel, how):
        plan = lambda: _lib.check(l.gp_mesh_simplify_plan(mesh.vertices, mesh.faces, nv, nf, mode, voxel, box, how, 0, 1, 0, scratch, counts, st), "plan")      # noqa: E731
        ms = timed(plan)
        read = counts.tolist()
        nv2, nf2 = read[MZ.VERTICES], read[MZ.FACES]
        passes = sum((b + 7) // 8 for b in ([32] * 3 if mode == MZ.WELD else [max(1, (int((2.6 + voxel) / voxel) + 1).bit_length())] * 3))
        row(f"gp_mesh_simplify_plan, {name}: {read[MZ.CLUSTERS]} clusters, collapsed {read[MZ.COLLAPSED]}, duplicates {read[MZ.DUPLICATES]} "
            f"({passes} sort passes over the vertices, {3 * ((nv.bit_length() + 7) // 8)} over the faces)", ms)
        out = [torch.empty(max(n, 1), *s, dtype=d, device=DEV) for n, s, d in ((nv2, (3,), torch.float32), (nf2, (3,), torch.int32), (nv, (), torch.int32),
                                                                                 (nf2, (), torch.int32), (nv2, (), torch.int32), (nv2, (3,), torch.float32))]

        def apply():
            _lib.check(l.gp_mesh_simplify_apply(mesh.faces, nv, nf, scratch, *out[:5], st), "apply")
            _lib.check(l.gp_mesh_simplify_rows(mesh.colors, nv, nf, 3, how, scratch, out[5], st), "rows")

        row(f"gp_mesh_simplify_apply and gp_mesh_simplify_rows of the colours, {name}", timed(apply))
        lines.append("  " + size("after", nv2, nf2) + f": {100 * ply_bytes(nv2, nf2) / ply_bytes(nv, nf):.1f}% of the bytes")

    entries("weld", MZ.WELD, 0.0, MZ.FIRST)
    row("weld() as a whole: scratch, plan, the read of eight words, apply, rows (host clock)", timed(lambda: MZ.weld(mesh), host_ms))
    row("gp_mesh_simplify_bounds", timed(lambda: _lib.check(l.gp_mesh_simplify_bounds(mesh.vertices, nv, scratch, record, st), "bounds")))
    box[:] = record.tolist()[:6]
    for cells in (2, 4):
        entries(f"grid of {cells} cells of the volume ({cells * cell:.4f}), average", MZ.GRID, cells * cell, MZ.AVERAGE)
        row(f"simplify({cells} cells) as a whole: scratch, bounds, a read, plan, a read, apply, rows (host clock)", timed(lambda: MZ.simplify(mesh, cells * cell), host_ms))
    both = lambda: MZ.simplify(MZ.weld(mesh).mesh, 2 * cell)      # noqa: E731
    row("weld() then simplify(2 cells), as render_meshes chains them (host clock)", timed(both, host_ms))
    del scratch

    # ---- beside the numpy restatement, 64^3 ----
    small = sphere_mesh(64)
    cell = 2.6 / 63
    v, f, c = small.vertices.cpu().numpy(), small.faces.cpu().numpy(), small.colors.cpu().numpy()
    lines.append(size("64^3", len(v), len(f)))
    equal = True
    for name, fn, options in (("weld", lambda: MZ.weld(small), dict(voxel_size=None)), ("simplify at 2 cells", lambda: MZ.simplify(small, 2 * cell), dict(voxel_size=2 * cell)),
                              ("simplify at 4 cells", lambda: MZ.simplify(small, 4 * cell), dict(voxel_size=4 * cell))):
        got = fn()
        row(f"64^3, {name} on the device (host clock)", timed(fn, host_ms))
        start = time.perf_counter()
        want = mesh_simplify_ref.simplify(v, f, [c], **options)
        row(f"  the same in numpy (tests/mesh_simplify_ref.py), host: {len(want.vertices)} vertices, {len(want.faces)} triangles", (time.perf_counter() - start) * 1e3)
        equal = equal and (got.mesh.vertices.cpu().numpy().tobytes() == want.vertices.tobytes() and got.mesh.faces.cpu().numpy().tobytes() == want.faces.tobytes()
                           and got.mesh.colors.cpu().numpy().tobytes() == want.rows[0].tobytes() and got.vertex_map.cpu().numpy().tobytes() == want.vertex_map.tobytes())
    lines.append(f"the device's meshes, colours and maps of that mesh and the restatement's: {'equal bytes' if equal else 'DIFFERENT'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mesh_simplify_probe.txt"), "w") as fp:
        fp.write(text)


if __name__ == "__main__":
    main()
