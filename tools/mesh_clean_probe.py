#!/usr/bin/env python
"""Time the mesh cleanup (mesh_ops) on the mesh of tools/mesh_probe.py: a 256^3 volume holding a unit sphere seen by 16 views of
800 x 800, extracted (914254 vertices, 1780644 triangles where that probe recorded it):

    components   gp_mesh_components alone with 12 rounds enqueued (hipEvent), the rounds it used, and connected_components() as a
                 whole with its read (host clock around a synchronise)
    filter       gp_mesh_filter_plan (keep_largest = 1) and gp_mesh_filter_apply + the two gathers alone (hipEvent), and
                 filter_components() as a whole with its read (host clock)
    normals      gp_mesh_vertex_normals (hipEvent)
    clean        clean(keep_largest=1, normals=True) as a whole (host clock)
    numpy        the same three steps of tests/mesh_ref.py on the mesh of a 64^3 volume, beside the device, with the bytes compared

with the bytes each has to move at the least (every array once) against the copy peak recorded in profiles/.  Informative only: no
pass/fail threshold comes from here.  Prints one table and writes it to profiles/mesh_clean_probe.txt.

    python tools/mesh_clean_probe.py
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import mesh_ref  # noqa: E402
from mesh_probe import DEV, REPS, host_ms, recorded_copy_peak, ring_views, timed  # noqa: E402
from gaussianprediction_amd import _lib, mesh_ops as MO, tsdf_ops as TO  # noqa: E402


def sphere_mesh(n, V=16, H=800, W=800):
    """mesh_probe.py's volume: n^3 points, V views of the unit sphere 3 away, extracted."""
    volume = TO.TsdfVolume((-1.3, -1.3, -1.3), 2.6 / (n - 1), (n, n, n), device=DEV)
    ys, xs = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    rx, ry = ((2 * xs + 1) / W - 1) * 0.45, ((2 * ys + 1) / H - 1) * 0.45
    a, b = rx * rx + ry * ry + 1, -6.0
    disc = b * b - 4 * a * 8.0
    depth = torch.where(disc > 0, (-b - torch.sqrt(disc.clamp_min(0))) / (2 * a), torch.zeros_like(a))[None].repeat(V, 1, 1).contiguous()
    torch.manual_seed(0)
    volume.integrate(depth, depth > 0, ring_views(V), image=torch.rand(V, 3, H, W, device=DEV))
    return volume.extract()


def main():
    copy_peak, where = recorded_copy_peak()
    lines = [f"mesh cleanup probe on {torch.cuda.get_device_name(DEV)}: hipEvent medians of {REPS} after one warm-up unless a host clock is named",
             f"copy peak (read + written bytes): {copy_peak:.0f} GB/s, {where}",
             f"{'entry':<96}{'ms':>10}{'MB moved':>12}{'GB/s':>10}{'of peak':>9}"]

    def row(name, ms, nbytes=0):
        rate = nbytes / (ms * 1e-3) / 1e9 if nbytes else 0.0
        lines.append(f"{name:<96}{ms:>10.3f}" + (f"{nbytes / 1e6:>12.1f}{rate:>10.1f}{100 * rate / copy_peak:>8.1f}%" if nbytes else ""))

    mesh = sphere_mesh(256)
    nv, nf = mesh.vertices.shape[0], mesh.faces.shape[0]
    l, st = MO.lib(), _lib.stream_ptr(DEV)
    scratch = _lib.scratch(l.gp_mesh_scratch_bytes, nv, nf, device=DEV)
    lines.append(f"the mesh: {nv} vertices, {nf} triangles; scratch {scratch.numel() / 1e6:.1f} MB = {scratch.numel() / max(nv + nf, 1):.1f} bytes per vertex-or-face")
    vertex_label, face_label = torch.empty(nv, dtype=torch.int32, device=DEV), torch.empty(nf, dtype=torch.int32, device=DEV)
    table, state = torch.empty(3, nv, dtype=torch.int32, device=DEV), torch.empty(4, dtype=torch.int32, device=DEV)
    per = MO.ROUNDS_PER_READ
    ms = timed(lambda: _lib.check(l.gp_mesh_components(mesh.faces, nv, nf, per, 1, vertex_label, face_label, table, scratch, state, st), "components"))
    status, converged, count, rounds = state.tolist()
    # a round: the faces (12 nf) and two gathers of parents per index in the hook and again in settle, the parents read and written in the jump
    round_bytes = 2 * (12 * nf + 4 * 3 * nf) + 8 * nv + 4 * nv
    row(f"gp_mesh_components, {per} rounds enqueued, {rounds} used, converged {converged}: {count} components", ms, rounds * round_bytes + 12 * nf + 4 * nf + 16 * nv)
    one = timed(lambda: _lib.check(l.gp_mesh_components(mesh.faces, nv, nf, 1, 1, vertex_label, face_label, table, scratch, state, st), "components"))
    row("  the same with ONE round enqueued (a round and the table; not converged)", one)
    row(f"  hence per further round enqueued ({rounds - 1} that work, {per - rounds} that return at once), about {1e3 * (ms - one) / max(per - 1, 1):.1f} us each",
        (ms - one) / max(per - 1, 1))
    comps = MO.connected_components(mesh.faces, nv)
    row("connected_components() as a whole: scratch, the rounds, the table, the read of four words (host clock)", timed(lambda: MO.connected_components(mesh.faces, nv), host_ms))
    sizes = sorted(comps.face_counts.tolist(), reverse=True)
    lines.append(f"  components by faces: {sizes[:6]}{' ...' if len(sizes) > 6 else ''}; rounds {comps.rounds}")

    counts = torch.empty(3, dtype=torch.int32, device=DEV)
    ncomp = comps.labels.shape[0]
    labels, face_counts = comps.labels.contiguous(), comps.face_counts.contiguous()
    plan = lambda: _lib.check(l.gp_mesh_filter_plan(mesh.faces, nv, nf, comps.vertex_label, labels, face_counts, ncomp, -1, 1, scratch, counts, st), "plan")      # noqa: E731
    ms_plan = timed(plan)
    _, nv2, nf2 = counts.tolist()
    row(f"gp_mesh_filter_plan, keep_largest = 1: {nv2} vertices and {nf2} triangles stay", ms_plan, 4 * nv + 2 * nv + 12 * nf + nf + 2 * (nv + nf) + 4 * (nv + nf))
    vertex_index, face_index = torch.empty(nv2, dtype=torch.int32, device=DEV), torch.empty(nf2, dtype=torch.int32, device=DEV)
    faces_out, rows_out = torch.empty(nf2, 3, dtype=torch.int32, device=DEV), torch.empty(nv2, 3, device=DEV)

    def apply():
        _lib.check(l.gp_mesh_filter_apply(mesh.faces, nv, nf, scratch, vertex_index, face_index, faces_out, st), "apply")
        for src in (mesh.vertices, mesh.colors):
            _lib.check(l.gp_mesh_gather_rows(src, nv, 3, scratch, rows_out, st), "gather")

    row("gp_mesh_filter_apply and gp_mesh_gather_rows of positions and colours", timed(apply), 5 * (nv + nf) + 12 * nf + 12 * nf + 16 * nf2 + 4 * nv2 + 2 * 12 * (nv + nv2))
    row("filter_components() as a whole, components given: scratch, plan, the read of three words, apply, gathers (host clock)",
        timed(lambda: MO.filter_components(mesh, keep_largest=1, components=comps), host_ms))
    normals = torch.empty(nv, 3, device=DEV)
    ms_n = timed(lambda: _lib.check(l.gp_mesh_vertex_normals(mesh.vertices, mesh.faces, nv, nf, scratch, normals, None, st), "normals"))
    # the faces twice and three gathered positions, the face vectors written and gathered once per incidence, keys and ids through the sort's passes
    passes = (MO_bits(nv) + 7) // 8
    row(f"gp_mesh_vertex_normals ({passes} sort passes over {3 * nf} pairs)", ms_n, 2 * 12 * nf + 36 * nf + 12 * nf + 36 * nf + passes * 2 * 24 * nf + 12 * nf + 8 * nv + 12 * nv)
    row("clean(keep_largest=1, normals=True) as a whole: two reads (host clock)", timed(lambda: MO.clean(mesh, keep_largest=1, normals=True), host_ms))
    del scratch, table, face_label, vertex_label

    # ---- beside the numpy restatement, 64^3 ----
    small = sphere_mesh(64)
    got_c = MO.connected_components(small.faces, small.vertices.shape[0])
    got_f = MO.filter_components(small, keep_largest=1, components=got_c)
    got_n = MO.vertex_normals(got_f.mesh.vertices, got_f.mesh.faces)
    row(f"64^3 ({small.vertices.shape[0]} vertices, {small.faces.shape[0]} triangles): components, filter, normals on the device (host clock)",
        timed(lambda: MO.clean(small, keep_largest=1, normals=True), host_ms))
    v, f, c = small.vertices.cpu().numpy(), small.faces.cpu().numpy(), small.colors.cpu().numpy()
    start = time.perf_counter()
    want_c = mesh_ref.components(f, len(v))
    want_f = mesh_ref.filter_components(v, f, [c], None, 1)
    want_n = mesh_ref.vertex_normals(want_f[1], want_f[2])
    row("the same in numpy (tests/mesh_ref.py: a union in Python, the components twice), host", (time.perf_counter() - start) * 1e3)
    equal = (got_c.vertex_label.cpu().numpy().tobytes() == want_c[1].tobytes() and got_f.mesh.faces.cpu().numpy().tobytes() == want_f[2].tobytes()
             and got_f.mesh.vertices.cpu().numpy().tobytes() == want_f[1].tobytes() and got_n.cpu().numpy().tobytes() == want_n.tobytes())
    lines.append(f"the device's labels, kept mesh and normals of that mesh and the restatement's: {'equal bytes' if equal else 'DIFFERENT'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mesh_clean_probe.txt"), "w") as fp:
        fp.write(text)


def MO_bits(v):
    return max(1, int(v).bit_length())


if __name__ == "__main__":
    main()
