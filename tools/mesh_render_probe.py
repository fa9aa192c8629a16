#!/usr/bin/env python
"""Time the triangle rasterizer (mesh_render) on the mesh of tools/mesh_probe.py: a 256^3 volume holding a unit sphere seen by 16 views
of 800 x 800, extracted (914254 vertices, 1780644 triangles where that probe recorded it), drawn at 800 x 800 from the first four of
those views:

    rasterize    gp_mesh_render_rasterize alone (hipEvent): the two clears, the vertex launch, the face launch, the wide launch
    resolve      gp_mesh_render_resolve alone
    shade        interpolate of the colours, normals and shade: what mode "shaded" adds
    a view       rasterize + resolve + shade as render_mesh chains them (host clock around a synchronise; it reads nothing)

with the face count, the share of wide faces, faces per second, and the bytes per second against the bytes the design must move: the
faces (12 bytes each), three 16-byte corner records per face, and the 8-byte visibility word per pixel (written by the clear, read
by the resolve), beside the copy peak recorded in profiles/.  Informative only: no pass/fail threshold comes from here.  Prints one
table and writes it to profiles/mesh_render_probe.txt.

    python tools/mesh_render_probe.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from mesh_clean_probe import sphere_mesh  # noqa: E402
from mesh_probe import DEV, REPS, event_ms, host_ms, median, recorded_copy_peak, ring_views, timed  # noqa: E402
from gaussianprediction_amd import _lib, mesh_render as MR  # noqa: E402

H = W = 800
BATCH = 40          # calls per timed window: a window of one call is a fraction of a millisecond


def batch(fn):
    def run():
        for _ in range(BATCH):
            fn()
    return run


def alternating(a, b):
    """The per-call medians of a and b, timed in alternating windows after one warm-up of each."""
    a(), b()
    ta, tb = [], []
    for _ in range(REPS):
        ta.append(event_ms(a))
        tb.append(event_ms(b))
    return median(ta) / BATCH, median(tb) / BATCH


def main():
    copy_peak, where = recorded_copy_peak()
    lines = [f"mesh render probe on {torch.cuda.get_device_name(DEV)}: per call, from hipEvent windows of {BATCH} calls, medians of {REPS} after one warm-up, unless a host clock is named; {H} x {W}",
             f"copy peak (read + written bytes): {copy_peak:.0f} GB/s, {where}",
             f"{'entry':<96}{'ms':>10}{'MB moved':>12}{'GB/s':>10}{'of peak':>9}"]

    def row(name, ms, nbytes=0):
        rate = nbytes / ms / 1e6 if nbytes else 0.0
        lines.append(f"{name:<96}{ms:>10.3f}" + (f"{nbytes / 1e6:>12.1f}{rate:>10.0f}{100 * rate / copy_peak:>8.1f}%" if nbytes else ""))

    mesh = sphere_mesh(256)
    nv, nf = mesh.vertices.shape[0], mesh.faces.shape[0]
    l, st = MR.lib(), _lib.stream_ptr(DEV)
    scratch = _lib.scratch(l.gp_mesh_render_scratch_bytes, nv, nf, H, W, device=DEV)
    lines.append(f"the mesh: {nv} vertices, {nf} triangles; scratch {scratch.numel() / 1e6:.1f} MB")
    counts = torch.empty(MR.COUNT_WORDS, dtype=torch.int32, device=DEV)
    face = torch.empty(H, W, dtype=torch.int32, device=DEV)
    depth = torch.empty(H, W, dtype=torch.float32, device=DEV)
    valid = torch.empty(H, W, dtype=torch.uint8, device=DEV)
    bary = torch.empty(3, H, W, dtype=torch.float32, device=DEV)
    plane = H * W
    must = 12 * nf + 3 * 16 * nf + 12 * nv + 16 * nv + 8 * plane          # faces, corner gathers, vertices in, records out, the clear
    for k, view in enumerate(ring_views(16)[:4]):
        vm, tx, ty = view

        def raster(cull):
            return lambda: _lib.check(l.gp_mesh_render_rasterize(mesh.vertices, mesh.faces, nv, nf, vm, tx, ty, H, W, 0.01, cull, scratch, None, counts, st), "rasterize")

        both = alternating(batch(raster(0)), batch(raster(1)))          # the two cull modes in alternating windows of BATCH calls each
        raster(0)()
        read = counts.tolist()
        row(f"view {k}: gp_mesh_render_rasterize: drawn {read[MR.DRAWN]}, degenerate {read[MR.DEGENERATE]}, wide {read[MR.WIDE]} "
            f"({100 * read[MR.WIDE] / max(read[MR.DRAWN], 1):.3f}%); {nf / both[0] / 1e6:.2f} G faces/s", both[0], must)
        raster(1)()
        row(f"view {k}: gp_mesh_render_rasterize with cull = back: culled {counts.tolist()[MR.CULLED]}", both[1], must)
        raster(0)()
        resolve = lambda: _lib.check(l.gp_mesh_render_resolve(mesh.faces, nv, nf, H, W, scratch, face, depth, valid, bary, st), "resolve")      # noqa: E731
        ms = timed(batch(resolve)) / BATCH
        row(f"view {k}: gp_mesh_render_resolve ({int(valid.sum())} covered pixels)", ms, (8 + 4 + 4 + 1 + 12) * plane)
        r = MR.rasterize(mesh, view, size=(H, W))

        def shaded():
            colour = MR.interpolate(r, mesh.colors)
            return MR.shade(colour, MR.normals(r, mesh, view, size=(H, W)), r, view, size=(H, W))

        row(f"view {k}: interpolate of the colours, normals, shade", timed(batch(shaded)) / BATCH, (12 + 4 + 1 + 12 + 12 + 1 + 12 + 12) * plane)
        whole = timed(batch(lambda: MR.render_mesh(mesh, view, size=(H, W))), host_ms) / BATCH
        row(f"view {k}: render_mesh(mode='shaded') as a whole: scratch, rasterize, resolve, interpolate, normals, shade (host clock)", whole)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mesh_render_probe.txt"), "w") as fp:
        fp.write(text)


if __name__ == "__main__":
    main()
