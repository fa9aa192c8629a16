#!/usr/bin/env python
"""Time TSDF fusion and mesh extraction (tsdf_ops):

    integrate    a 256^3 colour volume, 16 views of 800 x 800 in ONE launch, and the same 16 views as 16 launches of one view: hipEvent
                 medians of REPS after one warm-up, with the bytes each form has to move (the volume read and written once per launch,
                 the pictures once) and the share of the copy peak recorded in profiles/ (densify_probe.txt; measured where absent)
    extract      the two extraction calls on that volume holding a sphere: gp_tsdf_extract_count and gp_tsdf_extract_fill, each alone
                 (hipEvent), and extract() as a whole with its one read (host clock around a synchronise)
    fuse         one fuse() of bench.py's synthetic scene from its 8 cameras at 800 x 800 (host clock), and integrate + extract of 4 of
                 those views into a 64^3 volume beside tests/tsdf_ref.py's numpy restatement of the same, with the bytes compared

Informative only: no pass/fail threshold comes from here.  Prints one table and writes it to profiles/mesh_probe.txt.

    python tools/mesh_probe.py [--gaussians 200000]
"""
import ctypes as C
import os
import re
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import tsdf_ref  # noqa: E402
from gaussianprediction_amd import _lib, depth_ops as DO, peaks, tsdf_ops as TO  # noqa: E402
from gaussianprediction_amd.renderer import render  # noqa: E402

DEV = torch.device("cuda", 0)
ITERATION, REPS = 50000, 7


def median(v):
    return sorted(v)[len(v) // 2]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def host_ms(fn):
    torch.cuda.synchronize()
    start = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - start) * 1e3


def timed(fn, clock=event_ms):
    fn()
    return median([clock(fn) for _ in range(REPS)])


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def recorded_copy_peak():
    path = os.path.join(ROOT, "profiles", "densify_probe.txt")
    m = re.search(r"measured copy peak \(peaks\.measure, read \+ written bytes\): (\d+) GB/s", open(path).read()) if os.path.exists(path) else None
    return (float(m.group(1)), "recorded in profiles/densify_probe.txt") if m else (peaks.measure(str(DEV), gib=0.25, reps=5)["copy_GBps"], "measured now")


def ring_views(V):
    out = []
    for v in range(V):
        a = 2 * np.pi * v / V
        eye = 3.0 * np.array([np.cos(a), 0.3 * np.sin(3 * a), np.sin(a)])
        z = -eye / np.linalg.norm(eye)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = R, -R @ eye
        out.append(TO.View(torch.from_numpy(m.T.astype(np.float32).copy()).to(DEV), 0.45, 0.45))
    return out


def main():
    copy_peak, where = recorded_copy_peak()
    lines = [f"mesh probe on {torch.cuda.get_device_name(DEV)}: hipEvent medians of {REPS} after one warm-up unless a host clock is named",
             f"copy peak (read + written bytes): {copy_peak:.0f} GB/s, {where}",
             f"{'entry':<74}{'ms':>10}{'MB moved':>12}{'GB/s':>10}{'of peak':>9}"]

    def row(name, ms, nbytes=0):
        rate = nbytes / (ms * 1e-3) / 1e9 if nbytes else 0.0
        lines.append(f"{name:<74}{ms:>10.3f}" + (f"{nbytes / 1e6:>12.1f}{rate:>10.1f}{100 * rate / copy_peak:>8.1f}%" if nbytes else ""))

    # ---- integrate: 256^3 with colour, 16 views of 800 x 800 of a sphere of radius 1 ----
    n, V, H, W = 256, 16, 800, 800
    views = ring_views(V)
    voxel = 2.6 / (n - 1)
    volume = TO.TsdfVolume((-1.3, -1.3, -1.3), voxel, (n, n, n), device=DEV)
    ys, xs = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    rx, ry = ((2 * xs + 1) / W - 1) * 0.45, ((2 * ys + 1) / H - 1) * 0.45           # the ray (rx, ry, 1) z against the unit sphere 3 away
    a, b = rx * rx + ry * ry + 1, -6.0
    disc = b * b - 4 * a * 8.0
    depth1 = torch.where(disc > 0, (-b - torch.sqrt(disc.clamp_min(0))) / (2 * a), torch.zeros_like(a))
    depth = depth1[None].repeat(V, 1, 1).contiguous()
    valid = (depth > 0)
    image = torch.rand(V, 3, H, W, device=DEV)
    points, plane = n ** 3, H * W
    volume_bytes, picture_bytes = 2 * 20 * points, V * plane * 17
    row(f"integrate, {n}^3 colour volume, {V} views of {W}x{H}, ONE launch", timed(lambda: volume.integrate(depth, valid, views, image=image)), volume_bytes + picture_bytes)

    def one_by_one():
        for v in range(V):
            volume.integrate(depth[v], valid[v], views[v], image=image[v])

    row(f"the same {V} views, one launch each", timed(one_by_one), V * volume_bytes + picture_bytes)
    volume.reset()
    volume.integrate(depth, valid, views, image=image)
    seen = float((volume.weight > 0).float().mean())

    # ---- extract: the two calls alone, then extract() with its read ----
    vol_c = volume._c()
    counts = torch.empty(2, dtype=torch.int32, device=DEV)
    scratch = _lib.scratch(TO.lib().gp_tsdf_extract_scratch_bytes, n, n, n, device=DEV)
    count_call = lambda: _lib.check(TO.lib().gp_tsdf_extract_count(C.byref(vol_c), 0.0, 1.0, scratch, counts, _lib.stream_ptr(DEV)), "count")      # noqa: E731
    ms_count = timed(count_call)
    nv, nf = counts.tolist()
    vertices, colors, faces = torch.empty(nv, 3, device=DEV), torch.empty(nv, 3, device=DEV), torch.empty(nf, 3, dtype=torch.int32, device=DEV)
    fill_call = lambda: _lib.check(TO.lib().gp_tsdf_extract_fill(C.byref(vol_c), 0.0, scratch, vertices, colors, faces, _lib.stream_ptr(DEV)), "fill")   # noqa: E731
    ms_fill = timed(fill_call)
    # count: tsdf and weight read (corner reads hit the caches), 11 bytes a point written and the 3 bytes read again; fill: tsdf, 10 bytes a point, the lists
    row(f"gp_tsdf_extract_count, {n}^3 ({nv} vertices, {nf} triangles; {100 * seen:.0f} % of the points seen)", ms_count, (8 + 11 + 3) * points)
    row("gp_tsdf_extract_fill", ms_fill, (4 + 10) * points + 24 * nv + 12 * nf)
    row("extract() as a whole: scratch, count, the read of counts, fill (host clock)", timed(lambda: volume.extract(), host_ms))
    del volume, depth, valid, image, scratch, vertices, colors, faces

    # ---- fuse: bench.py's synthetic scene ----
    args = SimpleNamespace(gaussians=arg("--gaussians", 200_000), width=800, height=800, keypoints=250, nearest_num=6, time_freq=8, iteration=ITERATION,
                           scale_lo=0.003, scale_hi=0.012)
    pc, cams, _, _ = bench.build_workload(args, DEV)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    mesh = TO.fuse(cams, pc, pipe, ITERATION, time=0.5, resolution=256)
    row(f"fuse(), {pc.get_xyz.shape[0]} Gaussians, {len(cams)} views of 800x800, resolution 256: {mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} triangles (host clock)",
        timed(lambda: TO.fuse(cams, pc, pipe, ITERATION, time=0.5, resolution=256), host_ms))
    # 4 views into 64^3 beside the numpy restatement
    t = torch.tensor([0.5], device=DEV)
    four = cams[:4]
    with torch.no_grad():
        res = [DO.render_depth(c, pc, pipe, ITERATION, time=t, alpha_min=0.5) for c in four]
        pics = torch.stack([render(c, pc, pipe, torch.zeros(3, device=DEV), time=t, it=ITERATION)["render"].detach() for c in four])
        xyz = pc(t, ITERATION)[0]
        lo, hi = xyz.min(dim=0).values.tolist(), xyz.max(dim=0).values.tolist()
    d4, v4 = torch.stack([r.depth for r in res]), torch.stack([r.valid for r in res])
    voxel = max(h - l for l, h in zip(lo, hi)) / 62
    small = TO.TsdfVolume(lo, voxel, (64, 64, 64), device=DEV)

    def device_small():
        small.reset()
        small.integrate(d4, v4, four, image=pics)
        return small.extract()

    got = device_small()
    row("integrate 4 views of 800x800 into 64^3 and extract, device (host clock)", timed(device_small, host_ms))
    rv = tsdf_ref.volume(64, 64, 64, lo, voxel, 4 * voxel)
    ref_views = [SimpleNamespace(vm=c.world_view_transform.cpu().numpy().reshape(16), tanfovx=DO.view_constants(c).tanfovx, tanfovy=DO.view_constants(c).tanfovy) for c in four]
    start = time.perf_counter()
    rv.tsdf, rv.weight, rv.color = tsdf_ref.integrate(rv, d4.cpu().numpy(), v4.cpu().numpy(), pics.cpu().numpy(), ref_views)
    _, want_v, want_c, want_f = tsdf_ref.extract(rv)
    row("the same in numpy (tests/tsdf_ref.py), host", (time.perf_counter() - start) * 1e3)
    equal = (got.vertices.cpu().numpy().tobytes() == want_v.tobytes() and got.faces.cpu().numpy().tobytes() == want_f.tobytes()
             and got.colors.cpu().numpy().tobytes() == want_c.tobytes())
    lines.append(f"the device's mesh of that volume ({got.vertices.shape[0]} vertices, {got.faces.shape[0]} triangles) and the restatement's: {'equal bytes' if equal else 'DIFFERENT'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mesh_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
