#!/usr/bin/env python
"""Time the GCN keypoint motion predictor on the HIP path (motion.GCN_xyzr: gp_gcn_rollout, gp_gcn_layer_forward / _backward) and on the
float32 torch restatement of tests/gcn_ref.py, on the same device in one process, alternated, after warm-ups, each run timed with device
events; the figure is the median of 20 runs and the run-to-run spread (min .. max) is printed beside it.

Shapes: K = 100 and K = 300 keypoints, T = 10, H = 128, 4 stages, output_size 1 [REF options/gaussian_option.py:21-38]:
  * the 150-frame eval-mode rollout (B = 1);
  * one training iteration (forward + backward + Adam) at B = 32.
FLOPs are counted from the shapes (2 B M Fin Fout + 2 B M^2 Fout per graph convolution, 2 B M Fin Fout per Linear; the backward as
twice the forward) and set against the 155 Tflop/s fp32 matrix peak measured on this part.  Launch counts come from
the torch profiler.  Writes profiles/gcn_probe.txt.

    python tools/gcn_probe.py [--keypoints 100,300]
"""
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import gcn_ref as R  # noqa: E402
from gaussianprediction_amd import motion  # noqa: E402

DEV = torch.device("cuda", 0)
T, H, STAGES, OUT, FRAMES, BATCH = 10, 128, 4, 1, 150, 32
REPS, WARM = 20, 3
PEAK_TFLOPS = 155.0


def stats(v):
    s = sorted(v)
    return s[len(s) // 2], s[0], s[-1]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


def forward_flop(c, B):
    total = 0
    for ch in (3, 4):
        M = ch * c.K
        gc = lambda fin, fout: 2 * B * M * fin * fout + 2 * B * M * M * fout
        total += gc(c.T, c.H) + 2 * c.num_stage * gc(c.H, c.H) + 2 * B * M * c.H * c.H + 2 * B * M * c.H * c.out
    return total


def alternate(hip_fn, torch_fn):
    th, tt = [], []
    for k in range(WARM + REPS):
        a, b = event_ms(hip_fn), event_ms(torch_fn)
        if k >= WARM:
            th.append(a), tt.append(b)
    return stats(th), stats(tt)


def report(lines, what, hip, ref, flop, n_hip, n_ref, per=1):
    (mh, lh, hh), (mt, lt, ht) = hip, ref
    inside = not (hh < lt or ht < lh)
    lines.append(f"  {what}")
    lines.append(f"    HIP path          : {mh:9.3f} ms (min {lh:.3f} .. max {hh:.3f}), {n_hip} launches = {n_hip / per:.1f} per frame"
                 if per > 1 else f"    HIP path          : {mh:9.3f} ms (min {lh:.3f} .. max {hh:.3f}), {n_hip} launches")
    lines.append(f"    torch restatement : {mt:9.3f} ms (min {lt:.3f} .. max {ht:.3f}), {n_ref} launches" + (f" = {n_ref / per:.1f} per frame" if per > 1 else ""))
    lines.append(f"    torch / HIP = {mt / mh:.2f}x" + ("  (the two spreads overlap: counts as equal)" if inside else ""))
    lines.append(f"    {flop / 1e9:.2f} Gflop from the shapes: HIP path {flop / mh / 1e9:.2f} Tflop/s = {100 * flop / mh / 1e9 / PEAK_TFLOPS:.2f} % of the "
                 f"{PEAK_TFLOPS:.0f} Tflop/s fp32 matrix peak")


def probe(K, lines):
    c = SimpleNamespace(name=f"probe{K}", K=K, T=T, H=H, num_stage=STAGES, out=OUT, B=BATCH, no_mapping=False)
    state = R.seeded_state(c)
    batch = R.to_torch(R.seeded_batch(c), torch.float32, DEV)
    args = SimpleNamespace(norm_rotation=True, epoch=100)
    model = motion.GCN_xyzr(T, H, OUT, 0, num_stage=STAGES, node_n=K).to(DEV)
    model.load_state_dict(R.to_torch(state, torch.float32, DEV), strict=True)
    s = R.to_torch(state, torch.float32, DEV)
    xyz, rot = batch["xyz_inputs"][0].contiguous(), batch["rotation_inputs"][0].contiguous()
    lines.append("")
    lines.append(f"K = {K} keypoints (M = {3 * K} and {4 * K}), T = {T}, H = {H}, {STAGES} stages, output_size {OUT} "
                 f"(median of {REPS} after {WARM} warm-ups, hipEvent, the two paths alternated)")
    # the rollout
    model.eval()
    hip_fn = lambda: model.rollout(xyz, rot, FRAMES, OUT, True)                # noqa: E731
    torch_fn = lambda: R.rollout(s, c, xyz, rot, FRAMES, True)                 # noqa: E731
    hip, ref = alternate(hip_fn, torch_fn)
    a, b = hip_fn(), torch_fn()
    report(lines, f"rollout of {FRAMES} frames, B = 1", hip, ref, FRAMES * forward_flop(c, 1), launches(hip_fn), launches(torch_fn), per=FRAMES)
    lines.append(f"    frame {FRAMES - 1}: |HIP - torch| = {float((a[0] - b[0]).abs().max()):.2e} (xyz), {float((a[1] - b[1]).abs().max()):.2e} (rot); "
                 f"two HIP runs bit-identical: {all(torch.equal(x, y) for x, y in zip(a, hip_fn()))}")
    # one training iteration
    model.train()
    optimizer, _ = motion.make_optimizer(args, model)
    params = [s[k].requires_grad_(True) for k in s if R.is_param(k)]
    opt_ref = torch.optim.Adam(params, lr=0.01, eps=1e-15)

    def torch_iter():
        stats_ = {}
        xp, rp = R.operate(s, c, batch["xyz_inputs"], batch["rotation_inputs"], True, True, stats_)
        loss = R.loss_of(xp, batch["xyz_gt"], rp, batch["rotation_gt"])
        opt_ref.zero_grad()
        loss.backward()
        opt_ref.step()
        with torch.no_grad():
            for k, v in stats_.items():
                s[k].copy_(v)

    hip_iter = lambda: motion.train_iteration(args, model, optimizer, batch)   # noqa: E731
    hip, ref = alternate(hip_iter, torch_iter)
    report(lines, f"one training iteration (forward + backward + Adam), B = {BATCH}", hip, ref, 3 * forward_flop(c, BATCH), launches(hip_iter),
           launches(torch_iter))
    del model, s, batch
    torch.cuda.empty_cache()


def main():
    ks = (100, 300)
    if "--keypoints" in sys.argv:
        ks = tuple(int(v) for v in sys.argv[sys.argv.index("--keypoints") + 1].split(","))
    lines = [f"GCN motion predictor probe on {torch.cuda.get_device_name(DEV)}: HIP path (include/gp_gcn.h) against the float32 torch restatement "
             f"(tests/gcn_ref.py), seeded weights"]
    for K in ks:
        probe(K, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "gcn_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
