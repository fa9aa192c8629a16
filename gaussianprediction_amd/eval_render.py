"""The render-to-disk loops of the reference's eval.py: the test views, a frozen-view sequence over the training times, and the
interpolated-pose video frames, written as PNG files encoded on the device (png_ops) behind a render loop that never waits for a
frame (SpeculativeRenderer); on request the video frames also go into a Motion-JPEG video encoded on the device (jpeg_ops).

  [REF eval.py:75-118]     render_video          (+ utils/camera_utils.py:20-70, 269-276: lerp, slerp, interpolation_pose)
  [REF eval.py:159-190]    render_trainSequence
  [REF eval.py:192-226]    render_set
  [REF eval.py:110,155,182,217]   torchvision.utils.save_image per frame -> one PngWriter.submit per ring of frames

The reference muxes the video frames into an mp4 with cv2 [REF eval.py:113-115]; neither cv2 nor ffmpeg exists here, so by default
render_video stops at the numbered frames in renders_video/ and returns their count, and with `video=` it writes the reference's
file name with another container beside that directory: ours_<iteration>/<scene>.avi, Motion-JPEG from jpeg_ops.VideoWriter.  The
files: eval/<name>/ours_<iteration>/{renders, gt}/%05d.png, renders/view_%03d/%05d.png, renders_video/%05d.png -- the trees
`metrics.evaluate_dirs` scores.

  [REF eval.py:38-73]      project_trajectory, drawn on the device (trajectory_ops: this project's own line definition, parity with
                           cv2.line is unpinned); keypoint_trails for ready-made paths; render_trajectories writes
                           trajectories/%05d.png and is opt-in -- none of the loops above calls it.
  [REF utils/visualizer_utils.py:57-82]   PCA_vis, as rendered pictures: render_features colours every Gaussian by the leading
                           principal components of its motion feature (feature_vis) and writes features/%05d.png; opt-in as well.
  [REF scene/cameras.py fwd_flow / bwd_flow, never rendered there]   render_flows: the optical flow between neighbouring views, or of
                           one camera over a time step, rendered through the composite (flow_ops) and written as colour-wheel
                           pictures to flows/%05d.png, on request as Middlebury .flo files and a video; opt-in as well.
  [REF eval.py:109 unwraps the render's "depth" and drops it]   render_depths: the depth map of every view (depth_ops) as a colour-mapped
                           picture to depths/%05d.png, on request normals/%05d.png, PFM files, the visible surface as points/%05d.ply
                           and a video; opt-in as well.
  [no counterpart in the reference]   render_meshes: the views of every time step fused into a TSDF volume and extracted as one
                           watertight, coloured triangle mesh (tsdf_ops) to meshes/%05d.ply; opt-in as well."""
from __future__ import annotations

import json
import os
import time as _time

import numpy as np
import torch

from .cameras import Camera
from .png_ops import PngWriter

DOT_THRESHOLD = 0.9995


def slerp(t, q0, q1):
    """The reference's slerp [REF utils/camera_utils.py:26-70] on the host, in the inputs' precision: the angle comes from the
    normalised inputs, the weights multiply the inputs AS GIVEN, there is no shortest-arc flip, and above |dot| 0.9995 the result is
    the plain lerp of the un-normalised inputs.  numpy arrays or CPU tensors in, a numpy array out."""
    a = q0.detach().cpu().numpy() if torch.is_tensor(q0) else np.asarray(q0)
    b = q1.detach().cpu().numpy() if torch.is_tensor(q1) else np.asarray(q1)
    cos_angle = np.sum((a / np.linalg.norm(a)) * (b / np.linalg.norm(b)))
    if np.abs(cos_angle) > DOT_THRESHOLD:
        return (1 - t) * a + t * b
    angle = np.arccos(cos_angle)
    return (np.sin(angle - angle * t) / np.sin(angle)) * a + (np.sin(angle * t) / np.sin(angle)) * b


def interpolation_pose(view, previous_view, ratio):
    """(new_T, new_R) between previous_view (ratio 0) and view (ratio 1) [REF utils/camera_utils.py:269-276]: the translation
    interpolated linearly, the rotation by slerp of the two matrices' quaternions (pytorch3d.transforms: this repository's shim)."""
    from pytorch3d.transforms import matrix_to_quaternion, quaternion_to_matrix
    t, pre_t = np.asarray(view.T), np.asarray(previous_view.T)
    new_t = pre_t + (t - pre_t) * ratio
    quat = matrix_to_quaternion(torch.from_numpy(np.asarray(view.R)))
    pre_quat = matrix_to_quaternion(torch.from_numpy(np.asarray(previous_view.R)))
    new_quat = torch.from_numpy(np.asarray(slerp(ratio, pre_quat, quat)))
    new_R = quaternion_to_matrix(new_quat[None]).squeeze().cpu().numpy()
    return new_t, new_R


def video_schedule(n_views, interpolation, step):
    """The frames render_video walks, as (frame_id, previous_index, view_index, ratio) [REF eval.py:81-112]: view 0 gives the one
    frame 0; view idx with idx % step == 0 gives `interpolation` frames between view idx - step and itself, numbered
    frame + (idx // step - 1) * interpolation for frame = 1 .. interpolation.  interpolation * ((n_views - 1) // step) + 1 in all."""
    n_views, interpolation, step = int(n_views), int(interpolation), int(step)
    if n_views < 1 or interpolation < 1 or step < 1:
        raise ValueError(f"video_schedule: n_views = {n_views}, interpolation = {interpolation}, step = {step} must all be >= 1")
    frames = [(0, 0, 0, 1 / interpolation)]
    for idx in range(step, n_views, step):
        for frame in range(1, interpolation + 1):
            frames.append((frame + (idx // step - 1) * interpolation, idx - step, idx, frame / interpolation))
    return frames


def _cam(view):
    return view["cam"] if isinstance(view, dict) else view          # (optical-flow datasets wrap the camera)


def _time_of(view, dev):
    return torch.as_tensor(np.asarray(view.time), dtype=torch.float32).reshape(-1)[:1].to(dev)


def _run(frames, gaussians, pipeline, background, iteration, writer, renderer, video=None):
    """Render `frames` -- an iterable of (camera, time tensor, render file, gt image or None, gt file) -- through a
    SpeculativeRenderer; after every ring's flush() (the images are final then: overflowed frames were replaced in place) the ring's
    images go to ONE writer.submit, its ground truths to a second; video: a jpeg_ops.VideoWriter that takes the ring's images too
    (closed here).  Returns the statistics dictionary."""
    from .renderer import SpeculativeRenderer
    sr = renderer if renderer is not None else SpeculativeRenderer(gaussians, pipeline, background)
    own = writer is None
    w = PngWriter() if own else writer
    sr.flush()
    ring, count, again = [], 0, 0

    def close_ring():
        nonlocal ring, again
        again += sr.flush()
        if ring:
            w.submit([im for im, _, _, _ in ring], [p for _, p, _, _ in ring])
            if video is not None:
                video.submit([im for im, _, _, _ in ring])
            gts = [(gt, gp) for _, _, gt, gp in ring if gt is not None]
            if gts:
                w.submit([gt for gt, _ in gts], [gp for _, gp in gts])
        ring = []

    torch.cuda.synchronize(background.device)
    start = _time.perf_counter()
    try:
        with torch.no_grad():
            for cam, time_, path, gt, gt_path in frames:
                if len(ring) >= sr.slots:
                    close_ring()
                image = sr(cam, time=time_, it=iteration)["render"]
                ring.append((image, path, gt[0:3].to(image.device) if gt is not None else None, gt_path))
                count += 1
            close_ring()
        if own:
            w.close()
        else:
            torch.cuda.synchronize(background.device)       # (a caller's writer: its files are complete after its close())
        if video is not None:
            video.close()
    except BaseException:
        if video is not None:
            try:
                video.close()
            except BaseException:       # noqa: BLE001  (the loop's own exception wins)
                pass
        if own:
            try:
                w.close()
            except BaseException:       # noqa: BLE001  (the loop's own exception wins)
                pass
        raise
    seconds = _time.perf_counter() - start
    return {"frames": count, "seconds": seconds, "views_per_s": count / seconds if seconds > 0 else float("inf"), "rerendered": again}


def render_set(model_path, name, iteration, views, gaussians, pipeline, background, args=None, writer=None, renderer=None):
    """Every view at its own time to eval/<name>/ours_<iteration>/renders/%05d.png, its ground truth (`original_image`) to gt/
    [REF eval.py:192-226]; the keypoints to <model_path>/kpts_fps.txt (the first args.max_points) and, with args.adaptive_points_num > 0,
    kpts_incre.txt (the rest).  `args` defaults to the model's own.  writer: a PngWriter of the caller's (it closes it); renderer: a
    SpeculativeRenderer to keep its capacity across calls.  Returns (eval_path, {"frames", "seconds", "views_per_s", "rerendered"})."""
    eval_path = os.path.join(model_path, "eval", name)
    render_path = os.path.join(eval_path, "ours_{}".format(iteration), "renders")
    gts_path = os.path.join(eval_path, "ours_{}".format(iteration), "gt")
    os.makedirs(render_path, exist_ok=True)
    os.makedirs(gts_path, exist_ok=True)
    args = args if args is not None else getattr(gaussians, "args", None)
    kpts = getattr(gaussians, "get_superGaussians", None)
    if kpts is not None:
        kpts = kpts.detach().cpu().numpy()
        max_points = int(getattr(args, "max_points", kpts.shape[0]))
        np.savetxt(os.path.join(model_path, "kpts_fps.txt"), kpts[:max_points])
        if getattr(args, "adaptive_points_num", 0) > 0:
            np.savetxt(os.path.join(model_path, "kpts_incre.txt"), kpts[max_points:])
    dev = background.device
    views = [_cam(v) for v in views]
    frames = ((v, _time_of(v, dev), os.path.join(render_path, "{0:05d}.png".format(i)), v.original_image,
               os.path.join(gts_path, "{0:05d}.png".format(i))) for i, v in enumerate(views))
    return eval_path, _run(frames, gaussians, pipeline, background, iteration, writer, renderer)


def render_trainSequence(model_path, name, iteration, train_views, gaussians, pipeline, background, test_views, freeze_view_number=5,
                         writer=None, renderer=None):
    """The frozen test view `freeze_view_number` at every training view's time to renders/view_%03d/%05d.png, the training views'
    ground truth to gt/ [REF eval.py:159-190].  Returns (eval_path, statistics)."""
    eval_path = os.path.join(model_path, "eval", name)
    render_path = os.path.join(eval_path, "ours_{}".format(iteration), "renders", f"view_{freeze_view_number:03d}")
    gts_path = os.path.join(eval_path, "ours_{}".format(iteration), "gt")
    os.makedirs(render_path, exist_ok=True)
    os.makedirs(gts_path, exist_ok=True)
    dev = background.device
    view_freeze = _cam(test_views[freeze_view_number])
    train_views = [_cam(v) for v in train_views]
    frames = ((view_freeze, _time_of(v, dev), os.path.join(render_path, "{0:05d}.png".format(i)), v.original_image,
               os.path.join(gts_path, "{0:05d}.png".format(i))) for i, v in enumerate(train_views))
    return eval_path, _run(frames, gaussians, pipeline, background, iteration, writer, renderer)


def render_video(model_path, name, iteration, views, gaussians, pipeline, background, interpolation=5, step=None, writer=None,
                 renderer=None, video=None, fps=120):
    """The frames of `video_schedule` -- poses and times interpolated between neighbouring views -- to renders_video/%05d.png
    [REF eval.py:75-118]; step defaults to the reference's 2 for a "vrig" model path, else 1.  video: True for
    ours_<iteration>/<basename(dirname(model_path))>.avi -- the reference's name [REF eval.py:113] with the container's extension,
    beside renders_video/ -- or a path; the frames then also go, in order, into a Motion-JPEG video at `fps` (the reference's 120),
    encoded on the device, and the statistics gain "video": its path.  Returns (eval_path, statistics)."""
    eval_path = os.path.join(model_path, "eval", name)
    render_path = os.path.join(eval_path, "ours_{}".format(iteration), "renders_video")
    os.makedirs(render_path, exist_ok=True)
    if step is None:
        step = 2 if "vrig" in model_path else 1
    dev = background.device
    views = [_cam(v) for v in views]

    def frames():
        for frame_id, pi, vi, ratio in video_schedule(len(views), interpolation, step):
            view, previous = views[vi], views[pi]
            t1, t0 = _time_of(view, "cpu"), _time_of(previous, "cpu")              # (float32 on the host: no read of the device)
            time_inter = t0 + round(ratio * interpolation) * ((t1 - t0) / interpolation)        # previous + frame * time_slice
            new_t, new_R = interpolation_pose(view, previous, ratio)
            cam = Camera(R=new_R, T=new_t, FoVx=previous.FoVx, FoVy=previous.FoVy, width=previous.image_width, height=previous.image_height,
                         time=float(time_inter), device=dev, uid=getattr(previous, "uid", 0))
            yield cam, time_inter.to(dev), os.path.join(render_path, "{0:05d}.png".format(frame_id)), None, None

    if video is None or video is False:
        return eval_path, _run(frames(), gaussians, pipeline, background, iteration, writer, renderer)
    from .jpeg_ops import VideoWriter
    video_path = (os.path.join(eval_path, "ours_{}".format(iteration), os.path.basename(os.path.dirname(model_path)) + ".avi")
                  if video is True else os.fspath(video))
    stats = _run(frames(), gaussians, pipeline, background, iteration, writer, renderer, video=VideoWriter(video_path, fps))
    stats["video"] = video_path
    return eval_path, stats


# ---- motion trajectories [REF eval.py:38-73] ----------------------------------------------------------------------------------
def _on_device(what, t):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{what} is on {t.device if torch.is_tensor(t) else 'the host'} -- HIP kernels only (no CPU fallback)")


def project_trajectory(gaussians, view, tidx, time_freq, iteration, steps=60, colors=None, seed=0, base=None, min_depth=None):
    """The picture of [REF eval.py:38-73]: for the Gaussian seen at every pixel of `view` (tidx [H, W] int32 from render(), -1 where
    there is none), the polyline of its projected position at `steps` times from 0 to the view's time, a later line over an earlier
    one.  Returns [H, W, 3] float32 on the device, over zero or over `base` [3, H, W].  The points are the valid entries of
    tidx.view(-1) in pixel order; colors: [P, 3] for them, default trajectory_ops.default_colors(P, seed).  The drawing's definition is
    trajectory_ops' (parity with cv2.line is unpinned).

    Each raw time goes to gaussians.forward(t, iteration) as render() passes it and the step's positions are the model's _last_xyz_t
    (the reference reads `all_xyz_motion + xyz`, which nothing there assigns).  `time_freq` is accepted for the reference's signature
    and is unused: the reference encodes the time with it BEFORE forward [REF eval.py:58], and forward encodes its argument again --
    here forward takes the raw time and encodes it once, with the model's own frequency count.  One read of the device before the
    loop (the number of valid pixels); none inside it."""
    from .trajectory_ops import TrajectoryCanvas
    steps = int(steps)
    if steps < 1:
        raise RuntimeError(f"project_trajectory: steps = {steps} must be >= 1")
    _on_device("project_trajectory: tidx", tidx)
    if tidx.dim() != 2 or tidx.dtype != torch.int32:
        raise RuntimeError(f"project_trajectory: tidx must be [H, W] int32 (got {tuple(tidx.shape)} {tidx.dtype})")
    H, W = tidx.shape
    flat = tidx.reshape(-1)
    idx = flat[flat != -1].contiguous()                      # (the one read: the count of valid pixels sizes the tensor)
    view = _cam(view)
    canvas = TrajectoryCanvas(view, idx.numel(), tidx.device, H=H, W=W, colors=colors, seed=seed, min_depth=min_depth)
    end = float(np.asarray(view.time.detach().cpu() if torch.is_tensor(view.time) else view.time).reshape(-1)[0])
    times = torch.linspace(0, end, steps).to(tidx.device)
    if canvas.P > 0 and steps > 1:
        with torch.no_grad():
            for i in range(steps):
                gaussians.forward(times[i:i + 1], iteration)
                canvas.step(gaussians._last_xyz_t, idx)
    return canvas.image(base)


def keypoint_trails(view, kpts_xyz, colors=None, base=None, seed=0, min_depth=None, H=None, W=None):
    """The same drawing for ready-made paths: kpts_xyz [S, K, 3] float32 on the device, such as the positions of
    motion.keypoint_trajectories or of a GCN rollout (observed and predicted steps concatenated along S).  Returns [H, W, 3] float32;
    H, W default to the view's."""
    from .trajectory_ops import TrajectoryCanvas
    if not torch.is_tensor(kpts_xyz) or kpts_xyz.dim() != 3 or kpts_xyz.shape[2] != 3:
        raise RuntimeError("keypoint_trails: kpts_xyz must be a [S, K, 3] tensor")
    _on_device("keypoint_trails: kpts_xyz", kpts_xyz)
    canvas = TrajectoryCanvas(_cam(view), kpts_xyz.shape[1], kpts_xyz.device, H=H, W=W, colors=colors, seed=seed, min_depth=min_depth)
    for xyz in kpts_xyz.detach().to(torch.float32):
        canvas.step(xyz)
    return canvas.image(base)


def render_trajectories(model_path, name, iteration, views, gaussians, pipeline, background, steps=60, overlay=True, writer=None):
    """Opt-in (no other loop calls it): per view one exact render() for tidx, then project_trajectory -- over the render with
    overlay=True -- to eval/<name>/ours_<iteration>/trajectories/%05d.png.  writer: a PngWriter of the caller's (it closes it).
    Returns (eval_path, {"frames", "seconds"})."""
    from .renderer import render
    eval_path = os.path.join(model_path, "eval", name)
    out_path = os.path.join(eval_path, "ours_{}".format(iteration), "trajectories")
    os.makedirs(out_path, exist_ok=True)
    import contextlib
    own = writer is None
    dev = background.device
    start = _time.perf_counter()
    with (PngWriter() if own else contextlib.nullcontext(writer)) as w:      # (its own writer is closed on every way out)
        for i, view in enumerate(_cam(v) for v in views):
            with torch.no_grad():
                out = render(view, gaussians, pipeline, background, time=_time_of(view, dev), it=iteration)
            image = project_trajectory(gaussians, view, out["tidx"], None, iteration, steps=steps, base=out["render"] if overlay else None)
            w.submit(image.permute(2, 0, 1), os.path.join(out_path, "{0:05d}.png".format(i)))
    if not own:
        torch.cuda.synchronize(dev)                          # (a caller's writer: its files are complete after its close())
    return eval_path, {"frames": len(views), "seconds": _time.perf_counter() - start}


# ---- feature renders [REF utils/visualizer_utils.py:57-82] ------------------------------------------------------------------------
def render_features(model_path, name, iteration, views, gaussians, pipeline, background, features=None, dim=3, model=None, writer=None):
    """Opt-in (no other loop calls it): every view rendered with override_color = the PCA colours of `features` [N, D] (default: the
    model's motion_feature), to eval/<name>/ours_<iteration>/features/%05d.png.  The basis is fitted once (feature_vis.pca_fit with
    `dim` components, 3 or 5), unless `model`, a feature_vis.PcaModel, gives a frozen one.  writer: a PngWriter of the caller's (it
    closes it).  Returns (the features directory, the PcaModel)."""
    from .feature_vis import pca_fit
    from .renderer import render
    import contextlib
    if features is None:
        features = gaussians.motion_feature
    _on_device("render_features: features", features)
    features = features.detach().contiguous()
    if model is None:
        model = pca_fit(features, dim)
    colors = model.colors(features)
    out_path = os.path.join(model_path, "eval", name, "ours_{}".format(iteration), "features")
    os.makedirs(out_path, exist_ok=True)
    own = writer is None
    dev = background.device
    with (PngWriter() if own else contextlib.nullcontext(writer)) as w:      # (its own writer is closed on every way out)
        for i, view in enumerate(_cam(v) for v in views):
            with torch.no_grad():
                out = render(view, gaussians, pipeline, background, time=_time_of(view, dev), it=iteration, override_color=colors)
            w.submit(out["render"], os.path.join(out_path, "{0:05d}.png".format(i)))
    if not own:
        torch.cuda.synchronize(dev)                          # (a caller's writer: its files are complete after its close())
    return out_path, model


# ---- segment renders [REF utils/visualizer_utils.py:35-44] ------------------------------------------------------------------------
def render_segments(model_path, name, iteration, views, gaussians, pipeline, background, labels=None, features=None, bandwidth=None, seeds=None,
                    writer=None):
    """Opt-in (no other loop calls it): every view rendered with override_color = feature_vis.label_colors(labels), to
    eval/<name>/ours_<iteration>/segments/%05d.png -- which Gaussians move together, as parts.  labels [N] int64 on the device; by
    default the mean-shift labels of `features` [N, D] (default: the model's motion_feature): feature_vis.cluster(features, "MeanShift"),
    or meanshift_ops.mean_shift(features, bandwidth, seeds) when a bandwidth or seeds are given.  writer: a PngWriter of the caller's (it
    closes it).  Returns (the segments directory, the MeanShiftResult, or None where the labels were given)."""
    from .feature_vis import label_colors
    from .meanshift_ops import mean_shift
    from .renderer import render
    import contextlib
    result = None
    if labels is None:
        if features is None:
            features = gaussians.motion_feature
        _on_device("render_segments: features", features)
        result = mean_shift(features.detach().contiguous(), bandwidth=bandwidth, seeds=seeds)      # (cluster(features, "MeanShift") is its .labels)
        labels = result.labels
    _on_device("render_segments: labels", labels)
    colors = label_colors(labels)
    out_path = os.path.join(model_path, "eval", name, "ours_{}".format(iteration), "segments")
    os.makedirs(out_path, exist_ok=True)
    own = writer is None
    dev = background.device
    with (PngWriter() if own else contextlib.nullcontext(writer)) as w:      # (its own writer is closed on every way out)
        for i, view in enumerate(_cam(v) for v in views):
            with torch.no_grad():
                out = render(view, gaussians, pipeline, background, time=_time_of(view, dev), it=iteration, override_color=colors)
            w.submit(out["render"], os.path.join(out_path, "{0:05d}.png".format(i)))
    if not own:
        torch.cuda.synchronize(dev)                          # (a caller's writer: its files are complete after its close())
    return out_path, result



# ---- optical-flow renders (flow_ops) ------------------------------------------------------------------------------------------------
def render_flows(model_path, name, iteration, views, gaussians, pipeline, background, dt=None, max_flow=None, alpha_min=1e-3, save_flo=False,
                 writer=None, video=False):
    """Opt-in (no other loop calls it): the optical flow of every frame as a colour-wheel picture (flow_ops.colorize; pixels without a
    valid flow are black) to eval/<name>/ours_<iteration>/flows/%05d.png.  dt=None: frame i is the flow from view i at its time to view
    i + 1 at its time -- scene and camera motion, len(views) - 1 frames; a number: the flow of view i's own camera from its time to its
    time + dt -- scene motion alone, len(views) frames.  max_flow=None scales every frame by its own largest magnitude; a number gives
    one scale for the sequence, which a video needs.  save_flo: also %05d.flo beside every picture (one read of the device per frame,
    only then).  video: True for ours_<iteration>/<basename(dirname(model_path))>_flows.avi, or a path: the pictures also go, in order,
    into a Motion-JPEG video as render_video's do, and the statistics gain "video".  `background` names the device only: the flow is
    composited over zero whatever the scene's background is.  Each frame costs flow_ops.render_flow's three deformation passes.
    writer: a PngWriter of the caller's (it closes it).  Returns (the flows directory, {"frames", "seconds"})."""
    from .flow_ops import colorize, render_flow, write_flo
    import contextlib
    out_path = os.path.join(model_path, "eval", name, "ours_{}".format(iteration), "flows")
    os.makedirs(out_path, exist_ok=True)
    dev = background.device
    views = [_cam(v) for v in views]
    if dt is None:
        frames = [(views[i], _time_of(views[i], dev), _time_of(views[i + 1], dev), views[i + 1]) for i in range(len(views) - 1)]
    else:
        frames = [(v, _time_of(v, dev), _time_of(v, dev) + float(dt), None) for v in views]
    vw, video_path = None, None
    if video is not None and video is not False:
        from .jpeg_ops import VideoWriter
        video_path = (os.path.join(os.path.dirname(out_path), os.path.basename(os.path.dirname(model_path)) + "_flows.avi")
                      if video is True else os.fspath(video))
        vw = VideoWriter(video_path, 120)                    # (render_video's default rate)
    own = writer is None
    start = _time.perf_counter()
    with contextlib.ExitStack() as stack:                    # (its own writers are closed on every way out)
        w = stack.enter_context(PngWriter()) if own else writer
        if vw is not None:
            stack.enter_context(vw)
        for i, (view, t0, t1, view1) in enumerate(frames):
            res = render_flow(view, gaussians, pipeline, iteration, t0, t1, view1=view1, alpha_min=alpha_min)
            image = colorize(res.flow, res.valid, max_flow)
            w.submit(image, os.path.join(out_path, "{0:05d}.png".format(i)))
            if vw is not None:
                vw.submit([image])
            if save_flo:
                write_flo(os.path.join(out_path, "{0:05d}.flo".format(i)), res.flow)
    if not own:
        torch.cuda.synchronize(dev)                          # (a caller's writer: its files are complete after its close())
    stats = {"frames": len(frames), "seconds": _time.perf_counter() - start}
    if vw is not None:
        stats["video"] = video_path
    return out_path, stats



# ---- depth renders (depth_ops) ------------------------------------------------------------------------------------------------------
def render_depths(model_path, name, iteration, views, gaussians, pipeline, background, mode="disparity", near=None, far=None, alpha_min=1e-3,
                  normals=False, save_pfm=False, save_ply=False, writer=None, video=False):
    """Opt-in (no other loop calls it): the depth map of every view at its own time as a colour-mapped picture (depth_ops.colorize
    with feature_vis.jet_lut; pixels without a valid depth are black) to eval/<name>/ours_<iteration>/depths/%05d.png.  mode: "disparity"
    (1 / depth, the usual picture) or "depth"; near / far: the values of that quantity at the two ends of the colour table, both or
    neither -- without them every frame is scaled by its own smallest and largest value, so a video wants fixed near / far.
    normals: also the camera-space normals (depth_ops.normals, n * 0.5 + 0.5) to a sibling normals/%05d.png.  save_pfm: also %05d.pfm
    beside every depth picture (one read of the device per frame, only then).  save_ply: also the visible surface as world points to
    points/%05d.ply (io_formats.save_point_cloud_ply), coloured by an ordinary render() of the same view over `background` -- one more
    render and the reads of the cloud per frame, only then.  video: True for ours_<iteration>/<basename(dirname(model_path))>_depths.avi,
    or a path: the depth pictures also go, in order, into a Motion-JPEG video as render_video's do, and the statistics gain "video".
    The depth itself is composited over zero whatever `background` is.  writer: a PngWriter of the caller's (it closes it).
    Returns (the depths directory, {"frames", "seconds"})."""
    from . import depth_ops
    from .renderer import render
    import contextlib
    root = os.path.join(model_path, "eval", name, "ours_{}".format(iteration))
    out_path = os.path.join(root, "depths")
    os.makedirs(out_path, exist_ok=True)
    if normals:
        os.makedirs(os.path.join(root, "normals"), exist_ok=True)
    dev = background.device
    views = [_cam(v) for v in views]
    vw, video_path = None, None
    if video is not None and video is not False:
        from .jpeg_ops import VideoWriter
        video_path = (os.path.join(root, os.path.basename(os.path.dirname(model_path)) + "_depths.avi") if video is True else os.fspath(video))
        vw = VideoWriter(video_path, 120)                    # (render_video's default rate)
    own = writer is None
    start = _time.perf_counter()
    with contextlib.ExitStack() as stack:                    # (its own writers are closed on every way out)
        w = stack.enter_context(PngWriter()) if own else writer
        if vw is not None:
            stack.enter_context(vw)
        for i, view in enumerate(views):
            t = _time_of(view, dev)
            res = depth_ops.render_depth(view, gaussians, pipeline, iteration, time=t, alpha_min=alpha_min)
            image = depth_ops.colorize(res.depth, res.valid, mode, near, far)
            w.submit(image, os.path.join(out_path, "{0:05d}.png".format(i)))
            if vw is not None:
                vw.submit([image])
            if normals:
                n, nvalid = depth_ops.normals(res.depth, res.valid, view)
                w.submit(depth_ops.normals_image(n, nvalid), os.path.join(root, "normals", "{0:05d}.png".format(i)))
            if save_pfm:
                depth_ops.write_pfm(os.path.join(out_path, "{0:05d}.pfm".format(i)), res.depth)
            if save_ply:
                from .io_formats import save_point_cloud_ply
                with torch.no_grad():
                    colour = render(view, gaussians, pipeline, background, time=t, it=iteration)["render"]
                points, colors = depth_ops.unproject(res.depth, res.valid, view, image=colour.detach())
                save_point_cloud_ply(os.path.join(root, "points", "{0:05d}.ply".format(i)), points.cpu().numpy(), colors.cpu().numpy())
    if not own:
        torch.cuda.synchronize(dev)                          # (a caller's writer: its files are complete after its close())
    stats = {"frames": len(views), "seconds": _time.perf_counter() - start}
    if vw is not None:
        stats["video"] = video_path
    return out_path, stats


# ---- mesh sequences (tsdf_ops) ------------------------------------------------------------------------------------------------------
def render_meshes(model_path, name, iteration, views, gaussians, pipeline, background, times=None, resolution=256, bounds=None,
                  voxel_size=None, alpha_min=0.5, smooth=0, smooth_method="taubin", smooth_boundary="fixed", topology_report=False, color=True, weld=False,
                  simplify_voxel=None, simplify_contraction="average", min_triangles=None, keep_largest=None, normals=False):
    """Opt-in (no other loop calls it): one watertight mesh per time step, from the same cameras, to
    eval/<name>/ours_<iteration>/meshes/%05d.ply (io_formats.save_mesh_ply).  For every time, ALL `views` are rendered at that time
    -- depth (depth_ops.render_depth) and, with color, an ordinary render over `background` -- fused into one TSDF volume and
    extracted (tsdf_ops.fuse).  times: default the distinct times of the views, in their order of first appearance.  resolution,
    bounds, voxel_size, alpha_min: as tsdf_ops.fuse takes them; without bounds every frame takes its own from the Gaussians at its
    time, so a sequence that is to share one grid wants fixed bounds.  Per frame the device is read for the mesh's two sizes, the
    bounds' six floats and the mesh itself.  Returns (the meshes directory, {"frames", "seconds", "vertices", "faces"}), the last
    two as lists with one number per frame.  min_triangles, keep_largest, normals: with any of them, every mesh goes through
    mesh_ops (components, filter_components with the two criteria, vertex_normals of what is left where normals is set -- written as
    float nx ny nz) before it is written, "vertices" and "faces" count what is written and the dict gains "components", the
    components of every frame's mesh before the filter; with all three off the files are byte for byte what they were.
    weld, simplify_voxel, simplify_contraction: with weld set or a simplify_voxel given, every fused mesh goes through
    mesh_simplify before the cleanup -- weld first (bit-equal vertices merged, collapsed and doubled faces dropped), then simplify
    on a grid of side simplify_voxel with that contraction; where `bounds` is given the same box is simplify's, so that a sequence
    shares one grid and simplify reads the device once a frame.  The dict then gains "fused_vertices" and "fused_faces", the
    sizes before; "vertices" and "faces" count what is written.  With both off the files are byte for byte what they were.
    smooth, smooth_method, smooth_boundary: with smooth > 0 every mesh goes through mesh_smooth.smooth (that many iterations of
    "taubin" or "laplacian", the boundary "fixed" or "free", the colours untouched) after the simplification and the cleanup and
    before the normals, so that normals=True writes the normals of the smoothed surface.  topology_report: one row per time step --
    mesh_smooth.edges' stats of the mesh as written: edges, boundary, non-manifold and inconsistent edges, the Euler characteristic,
    watertight -- goes to mesh_topology.json beside the meshes directory's files and the dict gains "topology".  Either costs one
    read of the device a frame (the eight counts; both share it).  With smooth=0 and no report the files are byte for byte what
    they were."""
    from . import tsdf_ops
    from .io_formats import save_mesh_ply, save_mesh_ply_normals
    cleanup = min_triangles is not None or keep_largest is not None or bool(normals)
    lighter = bool(weld) or simplify_voxel is not None
    root = os.path.join(model_path, "eval", name, "ours_{}".format(iteration))
    out_path = os.path.join(root, "meshes")
    os.makedirs(out_path, exist_ok=True)
    views = [_cam(v) for v in views]
    if times is None:
        times = []
        for v in views:
            t = float(np.asarray(v.time, dtype=np.float32).reshape(-1)[0])
            if t not in times:
                times.append(t)
    start = _time.perf_counter()
    stats = {"frames": 0, "seconds": 0.0, "vertices": [], "faces": []}
    if lighter:
        from . import mesh_simplify
        stats["fused_vertices"], stats["fused_faces"] = [], []
    if cleanup:
        from . import mesh_ops
        stats["components"] = []
    if smooth or topology_report:
        from . import mesh_smooth
    if topology_report:
        stats["topology"] = []
    for i, t in enumerate(times):
        mesh = tsdf_ops.fuse(views, gaussians, pipeline, iteration, time=t, bounds=bounds, voxel_size=voxel_size, resolution=resolution,
                             alpha_min=alpha_min, background=background, color=color)
        if lighter:
            stats["fused_vertices"].append(int(mesh.vertices.shape[0]))
            stats["fused_faces"].append(int(mesh.faces.shape[0]))
            if weld:
                mesh = mesh_simplify.weld(mesh).mesh
            if simplify_voxel is not None:
                mesh = mesh_simplify.simplify(mesh, simplify_voxel, contraction=simplify_contraction, bounds=bounds).mesh
        if cleanup:
            comps = mesh_ops.connected_components(mesh.faces, mesh.vertices.shape[0])
            mesh = mesh_ops.filter_components(mesh, min_triangles=min_triangles, keep_largest=keep_largest, components=comps).mesh
            stats["components"].append(int(comps.labels.shape[0]))
        if smooth or topology_report:
            topology = mesh_smooth.edges(mesh.faces, mesh.vertices.shape[0])
            if smooth:
                mesh = mesh_smooth.smooth(mesh, iterations=smooth, method=smooth_method, boundary=smooth_boundary, topology=topology).mesh
            if topology_report:
                stats["topology"].append(dict(topology.stats, frame=i, time=float(t)))
        if cleanup:
            save_mesh_ply_normals(os.path.join(out_path, "{0:05d}.ply".format(i)), mesh.vertices, mesh.faces,
                                  mesh_ops.vertex_normals(mesh.vertices, mesh.faces) if normals else None, mesh.colors)
        else:
            save_mesh_ply(os.path.join(out_path, "{0:05d}.ply".format(i)), mesh.vertices, mesh.faces, mesh.colors)
        stats["frames"] += 1
        stats["vertices"].append(int(mesh.vertices.shape[0]))
        stats["faces"].append(int(mesh.faces.shape[0]))
    if topology_report:
        with open(os.path.join(out_path, "mesh_topology.json"), "w") as fp:
            json.dump(stats["topology"], fp, indent=1)
    stats["seconds"] = _time.perf_counter() - start
    return out_path, stats


# ---- mesh pictures (mesh_render) ----------------------------------------------------------------------------------------------------
def render_mesh_views(model_path, name, iteration, views, gaussians, pipeline, background, meshes=None, mode="shaded", compare=False, writer=None,
                      video=False, **fuse):
    """Opt-in (no other loop calls it): the mesh of every view's time, drawn from that view by the triangle rasterizer
    (mesh_render.render_mesh: mode "shaded", "color", "normals" or "depth"; pixels without a surface are black) to
    eval/<name>/ours_<iteration>/mesh_views/%05d.png.  meshes: {time: a tsdf_ops.Mesh}, for instance what a cleanup or a
    simplification left; without it every distinct time is fused once from ALL `views` (tsdf_ops.fuse with the keywords `fuse`:
    resolution, bounds, voxel_size, alpha_min, ... over `background`) and kept for the views that share it.  compare: also, per view,
    one depth_ops.render_depth of the Gaussians and mesh_render.agreement of the mesh depth with it -- the standard depth errors over
    the pixels both cover, the IoU of the two masks -- as one dict per view in the statistics' "agreement" (one read of the device
    per view, only then).  video: True for ours_<iteration>/<basename(dirname(model_path))>_mesh_views.avi, or a path: the pictures
    also go, in order, into a Motion-JPEG video as render_video's do, and the statistics gain "video".  writer: a PngWriter of the
    caller's (it closes it).  Returns (the mesh_views directory, {"frames", "seconds"})."""
    from . import depth_ops, mesh_render, tsdf_ops
    import contextlib
    root = os.path.join(model_path, "eval", name, "ours_{}".format(iteration))
    out_path = os.path.join(root, "mesh_views")
    os.makedirs(out_path, exist_ok=True)
    dev = background.device
    views = [_cam(v) for v in views]
    time_key = lambda v: float(np.asarray(v.time, dtype=np.float32).reshape(-1)[0])          # noqa: E731
    kept = {float(np.float32(t)): m for t, m in meshes.items()} if meshes is not None else {}
    vw, video_path = None, None
    if video is not None and video is not False:
        from .jpeg_ops import VideoWriter
        video_path = (os.path.join(root, os.path.basename(os.path.dirname(model_path)) + "_mesh_views.avi") if video is True else os.fspath(video))
        vw = VideoWriter(video_path, 120)                    # (render_video's default rate)
    own = writer is None
    rows = []
    start = _time.perf_counter()
    with contextlib.ExitStack() as stack:                    # (its own writers are closed on every way out)
        w = stack.enter_context(PngWriter()) if own else writer
        if vw is not None:
            stack.enter_context(vw)
        for i, view in enumerate(views):
            t = time_key(view)
            if t not in kept:
                if meshes is not None:
                    raise KeyError(f"render_mesh_views: no mesh for time {t!r} (meshes holds {sorted(kept)})")
                kept[t] = tsdf_ops.fuse(views, gaussians, pipeline, iteration, time=t, background=background, **fuse)
            mesh = kept[t]
            raster = mesh_render.rasterize(mesh, view)
            image = mesh_render.render_mesh(mesh, view, mode=mode, raster=raster)
            w.submit(image, os.path.join(out_path, "{0:05d}.png".format(i)))
            if vw is not None:
                vw.submit([image])
            if compare:
                res = depth_ops.render_depth(view, gaussians, pipeline, iteration, time=_time_of(view, dev))
                rows.append(mesh_render.agreement(raster, res))
    if not own:
        torch.cuda.synchronize(dev)                          # (a caller's writer: its files are complete after its close())
    stats = {"frames": len(views), "seconds": _time.perf_counter() - start}
    if compare:
        stats["agreement"] = rows
    if vw is not None:
        stats["video"] = video_path
    return out_path, stats


def mesh_motion(meshes, n=100000, thresholds=None, seed=0, device="cuda", surface=False):
    """Opt-in (no other loop calls it): how far the surface moves from one time step to the next.  meshes: the meshes directory a
    render_meshes call returned (its %05d.ply files, in order), or a sequence of meshes ((vertices, faces, ...) on the device).
    Returns one geometry_ops.mesh_distance row per consecutive pair -- mesh k as the prediction, mesh k + 1 as the ground truth, n
    surface samples each, one read of the device per pair -- with its "frames" (k, k + 1), and under "mean" their mean:
    {"rows": [...], "mean": {...}}.  surface=True: every pair through mesh_distance(..., surface=True), the samples of each mesh
    against the other mesh's surface; surface="signed": the signed columns of sdf_ops.signed_surface_distance with them (a positive
    signed_accuracy: the surface at step k lies outside the one at step k + 1)."""
    from . import geometry_ops
    from .io_formats import read_mesh_ply
    thresholds = geometry_ops.THRESHOLDS if thresholds is None else thresholds
    if isinstance(meshes, (str, os.PathLike)):
        names = sorted(f for f in os.listdir(meshes) if len(f) == 9 and f.endswith(".ply") and f[:5].isdigit())
        loaded = []
        for f in names:
            vertices, faces = read_mesh_ply(os.path.join(meshes, f))[:2]
            loaded.append((torch.as_tensor(vertices, dtype=torch.float32).to(device), torch.as_tensor(faces, dtype=torch.int32).to(device)))
        meshes = loaded
    meshes = list(meshes)
    rows = []
    for k in range(len(meshes) - 1):
        row = geometry_ops.mesh_distance(meshes[k], meshes[k + 1], n=n, seed=seed, thresholds=thresholds, surface=surface)
        row["frames"] = (k, k + 1)
        rows.append(row)
    mean = geometry_ops.mean_row([{key: v for key, v in r.items() if key != "frames"} for r in rows])
    return {"rows": rows, "mean": mean}
