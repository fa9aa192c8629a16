"""Image metrics on the device: L1, MSE, PSNR (both call shapes of the reference), SSIM, MS-SSIM and D-SSIM of rendered views
against their ground truth in ONE call of libgp_hip.so (gp_image_metrics, csrc/metric_kernels.hip), and evaluation loops over it
that never read a number back per view.

  [REF metrics.py:138-147]  ssim, psnr on [1,3,H,W], ms_ssim(data_range=1), D-SSIM = (1 - MS-SSIM) / 2, the error image
  [REF train.py:107,252-282] psnr on [3,H,W] followed by .mean(); the clamped L1 / PSNR means of training_report
  [REF utils/loss_utils.py:54-98, utils/image_utils.py:18-20]

MS-SSIM follows the published five-scale form as pytorch_msssim computes it; that package is absent here, so parity with it is
unpinned (the definition is restated in include/gp_hip.h and checked against a float64 torch restatement in the tests).
LPIPS (the AlexNet and VGG16 backbones) lives in lpips.py and is re-exported here: `LPIPS`, `lpips`, `find_lpips_weights`; the caller
supplies the pretrained weight files, this package ships none and never fetches any.  The evaluation loops take it as an option
(`evaluate_views(lpips=[...])`, `evaluate_dirs(lpips_weights=...)`) and then report the reference's LPIPS-vgg / LPIPS-alex keys
[REF metrics.py:144-145, 157-162].  HIP only: CPU tensors raise."""
from __future__ import annotations

import json
import os
from types import SimpleNamespace

import torch

from . import _lib
from .lpips import LPIPS, find_lpips_weights, lpips  # noqa: F401  (re-exported)

NAMES = ("L1", "MSE", "PSNR", "PSNR_CH", "SSIM", "MS_SSIM", "D_SSIM", "reserved")
L1, MSE, PSNR, PSNR_CH, SSIM, MS_SSIM, D_SSIM = range(7)
METRIC_COUNT = 8
QUANTIZE8, CLAMP01, WITH_MS_SSIM = 1, 2, 4      # GP_METRICS_* of include/gp_hip.h

_scratch: dict = {}


def metrics_scratch(device, B, H, W, flags):
    """One scratch buffer per (device, stream, shape, flags): the calls on a stream are ordered, so the buffer is reused."""
    key = (device.index, _lib.stream_ptr(device).value, B, H, W, flags)
    t = _scratch.get(key)
    if t is None:
        t = _lib.scratch(_lib.lib().gp_image_metrics_scratch_bytes, B, H, W, flags, device=device, extra=256)
        if len(_scratch) >= 16:
            _scratch.pop(next(iter(_scratch)))
        _scratch[key] = t
    return t


def _as_batch(x, name):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError(f"image_metrics: {name} must be a GPU tensor -- HIP kernels only (no CPU fallback)")
    x = x.detach()
    if x.dim() == 3:
        x = x[None]
    if x.dim() != 4 or x.shape[1] != 3:
        raise RuntimeError(f"image_metrics: {name} must be [B,3,H,W] or [3,H,W] (got {tuple(x.shape)})")
    return x.to(torch.float32).contiguous()


def image_metrics(render, gt, *, quantize8=False, clamp=False, ms_ssim=True, out=None, invalid_flag=None, levels=False,
                  quantized=False, deltas=False):
    """Metrics of render against gt ([B,3,H,W] or [3,H,W], any float dtype: converted to contiguous float32).  Returns a namespace:
      table      [B,8] float64 on the device, columns `names` (L1, MSE, PSNR, PSNR_CH, SSIM, MS_SSIM, D_SSIM, reserved); nothing is
                 read back.  `out=` (a [B,8] float64 contiguous view, e.g. rows of a caller's table) receives it instead.
      levels     [B,5,3] float64 (levels=True): mean cs of scales 1-4 and mean ssim of scale 5 per channel, before the ReLU
      quantized  [B,3,H,W] uint8 (quantized=True, needs quantize8): the 8-bit render
      deltas     [B,H,W,3] uint8 (deltas=True): trunc(|render - gt| * 255), the error image of metrics.py:146-147
    quantize8: the render goes through an 8-bit image file first (floor(x * 255 + 0.5) clamped, / 255), as every render does before
    the reference's metrics.py sees it.  clamp: both images clamped to [0, 1] (training_report).  ms_ssim=False skips the four
    further pyramid levels (columns 5, 6 are NaN); with it min(H, W) must exceed 160, as pytorch_msssim asserts.
    invalid_flag: optional device word per image (int32 / uint32 [B]); non-zero turns that row into NaN."""
    a, b = _as_batch(render, "render"), _as_batch(gt, "gt")
    if a.shape != b.shape or a.device != b.device:
        raise RuntimeError(f"image_metrics: render {tuple(a.shape)} on {a.device} and gt {tuple(b.shape)} on {b.device} differ")
    dev = a.device
    B, _, H, W = a.shape
    flags = (QUANTIZE8 if quantize8 else 0) | (CLAMP01 if clamp else 0) | (WITH_MS_SSIM if ms_ssim else 0)
    if levels and not ms_ssim:
        raise RuntimeError("image_metrics: levels=True needs ms_ssim=True")
    if quantized and not quantize8:
        raise RuntimeError("image_metrics: quantized=True needs quantize8=True")
    if out is None:
        table = torch.empty(B, METRIC_COUNT, dtype=torch.float64, device=dev)
    else:
        table = out
        if table.dtype != torch.float64 or table.device != dev or tuple(table.shape) != (B, METRIC_COUNT) or not table.is_contiguous():
            raise RuntimeError(f"image_metrics: out must be a contiguous [{B},{METRIC_COUNT}] float64 tensor on {dev}")
    if invalid_flag is not None:
        if invalid_flag.device != dev or invalid_flag.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or invalid_flag.numel() != B \
                or not invalid_flag.is_contiguous():
            raise RuntimeError(f"image_metrics: invalid_flag must be {B} contiguous 32-bit words on {dev}")
    lv = torch.empty(B, 5, 3, dtype=torch.float64, device=dev) if levels else None
    qo = torch.empty(B, 3, H, W, dtype=torch.uint8, device=dev) if quantized else None
    do = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev) if deltas else None
    with _lib.on_device(dev):
        scratch = metrics_scratch(dev, B, H, W, flags)
        sp = (scratch.data_ptr() + 255) & ~255
        rc = _lib.lib().gp_image_metrics(a, b, B, 3, H, W, flags, sp, invalid_flag, table, lv, qo, do, _lib.stream_ptr(dev))
        _lib.check(rc, "gp_image_metrics")
    return SimpleNamespace(table=table, names=NAMES, levels=lv, quantized=qo, deltas=do)


def psnr(img, gt):
    """[B] (or a scalar tensor for [3,H,W]) float64: PSNR over all three channels, `psnr()` of the reference on [1,3,H,W]."""
    t = image_metrics(img, gt, ms_ssim=False).table[:, PSNR]
    return t[0] if img.dim() == 3 else t


def ms_ssim(img, gt):
    """[B] (or a scalar tensor for [3,H,W]) float64: MS-SSIM with data_range 1 (parity with pytorch_msssim is unpinned)."""
    t = image_metrics(img, gt, ms_ssim=True).table[:, MS_SSIM]
    return t[0] if img.dim() == 3 else t


def _times(cameras, times, dev):
    if times is not None:
        return list(times)
    return [torch.as_tensor(getattr(c, "time", 0.0), dtype=torch.float32, device=dev).reshape(1) for c in cameras]


def evaluate_views(model, cameras, gts, pipe, bg, iteration, *, quantize8=True, ms_ssim=True, speculative=True, clamp=False,
                   times=None, renderer=None, lpips=None):
    """Render every camera and score it against gts[v] ([3,H,W]) without a host read per view: the frames go through
    `SpeculativeRenderer`, each frame's metrics call takes that frame's overflow word as `invalid_flag`, and the [V,8] table is read
    ONCE at the end.  A ring of frames ends in one `flush()`; only if that flush had to re-render frames (their rows are NaN) are
    the ring's rows looked at, and the NaN ones recomputed from the replaced images.  speculative=False renders every frame with
    `render()` in its exact mode (one synchronisation inside each).  Returns {"summary": {"SSIM", "PSNR", "MS-SSIM", "D-SSIM",
    "L1": means over the views, the reference's key names [REF metrics.py:157-162]}, "per_view": the [V,8] float64 device table,
    "rerendered": frames rendered again}.
    lpips: a list of `LPIPS` objects.  Each frame's LPIPS call takes the same overflow word and the same quantised render as its
    metrics call, its rows stay on the device until the one read at the end, and rows redone after an overflow are redone for LPIPS
    too; the summary gains "LPIPS-vgg" / "LPIPS-alex" and the result "per_view_lpips": {net_type: the [V,8] device table}."""
    nets = list(lpips or [])
    table, m, again, ltabs = _score_views(model, cameras, gts, pipe, bg, iteration, speculative, times, renderer,
                                          dict(quantize8=quantize8, ms_ssim=ms_ssim, clamp=clamp), nets)
    summary = {"SSIM": float(m[SSIM]), "PSNR": float(m[PSNR]), "MS-SSIM": float(m[MS_SSIM]), "D-SSIM": float(m[D_SSIM]), "L1": float(m[L1])}
    result = {"summary": summary, "per_view": table, "rerendered": again}
    if nets:
        host = torch.stack([t[:, 0] for t in ltabs]).cpu()           # (one read for all the nets)
        for k, net in enumerate(nets):
            summary[f"LPIPS-{net.net_type}"] = float(host[k].mean())
        result["per_view_lpips"] = {net.net_type: t for net, t in zip(nets, ltabs)}
    return result


def _score_views(model, cameras, gts, pipe, bg, iteration, speculative, times, renderer, kw, nets=()):
    """The loop behind evaluate_views / report_views: (the [V,8] device table, its column means from the ONE host read, frames
    rendered again, one [V,8] device table per LPIPS object of `nets`)."""
    from .renderer import SpeculativeRenderer, render
    dev = bg.device
    V = len(cameras)
    if len(gts) != V:
        raise RuntimeError(f"evaluate_views: {V} cameras but {len(gts)} ground-truth images")
    times = _times(cameras, times, dev)
    table = torch.full((V, METRIC_COUNT), float("nan"), dtype=torch.float64, device=dev)
    ltabs = [torch.full((V, METRIC_COUNT), float("nan"), dtype=torch.float64, device=dev) for _ in nets]
    again = 0

    def score(img, row, flag):
        image_metrics(img, gts[row], out=table[row:row + 1], invalid_flag=flag, **kw)
        for net, lt in zip(nets, ltabs):
            net(img, gts[row], quantize8=kw["quantize8"], out=lt[row:row + 1], invalid_flag=flag)

    with torch.no_grad():
        if not speculative:
            for v in range(V):
                img = render(cameras[v], model, pipe, bg, time=times[v], it=iteration)["render"]
                score(img, v, None)
        else:
            sr = renderer if renderer is not None else SpeculativeRenderer(model, pipe, bg)
            sr.flush()          # (a caller's renderer: its ring starts empty, so ring and rows stay in step)
            ring = []           # (row, image) of the frames since the last flush

            def close_ring():
                nonlocal again, ring
                n = sr.flush()
                if n:
                    lo, hi = ring[0][0], ring[-1][0] + 1
                    bad = torch.isnan(table[lo:hi, L1]).cpu()       # (only after an overflow: the rows to do again)
                    for row, img in ring:
                        if bool(bad[row - lo]):
                            score(img, row, None)
                    again += n
                ring = []

            for v in range(V):
                if len(ring) >= sr.slots:
                    close_ring()
                img = sr(cameras[v], time=times[v], it=iteration)["render"]
                st = sr.last_status
                score(img, v, None if st is None else st[1:2])
                if st is not None:
                    ring.append((v, img))
            close_ring()
    return table, table.cpu().mean(dim=0), again, ltabs


def report_views(model, cameras, gts, pipe, bg, iteration, *, speculative=True, times=None, renderer=None):
    """The `training_report` form [REF train.py:252-282]: both images clamped to [0, 1], no quantisation, no MS-SSIM; returns
    {"L1": mean L1, "PSNR": mean over the views of the per-channel-mean PSNR, "per_view": the table}."""
    table, m, _, _ = _score_views(model, cameras, gts, pipe, bg, iteration, speculative, times, renderer,
                               dict(quantize8=False, ms_ssim=False, clamp=True))
    return {"L1": float(m[L1]), "PSNR": float(m[PSNR_CH]), "per_view": table}


def _load_rgb(path, device, resize=None):
    """An image file as `to_tensor` gives it: [1,3,H,W] float32 = byte / 255 (true division), first three channels.  resize (a
    callable (w, h) -> (width, height)): the decoded bytes, all channels, go up and are resized on the device as Image.resize does
    it (resize_ops.resize), before the slice -- the order of the reference's readImages."""
    from PIL import Image       # (lazy: only the directory form needs it)
    import numpy as np
    arr = np.array(Image.open(path))
    if arr.ndim == 2:
        arr = arr[:, :, None]
    t = torch.from_numpy(arr).permute(2, 0, 1)
    if t.dtype != torch.uint8:
        raise RuntimeError(f"evaluate_dirs: {path} is not an 8-bit image")
    if resize is not None:
        from . import resize_ops
        if t.shape[0] not in (1, 3, 4):
            raise RuntimeError(f"evaluate_dirs: {path} has {t.shape[0]} channels: L, RGB and RGBA images are resized on the device")
        size = resize_ops.target_size(resize, t.shape[2], t.shape[1], path)
        return resize_ops.resize(t.contiguous().to(device), size, dtype=torch.float32)[None, :3].contiguous()
    return (t[:3].to(torch.float32) / 255.0)[None].contiguous().to(device)


def _lpips_from(weights, device):
    """evaluate_dirs' `lpips_weights`: a directory holding the four weight files, or a dict {"vgg": w, "alex": w} with w a
    directory, a (backbone, lin) pair or {"backbone": ..., "lin": ...} -> [LPIPS vgg, LPIPS alex] (the nets the dict names)."""
    from . import lpips as _lp
    if isinstance(weights, dict):
        return [_lp.cached(net, device, weights[net]) for net in ("vgg", "alex") if net in weights]
    return [_lp.cached(net, device, os.fspath(weights)) for net in ("vgg", "alex")]


def _decode_by_signature(paths, device, sync=False, resize=None):
    """evaluate_dirs' device_decode: every file goes by its first bytes to png_decode or jpeg_decode (float32, the first three
    channels); one call of each per group.  Anything else raises, naming the file: there is no host decoder behind this path."""
    from . import jpeg_decode, png_decode
    kinds = {"png": ([], []), "jpeg": ([], [])}
    for i, path in enumerate(paths):
        with open(path, "rb") as fp:
            data = fp.read()
        if data[:8] == png_decode.SIGNATURE:
            kind = "png"
        elif data[:2] == b"\xff\xd8":
            kind = "jpeg"
        else:
            raise RuntimeError(f"evaluate_dirs: {path} is neither a PNG nor a JPEG file (device_decode reads these two)")
        kinds[kind][0].append(i)
        kinds[kind][1].append(data)
    out = [None] * len(paths)
    for kind, (idx, files) in kinds.items():
        if not files:
            continue
        names = [paths[i] for i in idx]
        if kind == "png":
            imgs = png_decode.decode(files, device=device, dtype=torch.float32, channels=3, names=names, resize=resize)
        else:
            imgs = jpeg_decode.decode(files, device=device, dtype=torch.float32, names=names, sync=sync, resize=resize)
        for i, im in zip(idx, imgs):
            out[i] = im
    return out


def _score_decoded_groups(rdir, gdir, rnames, gnames, mdir, device, table, nets, ltabs, write, jw, pending, group, by_signature=False, sync=False,
                          resize=None):
    """evaluate_dirs' loop with device_png: `group` pairs per png_decode.decode_files call (float32, the first three channels), and
    one batched image_metrics call per run of pairs of one shape.  by_signature (device_decode): PNG and JPEG files, each to its
    decoder."""
    from . import png_decode
    for lo in range(0, len(rnames), group):
        hi = min(len(rnames), lo + group)
        paths = [os.path.join(rdir, n) for n in rnames[lo:hi]] + [os.path.join(gdir, n) for n in gnames[lo:hi]]
        imgs = _decode_by_signature(paths, device, sync, resize) if by_signature else \
            png_decode.decode_files(paths, device=device, dtype=torch.float32, channels=3, resize=resize)
        renders, gts = imgs[:hi - lo], imgs[hi - lo:]
        i = lo
        while i < hi:
            j = i + 1
            while j < hi and renders[j - lo].shape == renders[i - lo].shape and gts[j - lo].shape == gts[i - lo].shape:
                j += 1
            render, gt = torch.stack(renders[i - lo:j - lo]), torch.stack(gts[i - lo:j - lo])
            r = image_metrics(render, gt, out=table[i:j], deltas=write)
            for k in range(i, j):
                for net, lt in zip(nets, ltabs):
                    net(render[k - i:k - i + 1], gt[k - i:k - i + 1], out=lt[k:k + 1])
            if jw is not None:
                jw.submit(r.deltas.permute(0, 3, 1, 2), [os.path.join(mdir, "deltas", "{0:05d}.jpg".format(k)) for k in range(i, j)])
            elif write:
                pending += [r.deltas[k - i:k - i + 1] for k in range(i, j)]
            i = j


def evaluate_dirs(path, device="cuda", write=True, lpips_weights=None, device_jpeg=False, device_png=False, png_group=16, device_decode=False, decode_sync=False,
                  resize=False, resize_ratio=0.5):
    """The directory form of the reference's metrics.py [REF metrics.py:113-178]: for every `<path>/<method>/` holding `renders/`
    and `gt/`, score the sorted image pairs (files whose name contains "depth" are skipped), write `<method>/deltas/%05d.jpg` and
    -- as the reference does -- `<path>/results.json` and `<path>/per_view.json` of the last method.  Keys: SSIM, PSNR, MS-SSIM,
    D-SSIM; with `lpips_weights` (a directory holding the weight files find_lpips_weights names, or a dict {"vgg": ..., "alex": ...})
    the reference's six in its order: SSIM, PSNR, LPIPS-vgg, LPIPS-alex, MS-SSIM, D-SSIM.  The images were saved as 8 bits already, so nothing is quantised again.  One table read per method.
    device_jpeg: the deltas images are encoded on the device (jpeg_ops.JpegWriter at quality 75, 4:2:0 -- the defaults of the host
    encoder the default path uses) and written behind the loop, instead of one read and one host encode per image.
    device_png: the image pairs are decoded on the device (png_decode.decode_files: float32, the first three channels), `png_group`
    pairs per call, and every run of equal-shaped pairs of a group is scored by one batched image_metrics call, instead of one host
    decode per file; the numbers are the same.
    device_decode: as device_png, but every file goes by its signature to png_decode or to jpeg_decode (baseline JPEG, 4:4:4 or
    4:2:0) -- a gt directory of .jpg frames, or .jpg renders; the numbers are the default path's.  Off by default.
    decode_sync: with device_decode, jpeg_decode.decode's `sync` -- JPEG files without restart markers go through jpeg_sync's many
    lanes; the pixels, and so the numbers, are the same.  Off by default.
    resize, resize_ratio: the reference's options of the same names [REF metrics.py evaluate, readImages] -- with resize=True every
    render and ground-truth image is resized to (int(w * resize_ratio), int(h * resize_ratio)) with Pillow's bicubic filter before it
    is scored, on the device and byte for byte as Image.resize does it (resize_ops): the default path uploads the decoded bytes and
    resizes them there, device_png / device_decode pass `resize=` to the decoders.  The numbers are those of scoring files that
    Pillow resized.  A target size of 0 raises, naming the file.  With resize=False the ratio is ignored.
    Returns {method: {"summary": ..., "per_view": ...}} with the dictionaries that were written."""
    from PIL import Image
    device = torch.device(device)
    nets = _lpips_from(lpips_weights, device) if lpips_weights is not None else []
    ratio = float(resize_ratio)
    target = (lambda w, h: (int(w * ratio), int(h * ratio))) if resize else None
    result = {}
    for method in sorted(os.listdir(path)):
        mdir = os.path.join(path, method)
        rdir, gdir = os.path.join(mdir, "renders"), os.path.join(mdir, "gt")
        if not (os.path.isdir(rdir) and os.path.isdir(gdir)):
            continue
        rnames = [f for f in sorted(os.listdir(rdir)) if "depth" not in f]
        gnames = sorted(os.listdir(gdir))
        if len(rnames) != len(gnames) or not rnames:
            raise RuntimeError(f"evaluate_dirs: {rdir} holds {len(rnames)} images, {gdir} holds {len(gnames)}")
        table = torch.empty(len(rnames), METRIC_COUNT, dtype=torch.float64, device=device)
        ltabs = [torch.empty(len(rnames), METRIC_COUNT, dtype=torch.float64, device=device) for _ in nets]
        if write:
            os.makedirs(os.path.join(mdir, "deltas"), exist_ok=True)
        pending = []
        jw = None
        if write and device_jpeg:
            from .jpeg_ops import JpegWriter
            jw = JpegWriter(quality=75, subsampling="420")
        for i, (rn, gn) in enumerate(zip(rnames, gnames)):
            if device_png or device_decode:
                break                           # (scored in groups below)
            render, gt = _load_rgb(os.path.join(rdir, rn), device, target), _load_rgb(os.path.join(gdir, gn), device, target)
            r = image_metrics(render, gt, out=table[i:i + 1], deltas=write)
            for net, lt in zip(nets, ltabs):
                net(render, gt, out=lt[i:i + 1])
            if jw is not None:
                jw.submit(r.deltas.permute(0, 3, 1, 2), [os.path.join(mdir, "deltas", "{0:05d}.jpg".format(i))])
            elif write:
                pending.append(r.deltas)
        if device_png or device_decode:
            _score_decoded_groups(rdir, gdir, rnames, gnames, mdir, device, table, nets, ltabs, write, jw, pending, max(1, int(png_group)),
                                  by_signature=bool(device_decode), sync=decode_sync, resize=target)
        h = table.cpu() if not nets else torch.cat([table] + [lt[:, :1] for lt in ltabs], dim=1).cpu()      # (one read either way)
        for i, d in enumerate(pending):
            Image.fromarray(d[0].cpu().numpy()).save(os.path.join(mdir, "deltas", "{0:05d}.jpg".format(i)))
        if jw is not None:
            jw.close()
        cols = {"SSIM": SSIM, "PSNR": PSNR}
        cols.update({f"LPIPS-{net.net_type}": METRIC_COUNT + k for k, net in enumerate(nets)})
        cols.update({"MS-SSIM": MS_SSIM, "D-SSIM": D_SSIM})
        summary = {k: float(h[:, c].mean()) for k, c in cols.items()}
        per_view = {k: {n: float(h[i, c]) for i, n in enumerate(rnames)} for k, c in cols.items()}
        result[method] = {"summary": summary, "per_view": per_view}
        if write:
            with open(os.path.join(path, "results.json"), "w") as fp:
                json.dump(summary, fp, indent=True)
            with open(os.path.join(path, "per_view.json"), "w") as fp:
                json.dump(per_view, fp, indent=True)
    return result
