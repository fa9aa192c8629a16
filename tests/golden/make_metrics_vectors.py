#!/usr/bin/env python
"""Generates tests/golden/metrics.npz by RUNNING the reference's own utils/loss_utils.py (l1_loss, ssim) and utils/image_utils.py
(psnr) on seeded image pairs, loaded by file path as make_golden.py does.  Needs a checkout of the reference
(`python tests/golden/make_metrics_vectors.py <reference root>`, or GP_REFERENCE_ROOT) and runs on the CPU.  Only data is written: the numbers the reference returns, and a checksum of each seeded image (tests/metrics_ref.golden_pair rebuilds the images).

Per pair (37 x 45 and 64 x 64): l1_loss and ssim on [3,H,W]; psnr in BOTH call shapes -- [3,H,W] (per channel, as train.py:107
calls it before .mean()) and [1,3,H,W] (over all channels, as metrics.py:141 calls it)."""
import importlib.util
import os
import sys

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GP_REFERENCE_ROOT", "")
OUT = os.path.dirname(os.path.abspath(__file__))


def load_by_path(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    if not os.path.isdir(os.path.join(REF, "utils")):
        sys.exit("usage: make_metrics_vectors.py <reference root>   (or set GP_REFERENCE_ROOT)")
    sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))      # (the extension shims utils/loss_utils.py imports)
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.dirname(OUT))
    from metrics_ref import GOLDEN_SIZES, golden_pair
    lu = load_by_path("ref_loss_utils", "utils/loss_utils.py")
    iu = load_by_path("ref_image_utils", "utils/image_utils.py")
    out = {}
    for k in range(len(GOLDEN_SIZES)):
        img, gt = golden_pair(k)            # (seeded: the file holds their checksums, not the images)
        a, b = torch.from_numpy(img), torch.from_numpy(gt)
        tag = f"p{k}_"
        out[tag + "size"] = np.asarray(GOLDEN_SIZES[k], dtype=np.int64)
        out[tag + "render_sum"], out[tag + "gt_sum"] = img.sum(dtype=np.float64), gt.sum(dtype=np.float64)
        out[tag + "l1"] = np.float64(lu.l1_loss(a, b).item())
        out[tag + "ssim"] = np.float64(lu.ssim(a, b).item())
        out[tag + "psnr_3hw"] = iu.psnr(a, b).numpy().astype(np.float64).reshape(3)
        out[tag + "psnr_13hw"] = np.float64(iu.psnr(a[None], b[None]).item())
    np.savez(os.path.join(OUT, "metrics.npz"), **out)
    print({k: (v.shape if getattr(v, "ndim", 0) else float(v)) for k, v in out.items()})


if __name__ == "__main__":
    main()
