#!/usr/bin/env python
"""Generates tests/golden/lpips.npz by RUNNING the reference's own lpipsPyTorch.modules classes -- BaseNet.forward (z_score, the
tap loop), normalize_activation, LinLayers and LPIPS.forward -- on the seeded weights and images of tests/lpips_ref.py, in float64
on the CPU.  Needs a checkout of the reference (`python tests/golden/make_lpips_vectors.py <reference root>`, or GP_REFERENCE_ROOT).

Nothing is downloaded: `torchvision` and `torchvision.models` are registered as empty stub modules before the import, the network and
LPIPS objects are created with __new__ (their __init__ would fetch weights), and `layers` is the recipe's nn.Sequential.  Only data
is written: target_layers / n_channels_list of AlexNet and VGG16 read from networks.py with ast, the mean / std buffers, per case
the float64 LPIPS and the five layer terms, and checksums of the seeded images and weights."""
import ast
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GP_REFERENCE_ROOT", "")
OUT = os.path.dirname(os.path.abspath(__file__))


def class_lists(path):
    """{class name: {"target_layers": [...], "n_channels_list": [...]}} from the assignments in each class's __init__."""
    out = {}
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.ClassDef):
            for a in ast.walk(node):
                if isinstance(a, ast.Assign) and isinstance(a.targets[0], ast.Attribute) and a.targets[0].attr in ("target_layers", "n_channels_list"):
                    out.setdefault(node.name, {})[a.targets[0].attr] = ast.literal_eval(a.value)
    return out


def main():
    if not os.path.isdir(os.path.join(REF, "lpipsPyTorch", "modules")):
        sys.exit("usage: make_lpips_vectors.py <reference root>   (or set GP_REFERENCE_ROOT)")
    sys.path.insert(0, os.path.dirname(OUT))
    import lpips_ref as R
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.models", tv.models)
    sys.path.insert(0, REF)
    from lpipsPyTorch.modules import lpips as ref_lpips, networks as ref_networks
    lists = class_lists(os.path.join(REF, "lpipsPyTorch", "modules", "networks.py"))
    out = {}
    for net_type, cls_name in (("alex", "AlexNet"), ("vgg", "VGG16")):
        cls = getattr(ref_networks, cls_name)
        w = R.seeded_weights(net_type)
        net = cls.__new__(cls)
        ref_networks.BaseNet.__init__(net)                 # (the mean / std buffers)
        net.layers = R.sequential(net_type, w, torch.float32)
        net.target_layers = lists[cls_name]["target_layers"]
        net.n_channels_list = lists[cls_name]["n_channels_list"]
        lin = ref_networks.LinLayers(net.n_channels_list)
        lin.load_state_dict(w["lin"])
        model = ref_lpips.LPIPS.__new__(ref_lpips.LPIPS)
        nn.Module.__init__(model)
        model.net, model.lin = net, lin
        model = model.double()
        out[f"{net_type}_target_layers"] = np.asarray(net.target_layers, dtype=np.int64)
        out[f"{net_type}_n_channels_list"] = np.asarray(net.n_channels_list, dtype=np.int64)
        out[f"{net_type}_mean"] = net.mean.double().numpy().reshape(3)      # (float32 values, widened)
        out[f"{net_type}_std"] = net.std.double().numpy().reshape(3)
        out[f"{net_type}_weights_sum"] = np.float64(R.weights_checksum(w))
        for k, (H, W) in enumerate(R.SIZES):
            render, gt = R.case_pair(k)
            x, y = torch.from_numpy(render).double()[None], torch.from_numpy(gt).double()[None]
            with torch.no_grad():
                total = model(x, y)                        # LPIPS.forward
                fx, fy = model.net(x), model.net(y)        # BaseNet.forward
                terms = [l((a - b) ** 2).mean((2, 3), True).reshape(()) for a, b, l in zip(fx, fy, model.lin)]
            tag = f"{net_type}_c{k}_"
            out[tag + "size"] = np.asarray((H, W), dtype=np.int64)
            out[tag + "render_sum"], out[tag + "gt_sum"] = render.sum(dtype=np.float64), gt.sum(dtype=np.float64)
            out[tag + "lpips"] = np.float64(total.reshape(()).item())
            out[tag + "terms"] = np.asarray([float(t) for t in terms], dtype=np.float64)
    np.savez(os.path.join(OUT, "lpips.npz"), **out)
    print({k: (v.tolist() if getattr(v, "ndim", 0) else float(v)) for k, v in out.items()})


if __name__ == "__main__":
    main()
