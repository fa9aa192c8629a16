"""Records tests/golden/gcn.npz and tests/golden/gcn_surface.json from the REFERENCE's own classes (motion_model/gcn.py needs only torch
and numpy, and runs on the CPU):

    python tests/golden/make_gcn_vectors.py /path/to/GaussianPrediction

For every configuration of tests/gcn_ref.py the seeded state (gcn_ref.seeded_state; its checksum is recorded) is loaded into the
reference's GCN_xyzr in float64, and recorded are: the train-mode outputs, the loss, every parameter gradient, the input gradients,
the updated running statistics, the losses of 3 Adam steps, and an eval-mode rollout of 12 frames with and without norm_rotation --
in full for the smallest configuration, as sums plus a strided sample for the others (gcn_ref.summarise)."""
import ast
import importlib.util
import inspect
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gcn_ref as R  # noqa: E402


def _load(ref_dir):
    spec = importlib.util.spec_from_file_location("reference_gcn", os.path.join(ref_dir, "motion_model", "gcn.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _operate(args, batch, model):
    """train_GCN.py:19-43 without the noise (the recorded passes use none)."""
    xp, rp = model(batch["xyz_inputs"].permute((0, 3, 2, 1)), batch["rotation_inputs"].permute((0, 3, 2, 1)))
    xp, rp = xp.permute((0, 3, 2, 1)), rp.permute((0, 3, 2, 1))
    if args.norm_rotation:
        rp = F.normalize(rp, dim=-1)
    return xp, rp


def _model(ref, c):
    m = ref.GCN_xyzr(input_feature=c.T, hidden_feature=c.H, output_feature=c.out, p_dropout=0, num_stage=c.num_stage, node_n=c.K,
                     no_mapping=c.no_mapping).double()
    state = R.seeded_state(c)
    assert list(m.state_dict().keys()) == list(state.keys())
    m.load_state_dict(R.to_torch(state, torch.float64), strict=True)
    return m, state


def record(ref, name):
    c = R.cfg_of(name)
    full = name == R.FULL
    out = {}
    put = lambda k, v: out.__setitem__(f"{name}/{k}", R.summarise(v.detach().numpy() if torch.is_tensor(v) else v, full))
    args = SimpleNamespace(norm_rotation=True)
    m, state = _model(ref, c)
    out[f"{name}/checksum"] = np.frombuffer(bytes.fromhex(R.checksum(state)), dtype=np.uint8)
    b = R.to_torch(R.seeded_batch(c), torch.float64)
    b["xyz_inputs"].requires_grad_(True), b["rotation_inputs"].requires_grad_(True)
    m.train()
    xp, rp = _operate(args, b, m)
    loss = torch.mean(torch.norm(xp - b["xyz_gt"], 2, -1)) + torch.mean(torch.norm(rp - b["rotation_gt"], 2, -1))
    loss.backward()
    put("xyz_pred", xp), put("r_pred", rp), put("loss", loss)
    put("grad_xyz_inputs", b["xyz_inputs"].grad), put("grad_rotation_inputs", b["rotation_inputs"].grad)
    for k, p in m.named_parameters():
        put("grad." + k, p.grad)
    for k, v in m.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            put("stat." + k, v)
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1
    # three Adam steps from the seeded state
    m, _ = _model(ref, c)
    m.train()
    b = R.to_torch(R.seeded_batch(c), torch.float64)
    opt = torch.optim.Adam(m.parameters(), lr=0.01, eps=1e-15)
    losses = []
    for _ in range(3):
        xp, rp = _operate(args, b, m)
        loss = torch.mean(torch.norm(xp - b["xyz_gt"], 2, -1)) + torch.mean(torch.norm(rp - b["rotation_gt"], 2, -1))
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    out[f"{name}/adam_losses"] = np.array(losses)
    # the eval-mode rollout, train_GCN.py:133-143
    for nr in (False, True):
        m, _ = _model(ref, c)
        m.eval()
        a = SimpleNamespace(norm_rotation=nr)
        batch = {k: v[:1].clone() for k, v in R.to_torch(R.seeded_batch(c), torch.float64).items()}
        kx, kr = [], []
        with torch.no_grad():
            for _ in range(R.ROLLOUT_FRAMES):
                xp, rp = _operate(a, batch, m)
                kx += [xp[0][-c.out:, ...]]
                kr += [rp[0][-c.out:, ...]]
                batch["xyz_inputs"] = torch.cat([batch["xyz_inputs"][:, c.out:], xp[:, -c.out:, ...]], dim=1)
                batch["rotation_inputs"] = torch.cat([batch["rotation_inputs"][:, c.out:], rp[:, -c.out:, ...]], dim=1)
        put(f"rollout{int(nr)}_xyz", torch.cat(kx, dim=0)), put(f"rollout{int(nr)}_rot", torch.cat(kr, dim=0))
    return out


def surface(ref, ref_dir):
    keys = {}
    for nm in (False, True):
        m = ref.GCN_xyzr(10, 16, 1, 0, num_stage=2, node_n=5, no_mapping=nm)
        keys[str(nm)] = list(m.state_dict().keys())
    sigs = {n: str(inspect.signature(getattr(ref, n).__init__)) for n in ("GraphConvolution", "GC_Block", "GCN", "Channel_GCN", "GCN_xyzr")}
    sigs["get_dct_matrix"] = str(inspect.signature(ref.get_dct_matrix))
    used = {}
    tree = ast.parse(open(os.path.join(ref_dir, "train_GCN.py")).read())
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.module and node.module.startswith("motion_model"):
            used[node.module] = [a.name for a in node.names]
    dataset_sig = None
    tree = ast.parse(open(os.path.join(ref_dir, "motion_model", "dataset.py")).read())
    for node in ast.walk(tree):
        if isinstance(node, ast.ClassDef) and node.name == "GCNBaseDataset":
            init = [f for f in node.body if isinstance(f, ast.FunctionDef) and f.name == "__init__"][0]
            dataset_sig = [a.arg for a in init.args.args]
    return {"state_dict_keys": keys, "signatures": sigs, "train_GCN_imports": used, "GCN3DDataset_init_args": dataset_sig,
            "item_keys": ["xyz_inputs", "xyz_gt", "rotation_inputs", "rotation_gt", "time"]}


if __name__ == "__main__":
    ref_dir = sys.argv[1]
    ref = _load(ref_dir)
    torch.manual_seed(0)
    data = {}
    for name in R.CONFIGS:
        data.update(record(ref, name))
    np.savez_compressed(os.path.join(HERE, "gcn.npz"), **data)
    json.dump(surface(ref, ref_dir), open(os.path.join(HERE, "gcn_surface.json"), "w"), indent=1)
    print("recorded", len(data), "arrays,", os.path.getsize(os.path.join(HERE, "gcn.npz")), "bytes")
