"""A plain-torch restatement (float64 or float32, CPU) of the GCN keypoint motion predictor: the layers, BatchNorm in both modes, the
loss, operate() and the autoregressive rollout [REF motion_model/gcn.py:108-275, train_GCN.py:19-43, 101, 126-143], with a deterministic
numpy recipe for every weight (`seeded_state`) and batch (`seeded_batch`).  tests/golden/make_gcn_vectors.py loads the same state into
the reference's own classes and records what they compute (tests/golden/gcn.npz); tests/test_gcn_host.py holds this restatement to those
records, tests/test_gpu_gcn.py holds the HIP kernels to this restatement."""
import hashlib
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

# (K, T, H, num_stage, out, B, no_mapping): the smallest shapes at which the tiling can go wrong
CONFIGS = OrderedDict([
    ("c0", (5, 10, 16, 1, 1, 2, False)),       # M = 15 and 20: below one tile
    ("c1", (37, 7, 48, 2, 3, 3, False)),       # M = 111 and 148: ragged against 16 and 32; odd Fin; Fout = 3; H no multiple of 32
    ("c2", (90, 10, 32, 1, 1, 4, True)),       # M = 270 and 360: more than one 256-wide k-chunk; the graph-convolution head
])
FULL = "c0"                                    # recorded in full; the others as sums plus a strided sample
ROLLOUT_FRAMES = 12
EPS, MOMENTUM = 1e-5, 0.1


def cfg_of(name):
    K, T, H, S, O, B, nm = CONFIGS[name]
    return SimpleNamespace(name=name, K=K, T=T, H=H, num_stage=S, out=O, B=B, no_mapping=nm)


def _net_keys(prefix, c, channels):
    """(key, shape, kind) in the reference's state_dict order."""
    M = channels * c.K

    def gconv(p, fin, fout):
        return [(p + ".weight", (fin, fout), ("u", fout)), (p + ".att", (M, M), ("u", fout)), (p + ".bias", (fout,), ("u", fout))]

    def bn(p, n):
        return [(p + ".weight", (n,), "gamma"), (p + ".bias", (n,), "beta"), (p + ".running_mean", (n,), "rm"),
                (p + ".running_var", (n,), "rv"), (p + ".num_batches_tracked", (), "nbt")]

    keys = gconv(prefix + ".gc1", c.T, c.H) + bn(prefix + ".bn1", M * c.H)
    for i in range(c.num_stage):
        b = f"{prefix}.gcbs.{i}"
        keys += gconv(b + ".gc1", c.H, c.H) + bn(b + ".bn1", M * c.H) + gconv(b + ".gc2", c.H, c.H) + bn(b + ".bn2", M * c.H)
    if c.no_mapping:
        keys += gconv(prefix + ".gc_out", c.H, c.out)
    else:
        keys += [(prefix + ".gc_out.0.weight", (c.H, c.H), ("u", c.H)), (prefix + ".gc_out.0.bias", (c.H,), ("u", c.H)),
                 (prefix + ".gc_out.2.weight", (c.out, c.H), ("u", c.H)), (prefix + ".gc_out.2.bias", (c.out,), ("u", c.H))]
    return keys


def state_keys(c):
    return _net_keys("GCN_xyz.GCN", c, 3) + _net_keys("GCN_r.GCN", c, 4)


def seeded_state(c):
    """Every parameter and buffer as float64 numpy (int64 for num_batches_tracked), keyed and ordered like state_dict().  Weights
    U(-s, s), s = 1 / sqrt(fan) as reset_parameters; NON-TRIVIAL BatchNorm state so that a missing or mis-indexed BatchNorm cannot
    hide: gamma in [0.5, 1.5], beta in [-0.3, 0.3], running_mean in [-0.5, 0.5], running_var in [0.5, 2]."""
    rng = np.random.default_rng(20240 + 7 * c.K + 11 * c.T + 13 * c.H + 17 * c.num_stage + 19 * c.out + 23 * int(c.no_mapping))
    ranges = {"gamma": (0.5, 1.5), "beta": (-0.3, 0.3), "rm": (-0.5, 0.5), "rv": (0.5, 2.0)}
    out = OrderedDict()
    for key, shape, kind in state_keys(c):
        if kind == "nbt":
            out[key] = np.array(0, dtype=np.int64)
        elif isinstance(kind, tuple):
            s = 1.0 / np.sqrt(kind[1])
            out[key] = rng.uniform(-s, s, size=shape)
        else:
            out[key] = rng.uniform(*ranges[kind], size=shape)
    return out


def seeded_batch(c):
    """The recorded batch: smooth keypoint trajectories plus noise, unit quaternions.  float64 numpy, the __getitem__ keys batched."""
    rng = np.random.default_rng(977 + c.K + 31 * c.T)
    n = c.T + c.out
    t = np.arange(n)[None, :, None, None] * 0.1 + rng.uniform(0, 1, size=(c.B, 1, 1, 1))
    base = rng.uniform(-1, 1, size=(1, 1, c.K, 3))
    xyz = base + 0.3 * np.sin(t + rng.uniform(0, 6, size=(1, 1, c.K, 3))) + 0.01 * rng.normal(size=(c.B, n, c.K, 3))
    q = rng.normal(size=(1, 1, c.K, 4)) + 0.3 * np.cos(t + rng.uniform(0, 6, size=(1, 1, c.K, 4))) + 0.01 * rng.normal(size=(c.B, n, c.K, 4))
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    return {"xyz_inputs": xyz[:, :c.T], "xyz_gt": xyz[:, c.T:], "rotation_inputs": q[:, :c.T], "rotation_gt": q[:, c.T:]}


def checksum(state):
    h = hashlib.sha256()
    for k, v in state.items():
        h.update(k.encode()), h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def to_torch(d, dtype, device="cpu"):
    return OrderedDict((k, torch.tensor(v, dtype=torch.int64 if np.asarray(v).dtype == np.int64 else dtype, device=device))
                       for k, v in d.items())


def is_param(key):
    return not (key.endswith("running_mean") or key.endswith("running_var") or key.endswith("num_batches_tracked"))


def excluded_bias(key, c):
    """The bias of a graph convolution that train-mode BatchNorm follows: its true gradient is exactly zero (the batch mean removes
    every per-feature shift), so what any implementation returns is rounding noise.  1 + 2 num_stage of them per network."""
    return key.endswith(".bias") and (key.endswith("GCN.gc1.bias") or ".gcbs." in key and (key.endswith(".gc1.bias") or key.endswith(".gc2.bias")))


# ---- the layers -------------------------------------------------------------------------------------------------------------------------
def act(v, kind):
    return torch.tanh(v) if kind == "tanh" else torch.relu(v) if kind == "relu" else v


def batchnorm(z, gamma, beta, rm, rv, training, stats=None, key=None):
    """BatchNorm1d(M * F) on z.view(b, -1); train mode writes the updated running statistics into `stats` under key + '.running_*'."""
    b = z.shape[0]
    v = z.reshape(b, -1)
    if training:
        mean, var = v.mean(0), v.var(0, unbiased=False)
        if stats is not None:
            stats[key + ".running_mean"] = (1 - MOMENTUM) * rm + MOMENTUM * mean.detach()
            stats[key + ".running_var"] = (1 - MOMENTUM) * rv + MOMENTUM * var.detach() * b / (b - 1)
    else:
        mean, var = rm, rv
    return ((v - mean) / torch.sqrt(var + EPS) * gamma + beta).reshape(z.shape)


def layer(x, W, att=None, bias=None, bn=None, training=False, kind="none", residual=None, stats=None, key=None):
    """act(BN(att @ (x @ W) + bias)) [+ residual]"""
    z = x @ W
    if att is not None:
        z = att @ z
    if bias is not None:
        z = z + bias
    if bn is not None:
        z = batchnorm(z, *bn, training, stats, key)
    z = act(z, kind)
    return z if residual is None else z + residual


def _bn_of(s, p):
    return s[p + ".weight"], s[p + ".bias"], s[p + ".running_mean"], s[p + ".running_var"]


def gcn(s, p, c, x, training, stats=None):
    def gl(gc, bn, x, residual=None):
        return layer(x, s[gc + ".weight"], s[gc + ".att"], s[gc + ".bias"], _bn_of(s, bn), training, "tanh", residual, stats, bn)
    y = gl(p + ".gc1", p + ".bn1", x)
    for i in range(c.num_stage):
        b = f"{p}.gcbs.{i}"
        y = gl(b + ".gc2", b + ".bn2", gl(b + ".gc1", b + ".bn1", y), residual=y)
    if c.no_mapping:
        return layer(y, s[p + ".gc_out.weight"], s[p + ".gc_out.att"], s[p + ".gc_out.bias"])
    y = torch.relu(y @ s[p + ".gc_out.0.weight"].t() + s[p + ".gc_out.0.bias"])
    return y @ s[p + ".gc_out.2.weight"].t() + s[p + ".gc_out.2.bias"]


def model(s, c, x, r, training, stats=None):
    """GCN_xyzr.forward: x (B, 3, K, T), r (B, 4, K, T) -> (B, 3, K, out), (B, 4, K, out) normalised over dim 1."""
    B = x.shape[0]
    xo = gcn(s, "GCN_xyz.GCN", c, x.reshape(B, -1, c.T), training, stats).reshape(B, 3, c.K, c.out)
    ro = gcn(s, "GCN_r.GCN", c, r.reshape(B, -1, c.T), training, stats).reshape(B, 4, c.K, c.out)
    return xo, F.normalize(ro, dim=1)


def operate(s, c, xyz_inputs, r_inputs, training, norm_rotation, stats=None):
    xp, rp = model(s, c, xyz_inputs.permute(0, 3, 2, 1), r_inputs.permute(0, 3, 2, 1), training, stats)
    xp, rp = xp.permute(0, 3, 2, 1), rp.permute(0, 3, 2, 1)
    return xp, (F.normalize(rp, dim=-1) if norm_rotation else rp)


def loss_of(xp, xg, rp, rg):
    return torch.mean(torch.norm(xp - xg, 2, -1)) + torch.mean(torch.norm(rp - rg, 2, -1))


def rollout(s, c, xyz, rot, frames, norm_rotation):
    """xyz [T, K, 3], rot [T, K, 4] -> ([frames * out, K, 3], [frames * out, K, 4])  [REF train_GCN.py:133-143]"""
    xyz, rot = xyz[None], rot[None]
    ox, orr = [], []
    with torch.no_grad():
        for _ in range(frames):
            xp, rp = operate(s, c, xyz, rot, False, norm_rotation)
            ox.append(xp[0][-c.out:]), orr.append(rp[0][-c.out:])
            xyz = torch.cat([xyz[:, c.out:], xp[:, -c.out:]], dim=1)
            rot = torch.cat([rot[:, c.out:], rp[:, -c.out:]], dim=1)
    return torch.cat(ox, 0), torch.cat(orr, 0)


# ---- what is recorded and compared ------------------------------------------------------------------------------------------------------
def train_pass(c, dtype, norm_rotation=True):
    """One train-mode forward + backward of the seeded state on the seeded batch: outputs, loss, every parameter gradient, the input
    gradients and the updated running statistics, as float64 numpy."""
    s = to_torch(seeded_state(c), dtype)
    b = to_torch(seeded_batch(c), dtype)
    params = [k for k in s if is_param(k)]
    for k in params:
        s[k].requires_grad_(True)
    b["xyz_inputs"].requires_grad_(True), b["rotation_inputs"].requires_grad_(True)
    stats = {}
    xp, rp = operate(s, c, b["xyz_inputs"], b["rotation_inputs"], True, norm_rotation, stats)
    loss = loss_of(xp, b["xyz_gt"], rp, b["rotation_gt"])
    loss.backward()
    out = {"xyz_pred": xp, "r_pred": rp, "loss": loss, "grad_xyz_inputs": b["xyz_inputs"].grad, "grad_rotation_inputs": b["rotation_inputs"].grad}
    out.update({"grad." + k: s[k].grad for k in params})
    out.update({"stat." + k: v for k, v in stats.items()})
    return {k: v.detach().double().numpy() for k, v in out.items()}


def adam_losses(c, dtype, steps=3, norm_rotation=True):
    """The losses of `steps` iterations of Adam(lr 0.01, eps 1e-15) on the seeded batch, without input noise."""
    s = to_torch(seeded_state(c), dtype)
    b = to_torch(seeded_batch(c), dtype)
    params = [s[k].requires_grad_(True) for k in s if is_param(k)]
    opt = torch.optim.Adam(params, lr=0.01, eps=1e-15)
    losses = []
    for _ in range(steps):
        stats = {}
        xp, rp = operate(s, c, b["xyz_inputs"], b["rotation_inputs"], True, norm_rotation, stats)
        loss = loss_of(xp, b["xyz_gt"], rp, b["rotation_gt"])
        opt.zero_grad()
        loss.backward()
        opt.step()
        with torch.no_grad():
            for k, v in stats.items():
                s[k].copy_(v)
        losses.append(float(loss.detach()))
    return np.array(losses, dtype=np.float64)


def rollout_pass(c, dtype, norm_rotation):
    s = to_torch(seeded_state(c), dtype)
    b = to_torch(seeded_batch(c), dtype)
    x, r = rollout(s, c, b["xyz_inputs"][0], b["rotation_inputs"][0], ROLLOUT_FRAMES, norm_rotation)
    return x.double().numpy(), r.double().numpy()


def summarise(a, full):
    """What the fixture keeps of a tensor: all of it, or its sum, its absolute sum and a strided sample."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    if full or a.size <= 64:
        return a
    return np.concatenate([[a.sum(), np.abs(a).sum()], a[::max(1, a.size // 61)]])


def bar(f32, f64):
    """The test bar of a tensor: max(8 x the float32 restatement's own distance from the float64 one, 8 * 2^-23 * max|float64|)."""
    f32, f64 = np.asarray(f32, dtype=np.float64), np.asarray(f64, dtype=np.float64)
    return max(8.0 * float(np.abs(f32 - f64).max()), 8.0 * 2.0 ** -23 * float(np.abs(f64).max()))
