"""The GCN motion predictor's kernels (include/gp_gcn.h, csrc/gcn_kernels.hip): one graph-convolution layer
`Y = act(BN(att @ (X @ W) + bias)) [+ residual]` as a torch.autograd.Function over gp_gcn_layer_forward / gp_gcn_layer_backward, and the
eval-mode autoregressive rollout of both networks (gp_gcn_rollout).

  [REF motion_model/gcn.py:132-138, 164-177, 220-235]   GraphConvolution / BatchNorm1d / Tanh / residual / the head
  [REF train_GCN.py:19-43, 126-143, 165-176]            operate() and the prediction loops

No kernel uses a float atomic: two calls on equal inputs give equal bits.  Nothing here reads the device.  HIP only: CPU tensors raise."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

GP_GCN_ABI_VERSION = 1           # include/gp_gcn.h
MAX_M, MAX_F, MAX_B, MAX_FRAMES, MAX_STAGES = 4096, 512, 1024, 4096, 16
ACT_NONE, ACT_TANH, ACT_RELU = 0, 1, 2
BN_OFF, BN_EVAL, BN_TRAIN = 0, 1, 2
TABLE_SLOTS = 7
BN_TRAIN_B1 = "Expected more than 1 value per channel when training"


def _prototypes():
    i32, i64, P = C.c_int32, C.c_int64, _lib.Ptr
    return {   # name: (restype, argtypes), as include/gp_gcn.h declares them (tests/test_gcn_host.py compares the two)
        "gp_gcn_abi_version": (i32, []),
        "gp_gcn_layer_forward": (i32, [i32, i32, i32, i32, P, P, i32, P, P, i32, P, P, P, P, i32, P, P, P, P, P, P, P]),
        "gp_gcn_layer_backward": (i32, [i32, i32, i32, i32, P, P, i32, P, i32, P, P, i32, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P]),
        "gp_gcn_scratch_bytes": (i64, [i32, i32, i32, i32, i32, i32]),
        "gp_gcn_rollout": (i32, [i32, i32, i32, i32, i32, i32, P, i32, P, P, i32, i32, P, P, P, P, P, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi("gp_gcn.h", "gp_gcn_abi_version", GP_GCN_ABI_VERSION, PROTOTYPES)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)


def _dev(t, name, shape=None):
    """A contiguous fp32 device tensor (of `shape`)."""
    if not torch.is_tensor(t):
        raise TypeError(f"gcn_ops: {name} must be a tensor (got {type(t).__name__})")
    if not t.is_cuda:
        raise RuntimeError(f"gcn_ops: {name} is on {t.device} -- HIP kernels only (no CPU fallback)")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"gcn_ops: {name} must be a contiguous torch.float32 tensor (got {t.dtype}, contiguous={t.is_contiguous()})")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"gcn_ops: {name} must be {tuple(shape)} (got {tuple(t.shape)})")
    return t


def _check_shape(B, M, Fin, Fout):
    for v, name, hi in ((B, "B", MAX_B), (M, "M", MAX_M), (Fin, "Fin", MAX_F), (Fout, "Fout", MAX_F)):
        if not 1 <= v <= hi:
            raise ValueError(f"gcn_ops: {name} = {v} outside [1, {hi}]")


class GcnLayerFn(torch.autograd.Function):
    """One layer.  x [B, M, Fin]; weight [Fin, Fout] (w_transposed: [Fout, Fin], nn.Linear's); att [M, M] or None; bias [Fout] or
    None; bn: None or (gamma, beta, running_mean, running_var) with `training` selecting batch or running statistics (train mode
    updates the running statistics in place); residual: None or a tensor of the output's shape."""

    @staticmethod
    def forward(ctx, x, weight, att, bias, gamma, beta, running_mean, running_var, residual, w_transposed, act, bn_mode, grad_mode):
        B, M, Fin = x.shape
        Fout = weight.shape[0] if w_transposed else weight.shape[1]
        dev = x.device
        need_grad = grad_mode and any(ctx.needs_input_grad)     # (grad_mode: torch.is_grad_enabled() at the call; it is off in here)
        if need_grad and bn_mode == BN_EVAL:
            raise RuntimeError("gcn_ops: a gradient was requested in eval mode -- the eval-mode BatchNorm has no backward here "
                               "(the reference only evaluates under no_grad); call .train() or wrap the call in torch.no_grad()")
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        Y = new(B, M, Fout)
        S = new(B, M, Fout) if att is not None else None
        Z = new(B, M, Fout) if (need_grad or bn_mode == BN_TRAIN) else None
        mean, inv = (new(M * Fout), new(M * Fout)) if bn_mode == BN_TRAIN else (None, None)
        with _lib.on_device(dev):
            _lib.check(lib().gp_gcn_layer_forward(B, M, Fin, Fout, x, weight, int(w_transposed), att, bias, bn_mode, gamma, beta, running_mean,
                                                  running_var, act, residual, S, Z, mean, inv, Y, _lib.stream_ptr(dev)), "gp_gcn_layer_forward")
        if need_grad:
            ctx.save_for_backward(x, weight, att, gamma, beta, S, Z, mean, inv)
            ctx.cfg = (int(w_transposed), act, bn_mode, bias is not None, residual is not None)
        return Y

    @staticmethod
    def backward(ctx, dY):
        x, weight, att, gamma, beta, S, Z, mean, inv = ctx.saved_tensors
        wt, act, bn_mode, has_bias, has_res = ctx.cfg
        B, M, Fin = x.shape
        Fout = Z.shape[2]
        dev = x.device
        dY = dY.contiguous()
        need = ctx.needs_input_grad
        new = lambda ref: torch.empty_like(ref)
        dZ = new(Z)
        dS = new(Z) if att is not None else None
        dX = new(x) if need[0] else None
        dW = new(weight) if need[1] else None
        datt = new(att) if (att is not None and need[2]) else None
        dbias = torch.empty(Fout, dtype=torch.float32, device=dev) if (has_bias and need[3]) else None
        dgamma = new(gamma) if (bn_mode == BN_TRAIN and need[4]) else None
        dbeta = new(beta) if (bn_mode == BN_TRAIN and need[5]) else None
        with _lib.on_device(dev):
            _lib.check(lib().gp_gcn_layer_backward(B, M, Fin, Fout, x, weight, wt, att, bn_mode, gamma, beta, act, S, Z, mean, inv, dY, dZ, dS,
                                                   dX, dW, datt, dbias, dgamma, dbeta, None, _lib.stream_ptr(dev)), "gp_gcn_layer_backward")
        dres = dY if (has_res and need[8]) else None         # (dresidual = dY: the tensor itself, no copy)
        return dX, dW, datt, dbias, dgamma, dbeta, None, None, dres, None, None, None, None


def layer(x, weight, att=None, bias=None, bn=None, training=False, act=ACT_NONE, residual=None, w_transposed=False):
    """Y = act(BN(att @ (x @ W) + bias)) [+ residual]; see GcnLayerFn."""
    _dev(x, "x")
    if x.dim() != 3:
        raise RuntimeError(f"gcn_ops: x must be [B, M, Fin] (got {tuple(x.shape)})")
    B, M, Fin = x.shape
    _dev(weight, "weight")
    if weight.dim() != 2 or weight.shape[1 if w_transposed else 0] != Fin:
        raise RuntimeError(f"gcn_ops: weight {tuple(weight.shape)} does not take Fin = {Fin} (w_transposed={bool(w_transposed)})")
    Fout = weight.shape[0 if w_transposed else 1]
    _check_shape(B, M, Fin, Fout)
    if act not in (ACT_NONE, ACT_TANH, ACT_RELU):
        raise ValueError(f"gcn_ops: act = {act} is none of ACT_NONE / ACT_TANH / ACT_RELU")
    if att is not None:
        _dev(att, "att", (M, M))
    if bias is not None:
        _dev(bias, "bias", (Fout,))
    if residual is not None:
        _dev(residual, "residual", (B, M, Fout))
    gamma = beta = rm = rv = None
    bn_mode = BN_OFF
    if bn is not None:
        gamma, beta, rm, rv = bn
        for t, name in ((gamma, "bn weight"), (beta, "bn bias"), (rm, "running_mean"), (rv, "running_var")):
            _dev(t, name, (M * Fout,))
        bn_mode = BN_TRAIN if training else BN_EVAL
        if training and B < 2:
            raise ValueError(f"{BN_TRAIN_B1}, got input size {(B, M * Fout)}")
    return GcnLayerFn.apply(x, weight, att, bias, gamma, beta, rm, rv, residual, bool(w_transposed), act, bn_mode, torch.is_grad_enabled())


def rollout_table(layers):
    """The host pointer table of gp_gcn_rollout from [[(W, att, bias, gamma, beta, running_mean, running_var), ..] per network]; the
    tensors must outlive the call."""
    flat = []
    for net in layers:
        for entry in net:
            assert len(entry) == TABLE_SLOTS
            for t in entry:
                if t is not None:
                    _dev(t, "a rollout table entry")
                flat.append(0 if t is None else t.data_ptr())
    return (C.c_void_p * len(flat))(*flat)


def rollout(table, K, T, H, num_stage, output_size, no_mapping, xyz, rot, frames, norm_rotation, base_xyz=None):
    """(xyz_out [frames * output_size, K, 3], rot_out [.., K, 4], delta_out [.., K, 7] or None): gp_gcn_rollout."""
    _dev(xyz, "xyz_inputs", (T, K, 3))
    _dev(rot, "rotation_inputs", (T, K, 4))
    if base_xyz is not None:
        _dev(base_xyz, "base_xyz", (K, 3))
    frames, output_size = int(frames), int(output_size)
    for v, name, lo, hi in ((K, "K", 1, MAX_M // 4), (T, "T", 1, MAX_F), (H, "H", 1, MAX_F), (num_stage, "num_stage", 0, MAX_STAGES),
                            (output_size, "output_size", 1, min(MAX_F, T)), (frames, "frames", 1, MAX_FRAMES)):
        if not lo <= v <= hi:
            raise ValueError(f"gcn_ops.rollout: {name} = {v} outside [{lo}, {hi}]")
    dev = xyz.device
    rows = frames * output_size
    xyz_out = torch.empty(rows, K, 3, dtype=torch.float32, device=dev)
    rot_out = torch.empty(rows, K, 4, dtype=torch.float32, device=dev)
    delta_out = torch.empty(rows, K, 7, dtype=torch.float32, device=dev) if base_xyz is not None else None
    scratch = _lib.scratch(lib().gp_gcn_scratch_bytes, K, T, H, num_stage, output_size, frames, device=dev)
    with _lib.on_device(dev):
        _lib.check(lib().gp_gcn_rollout(K, T, H, num_stage, output_size, int(bool(no_mapping)), table, len(table), xyz, rot, frames,
                                        int(bool(norm_rotation)), base_xyz, xyz_out, rot_out, delta_out, scratch, _lib.stream_ptr(dev)),
                   "gp_gcn_rollout")
    return xyz_out, rot_out, delta_out
