"""LPIPS v0.1 with the AlexNet and VGG16 backbones on the device (include/gp_lpips.h, csrc/lpips_kernels.hip): hand-written HIP
convolutions on the exact-float32 matrix instruction, max-pools, the per-layer normalised distance and a double-precision finalize;
no vendor convolution library and no torchvision.

  [REF lpipsPyTorch/__init__.py:6-21]          lpips(x, y, net_type)
  [REF lpipsPyTorch/modules/networks.py, lpips.py, utils.py]   the z-score, the tapped layers, the distance

The CALLER supplies the weight files -- the torchvision backbone (`alexnet-owt-7be5be79.pth`, `vgg16-397923af.pth`) and the published
`lin` layers (`alex.pth`, `vgg.pth`) -- as the reference's run-time downloads leave them in the torch hub cache; this package ships
none and never fetches any.  HIP only: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace

import torch

from . import _lib

GP_LPIPS_ABI_VERSION = 1            # include/gp_lpips.h
NETS = {"alex": 0, "vgg": 1, "squeeze": 2}
QUANTIZE8 = 1
TAPS, COLUMNS = 5, 8
NAMES = ("LPIPS", "layer1", "layer2", "layer3", "layer4", "layer5", "reserved", "reserved")
CONV, RELU, POOL = 0, 1, 2
BACKBONE_FILES = {"alex": "alexnet-owt-7be5be79.pth", "vgg": "vgg16-397923af.pth"}
LIN_FILES = {"alex": "alex.pth", "vgg": "vgg.pth"}


def _prototypes():
    i32, i64, u32, P = C.c_int32, C.c_int64, C.c_uint32, _lib.Ptr
    return {   # name: (restype, argtypes), as include/gp_lpips.h declares them (tests/test_lpips_host.py compares the two)
        "gp_lpips_abi_version": (i32, []),
        "gp_lpips_num_layers": (i32, [i32]),
        "gp_lpips_layer": (i32, [i32, i32, P]),
        "gp_lpips_weight_floats": (i64, [i32]),
        "gp_lpips_pack_weights": (i32, [i32, P, P, P, P, P]),
        "gp_lpips_scratch_bytes": (i64, [i32, i32, i32, i32]),
        "gp_lpips": (i32, [i32, P, P, P, i32, i32, i32, u32, P, P, P, P]),
        "gp_lpips_conv2d_relu": (i32, [P, P, P, P, P, i32, i32, i32, i32, i32, i32, i32, i32, P]),
        "gp_lpips_maxpool": (i32, [P, P, i32, i32, i32, i32, i32, i32, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi("gp_lpips.h", "gp_lpips_abi_version", GP_LPIPS_ABI_VERSION, PROTOTYPES)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)


def _net_id(net_type):
    if net_type == "squeeze":
        raise NotImplementedError("LPIPS: net_type 'squeeze' is not provided (nothing in the reference's evaluation asks for it); "
                                  "choose 'alex' or 'vgg'")
    if net_type not in ("alex", "vgg"):
        raise NotImplementedError(f"LPIPS: choose net_type from [alex, vgg] (got {net_type!r})")
    return NETS[net_type]


def network_table(net_type):
    """The library's table of torchvision's `features` entries: a list of namespaces (kind, cin, cout, k, stride, pad, tap, conv)."""
    net, l = _net_id(net_type), lib()
    n = int(l.gp_lpips_num_layers(net))
    if n < 0:
        raise _lib.GpHipError(f"gp_lpips_num_layers: {_lib.last_error()}")
    out = []
    for i in range(n):
        d = (C.c_int32 * 8)()
        _lib.check(l.gp_lpips_layer(net, i, d), "gp_lpips_layer")
        out.append(SimpleNamespace(kind=d[0], cin=d[1], cout=d[2], k=d[3], stride=d[4], pad=d[5], tap=bool(d[6]), conv=d[7]))
    return out


def target_layers(net_type):
    """The 1-based positions of the tapped entries, as the reference's `target_layers` counts them [REF networks.py:57-59]."""
    return [i + 1 for i, e in enumerate(network_table(net_type)) if e.tap]


def n_channels_list(net_type):
    return [e.cout for e in network_table(net_type) if e.tap]


def _load(obj, what):
    if isinstance(obj, (str, os.PathLike)):
        try:
            obj = torch.load(obj, map_location="cpu", weights_only=True)
        except TypeError:       # (a torch without the argument)
            obj = torch.load(obj, map_location="cpu")
    if hasattr(obj, "state_dict") and not isinstance(obj, dict):
        obj = obj.state_dict()
    if not isinstance(obj, dict):
        raise TypeError(f"LPIPS: {what} must be a state dict or a path to a .pth file (got {type(obj).__name__})")
    return obj


def _pick(sd, forms, what):
    for key in forms:
        if key in sd:
            return key, sd[key]
    raise KeyError(f"LPIPS: {what} has none of the keys {list(forms)}")


def _checked(key, t, shape):
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
        got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"LPIPS: {key} must have shape {tuple(shape)} (got {got})")
    return t.detach().to(torch.float32).contiguous()


def load_weights(net_type, backbone, lin):
    """(conv weights, conv biases, lin weights) of `net_type` from state dicts or .pth paths, in network order, float32, every
    shape checked against the library's table (the message names the key).  Needs no GPU.
      backbone keys   `features.{i}.weight|bias` (a whole torchvision model: other keys are ignored), `{i}.weight|bias`, or
                      `layers.{i}.weight|bias`, i = the convolution's position in torchvision's `features`
      lin keys        the published `lin{k}.model.1.weight` or the reference's renamed `{k}.1.weight` [REF utils.py:22-29], [1,C,1,1]"""
    table = network_table(net_type)
    bb, ln = _load(backbone, "backbone"), _load(lin, "lin")
    ws, bs, ls = [], [], []
    for i, e in enumerate(table):
        if e.kind != CONV:
            continue
        for part, shape, dst in (("weight", (e.cout, e.cin, e.k, e.k), ws), ("bias", (e.cout,), bs)):
            key, t = _pick(bb, (f"features.{i}.{part}", f"{i}.{part}", f"layers.{i}.{part}"), "backbone")
            dst.append(_checked(key, t, shape))
    for k, c in enumerate(e.cout for e in table if e.tap):
        key, t = _pick(ln, (f"lin{k}.model.1.weight", f"{k}.1.weight"), "lin")
        ls.append(_checked(key, t, (1, c, 1, 1)))
    return ws, bs, ls


class LPIPS:
    """LPIPS(net_type, backbone, lin, device="cuda"): `backbone` and `lin` are state dicts or paths to .pth files in the key forms
    of load_weights(); the weights are packed on the device once."""

    def __init__(self, net_type, backbone, lin, device="cuda"):
        self.net_type, self.net = net_type, _net_id(net_type)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("LPIPS: device must be a GPU -- HIP kernels only (no CPU fallback)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        ws, bs, ls = ([t.to(dev) for t in ts] for ts in load_weights(net_type, backbone, lin))
        l = lib()
        n = int(l.gp_lpips_weight_floats(self.net))
        self.packed = torch.zeros(n, dtype=torch.float32, device=dev)
        arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])      # noqa: E731
        with _lib.on_device(dev):
            _lib.check(l.gp_lpips_pack_weights(self.net, arr(ws), arr(bs), arr(ls), self.packed, _lib.stream_ptr(dev)), "gp_lpips_pack_weights")
            torch.cuda.current_stream(dev).synchronize()     # (once, at load time: the sources may be freed now)
        self._scratch = {}

    def scratch(self, H, W):
        key = (_lib.stream_ptr(self.device).value, H, W)
        t = self._scratch.get(key)
        if t is None:
            if len(self._scratch) >= 2:
                self._scratch.pop(next(iter(self._scratch)))
            t = _lib.scratch(lib().gp_lpips_scratch_bytes, self.net, 1, H, W, device=self.device, extra=256)
            self._scratch[key] = t
        return t

    def __call__(self, x, y, *, quantize8=False, out=None, invalid_flag=None):
        """x (the render), y (the ground truth): [B,3,H,W] or [3,H,W] in [0, 1].  Returns a namespace: `table` [B,8] float64 on the
        device (column 0 = LPIPS, 1..5 = the layer terms, 6..7 = 0), `names`; nothing is read back.  quantize8: x goes through 8
        bits first, as image_metrics does it.  out=: a contiguous [B,8] float64 view that receives the table.  invalid_flag:
        optional 32-bit word per pair on the device; non-zero makes that row NaN."""
        a, b = _as_batch(x, "x"), _as_batch(y, "y")
        if a.shape != b.shape or a.device != b.device:
            raise RuntimeError(f"LPIPS: x {tuple(a.shape)} on {a.device} and y {tuple(b.shape)} on {b.device} differ")
        dev = a.device
        if dev != self.device:
            raise RuntimeError(f"LPIPS: the weights are on {self.device}, the images on {dev}")
        B, _, H, W = a.shape
        if out is None:
            table = torch.empty(B, COLUMNS, dtype=torch.float64, device=dev)
        else:
            table = out
            if table.dtype != torch.float64 or table.device != dev or tuple(table.shape) != (B, COLUMNS) or not table.is_contiguous():
                raise RuntimeError(f"LPIPS: out must be a contiguous [{B},{COLUMNS}] float64 tensor on {dev}")
        if invalid_flag is not None:
            if invalid_flag.device != dev or invalid_flag.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) \
                    or invalid_flag.numel() != B or not invalid_flag.is_contiguous():
                raise RuntimeError(f"LPIPS: invalid_flag must be {B} contiguous 32-bit words on {dev}")
        with _lib.on_device(dev):
            scratch = self.scratch(H, W)
            sp = (scratch.data_ptr() + 255) & ~255
            rc = lib().gp_lpips(self.net, self.packed, a, b, B, H, W, QUANTIZE8 if quantize8 else 0, sp, invalid_flag, table,
                                _lib.stream_ptr(dev))
            _lib.check(rc, "gp_lpips")
        return SimpleNamespace(table=table, names=NAMES)


def _as_batch(x, name):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError(f"LPIPS: {name} must be a GPU tensor -- HIP kernels only (no CPU fallback)")
    x = x.detach()
    if x.dim() == 3:
        x = x[None]
    if x.dim() != 4 or x.shape[1] != 3:
        raise RuntimeError(f"LPIPS: {name} must be [B,3,H,W] or [3,H,W] (got {tuple(x.shape)})")
    return x.to(torch.float32).contiguous()


def find_lpips_weights(net_type, search=None):
    """(backbone path, lin path) of `net_type`: the file names the reference's downloads leave behind, looked for in `search` (a
    directory or a list of them), then $GP_LPIPS_WEIGHTS, then torch.hub.get_dir()/checkpoints.  Never downloads; raises
    FileNotFoundError listing every path tried."""
    _net_id(net_type)
    dirs = [] if search is None else ([search] if isinstance(search, (str, os.PathLike)) else list(search))
    if os.environ.get("GP_LPIPS_WEIGHTS"):
        dirs += os.environ["GP_LPIPS_WEIGHTS"].split(os.pathsep)
    dirs.append(os.path.join(torch.hub.get_dir(), "checkpoints"))
    found, tried = [], []
    for name in (BACKBONE_FILES[net_type], LIN_FILES[net_type]):
        for d in dirs:
            p = os.path.join(os.fspath(d), name)
            tried.append(p)
            if os.path.isfile(p):
                found.append(p)
                break
    if len(found) != 2:
        raise FileNotFoundError(f"LPIPS ({net_type}): the weight files {BACKBONE_FILES[net_type]} and {LIN_FILES[net_type]} are needed "
                                "(this package ships none and never downloads); tried: " + ", ".join(tried))
    return found[0], found[1]


_cache: dict = {}


def cached(net_type, device, weights=None):
    """One LPIPS per (net, device, weights): `weights` is None (find_lpips_weights), a directory, a (backbone, lin) pair of
    paths or state dicts, or a dict {"backbone": ..., "lin": ...}."""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if isinstance(weights, os.PathLike):
        weights = os.fspath(weights)
    if isinstance(weights, dict) and set(weights) >= {"backbone", "lin"}:
        weights = (weights["backbone"], weights["lin"])
    key = (net_type, str(dev), weights if isinstance(weights, (str, type(None))) else tuple(w if isinstance(w, str) else id(w) for w in weights))
    m = _cache.get(key)
    if m is None:
        pair = find_lpips_weights(net_type, weights) if weights is None or isinstance(weights, str) else weights
        m = _cache[key] = LPIPS(net_type, pair[0], pair[1], device=dev)
    return m


def lpips(x, y, net_type="alex", weights=None):
    """The reference's call shape [REF lpipsPyTorch/__init__.py:6-21]: LPIPS of x against y, a float64 device tensor ([B], or a
    scalar tensor for [3,H,W] inputs).  The network is built once per (net, device, weights), not per call."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError("LPIPS: x must be a GPU tensor -- HIP kernels only (no CPU fallback)")
    t = cached(net_type, x.device, weights)(x, y).table[:, 0]
    return t[0] if x.dim() == 3 else t

