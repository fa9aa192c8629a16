"""Flat-kernel mean-shift clustering on the device (csrc/gp_meanshift.h, csrc/meanshift_kernels.hip): sklearn's estimate_bandwidth and
MeanShift with the labels they give, without anyone choosing k.

  [REF utils/visualizer_utils.py:35-44]    cluster(): sklearn MeanShift().fit(features).labels_ on the host

The header states the definition in full: float32 distances summed in dimension order, an exact k-th distance per row by a radix select,
the members' means from float64 sums in ascending row order, sklearn's stopping rule with its off-by-one, the greedy merge in the
reference's precedence order, labels by kmeans_ops.assign.  Two calls on equal inputs give equal bytes.  What is unpinned: the results
on non-finite input (the calls return, nothing outside the arrays is touched).

Out of scope: bin_seeding / min_bin_freq -- `seeds=` takes any rows, and a voxel_ops.voxel_down_sample or a furthest-point subsample of
X is the intended way to seed a large cloud -- and sklearn's predict (kmeans_ops.assign(rows, result.cluster_centers) is that).

HIP only: CPU tensors, another dtype than float32 and non-contiguous tensors raise."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

GP_MEANSHIFT_ABI_VERSION = 1        # csrc/gp_meanshift.h
MAX_D, MAX_CENTRES, MAX_ITER = 64, 4096, 10000
STATUS_WORDS = 8
ST_UNFINISHED, ST_KEPT, ST_EMPTY, ST_OVERFLOW, ST_N_ITER, ST_BAD_BANDWIDTH, ST_LIVE = range(7)
MERGE_ROUNDS = 64                   # rounds of pick-and-suppress between two reads of the one status word
HEADER = "../gaussianprediction_amd/csrc/gp_meanshift.h"      # relative to include/: the header is not one of include/ 


def _prototypes():
    i32, i64, f64, P = C.c_int32, C.c_int64, C.c_double, _lib.Ptr
    return {   # name: (restype, argtypes), as csrc/gp_meanshift.h declares them (tests/test_meanshift_host.py compares the two)
        "gp_meanshift_abi_version": (i32, []),
        "gp_meanshift_scratch_size": (i64, [i64, i64, i64]),
        "gp_meanshift_bandwidth": (i32, [P, i64, i64, f64, P, P, P, i64, P]),
        "gp_meanshift_run": (i32, [P, i64, i64, P, i64, P, i32, P, P, P, P, P, i64, P]),
        "gp_meanshift_merge": (i32, [P, P, i64, i64, P, i32, i32, P, P, P, P, i64, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi(HEADER, "gp_meanshift_abi_version", GP_MEANSHIFT_ABI_VERSION, PROTOTYPES, register=False)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)


# ---- the refusals that need no device, as the library words them (None: accepted) ----
def check_sizes(N, S, D):
    N, S, D = int(N), int(S), int(D)
    if D < 1 or D > MAX_D:
        return "D must be in 1 .. 64"
    if N < 1 or N >= 2 ** 31:
        return "N must be in 1 .. 2^31 - 1"
    if S < 1 or S >= 2 ** 31:
        return "S must be in 1 .. 2^31 - 1"
    if N * D >= 2 ** 31:
        return "N*D must be below 2^31"
    if S * D >= 2 ** 31:
        return "S*D must be below 2^31"
    return None


def check_quantile(quantile):
    return None if 0.0 < float(quantile) <= 1.0 else "quantile must be in (0, 1]"


def check_max_iter(max_iter):
    return None if 0 <= int(max_iter) <= MAX_ITER else "max_iter must be in 0 .. 10000"


def check_rounds(rounds):
    return None if 1 <= int(rounds) <= MAX_CENTRES else "rounds must be in 1 .. 4096"


def check_bandwidth(bandwidth):
    b = float(bandwidth)
    return None if math.isfinite(b) and b > 0.0 else "bandwidth must be finite and > 0"


def radius2(bandwidth):
    """The largest float32 t with sqrtf(t) <= (float)bandwidth (ms_radius2 of csrc/meanshift_core.h), as a Python float."""
    bw = np.float32(bandwidth)
    with np.errstate(over="ignore"):
        k = min(int(np.float32(bw * bw).view(np.uint32)), 0x7F7FFFFF)
    root = lambda k: np.sqrt(np.uint32(k).view(np.float32))
    for _ in range(8):
        if k > 0 and root(k) > bw:
            k -= 1
    for _ in range(8):
        if k < 0x7F7FFFFF and root(k + 1) <= bw:
            k += 1
    return float(np.uint32(k).view(np.float32))


def _device_rows(what, t):
    if not torch.is_tensor(t):
        raise RuntimeError(f"{what} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{what} is on {t.device} -- HIP kernels only (no CPU fallback)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what} must be float32 (got {t.dtype})")
    if t.dim() != 2:
        raise RuntimeError(f"{what} must have 2 dimension(s) (got {tuple(t.shape)})")
    if not t.is_contiguous():
        raise RuntimeError(f"{what} must be contiguous")
    return t.detach()


def _refuse(what, why, **sizes):
    if why:
        raise _lib.GpHipError(f"{what}: {why} ({', '.join(f'{k} = {v}' for k, v in sizes.items())})")


def _bandwidth_tensor(what, bandwidth, dev):
    """A 0-dim float64 tensor on `dev`: a number is checked and uploaded, a device tensor is taken as it is (the kernels test it)."""
    if torch.is_tensor(bandwidth):
        if not bandwidth.is_cuda or bandwidth.device != dev:
            raise RuntimeError(f"{what}: bandwidth is on {bandwidth.device} -- HIP kernels only (no CPU fallback)")
        if bandwidth.dtype != torch.float64 or bandwidth.numel() != 1:
            raise RuntimeError(f"{what}: a bandwidth tensor must hold one float64 (got {bandwidth.dtype}, {tuple(bandwidth.shape)})")
        return bandwidth.detach().reshape(())
    _refuse(what, check_bandwidth(bandwidth), bandwidth=float(bandwidth))
    return torch.tensor(float(bandwidth), dtype=torch.float64, device=dev)


def estimate_bandwidth(X, quantile=0.3, n_samples=None, random_state=0, return_kth=False):
    """sklearn.cluster.estimate_bandwidth on the device: the mean over the rows of X [N, D] of the distance to the k-th nearest row, self
    included, k = max(1, int(N * quantile)).  n_samples: sklearn's subsample, check_random_state(random_state).permutation(N)[:n_samples]
    made with numpy on the host, then one gather on the device.  Returns a 0-dim float64 device tensor (with return_kth also the [N]
    float32 k-th distances); nothing is read from the device."""
    x = _device_rows("estimate_bandwidth: X", X)
    if n_samples is not None:
        rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
        idx = rs.permutation(x.shape[0])[:int(n_samples)]
        x = x[torch.from_numpy(idx).to(x.device)].contiguous()
    N, D = x.shape
    _refuse("estimate_bandwidth", check_sizes(N, 1, D) or check_quantile(quantile), N=N, D=D, quantile=float(quantile))
    dev = x.device
    out = torch.empty((), dtype=torch.float64, device=dev)
    kth = torch.empty(N, dtype=torch.float32, device=dev) if return_kth else None
    with _lib.on_device(dev):
        l = lib()
        scratch = _lib.scratch(l.gp_meanshift_scratch_size, N, 1, D, device=dev)
        _lib.check(l.gp_meanshift_bandwidth(x, N, D, float(quantile), out, kth, scratch, scratch.numel(), _lib.stream_ptr(dev)),
                   "gp_meanshift_bandwidth")
    return (out, kth) if return_kth else out


@dataclass
class MeanShiftResult:
    """labels [N] int64 (-1: an orphan, with cluster_all=False), cluster_centers [K, D] float32 in precedence order, counts [K] int64 (the
    members of each centre's last step), n_iter, bandwidth (the 0-dim float64 device tensor that was used), and per seed, for tests and
    diagnostics: seed_centers [S, D], seed_counts [S] int64 (0: no point was near, the seed was dropped), seed_iterations [S] int64."""
    labels: torch.Tensor
    cluster_centers: torch.Tensor
    counts: torch.Tensor
    n_iter: int
    bandwidth: torch.Tensor
    seed_centers: torch.Tensor
    seed_counts: torch.Tensor
    seed_iterations: torch.Tensor


def mean_shift(X, bandwidth=None, seeds=None, max_iter=300, cluster_all=True) -> MeanShiftResult:
    """sklearn's MeanShift(bandwidth, seeds, max_iter=max_iter, cluster_all=cluster_all).fit(X) on the device, X [N, D] float32.
    bandwidth: None estimates it (estimate_bandwidth(X)); a number is uploaded; a 0-dim float64 device tensor -- an estimate -- is used
    without a host read.  seeds [S, D]: the starting points, X itself by default, which costs N * N pairs per step: for a large cloud
    pass a subsample (voxel_ops.voxel_down_sample, a furthest-point sample, X[::stride]); bin_seeding is not provided.  The host reads
    one status word per 64 merge rounds and the status block once at the end.  Raises GpHipError on more than 4096 centres or a
    bandwidth that is not finite and > 0, ValueError when no point was within the bandwidth of any seed."""
    x = _device_rows("mean_shift: X", X)
    sd = x if seeds is None else _device_rows("mean_shift: seeds", seeds)
    N, D = x.shape
    S = sd.shape[0]
    if sd.shape[1] != D or sd.device != x.device:
        raise RuntimeError(f"mean_shift: seeds {tuple(sd.shape)} must be [S, {D}] on {x.device}")
    _refuse("mean_shift", check_sizes(N, S, D) or check_max_iter(max_iter), N=N, S=S, D=D, max_iter=int(max_iter))
    dev = x.device
    bw = estimate_bandwidth(x) if bandwidth is None else _bandwidth_tensor("mean_shift", bandwidth, dev)
    seed_centers = torch.empty(S, D, dtype=torch.float32, device=dev)
    seed_counts = torch.empty(S, dtype=torch.int32, device=dev)
    seed_iterations = torch.empty(S, dtype=torch.int32, device=dev)
    status = torch.empty(STATUS_WORDS, dtype=torch.int32, device=dev)
    centres = torch.empty(MAX_CENTRES, D, dtype=torch.float32, device=dev)
    counts = torch.empty(MAX_CENTRES, dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        l = lib()
        st = _lib.stream_ptr(dev)
        scratch = _lib.scratch(l.gp_meanshift_scratch_size, N, S, D, device=dev)
        _lib.check(l.gp_meanshift_run(x, N, D, sd, S, bw, int(max_iter), seed_centers, seed_counts, seed_iterations, status, scratch,
                                      scratch.numel(), st), "gp_meanshift_run")
        first = 1
        for _ in range(MAX_CENTRES // MERGE_ROUNDS + 1):
            _lib.check(l.gp_meanshift_merge(seed_centers, seed_counts, S, D, bw, first, MERGE_ROUNDS, centres, counts, status, scratch,
                                            scratch.numel(), st), "gp_meanshift_merge")
            first = 0
            if not int(status[ST_LIVE]):                       # (the one word read per batch of rounds)
                break
    words = status.tolist()
    if words[ST_BAD_BANDWIDTH]:
        _refuse("mean_shift", "bandwidth must be finite and > 0", bandwidth=float(bw))
    if words[ST_OVERFLOW]:
        _refuse("mean_shift", "more than 4096 centres were kept", S=S, bandwidth=float(bw))
    K = words[ST_KEPT]
    if K == 0:
        raise ValueError("No point was within bandwidth=%f of any seed. Try a different seeding strategy or increase the bandwidth."
                         % float(bw))
    from . import kmeans_ops
    cluster_centers = centres[:K].clone()
    labels, d2 = kmeans_ops.assign(x, cluster_centers, return_d2=True)
    if not cluster_all:
        labels = torch.where(d2 > radius2(float(bw)), torch.full_like(labels, -1), labels)      # sqrtf(d2) > (float)bandwidth
    return MeanShiftResult(labels, cluster_centers, counts[:K].long(), words[ST_N_ITER], bw, seed_centers, seed_counts.long(),
                           seed_iterations.long())
