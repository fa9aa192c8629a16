"""Deterministic Lloyd k-means on the device (include/gp_kmeans.h, csrc/kmeans_kernels.hip): the assignment, the per-cluster mean
with double sums in a fixed order, and the whole loop with its convergence word on the device.

  [REF utils/visualizer_utils.py:85]    kmeans()        (kmeans_pytorch.kmeans)
  [REF utils/visualizer_utils.py:86]    cluster_mean()  (torch_scatter.scatter, reduce="mean")

No kernel uses a float atomic: two calls on equal inputs give equal bits.  Nothing here reads the device, except KMeansResult's
`iterations` / `converged`, one read of the status block when one of them is asked for.  HIP only: CPU tensors raise."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

GP_KMEANS_ABI_VERSION = 1           # include/gp_kmeans.h
BLOCK = 256
MAX_D, MAX_K, MAX_ROWS, MAX_ITERS = 64, 4096, (1 << 31) - 1, 1000
STATUS_WORDS = 4
ST_ITERATIONS, ST_CONVERGED, ST_SHIFT2 = 0, 1, 2


def _prototypes():
    i32, i64, f64, P = C.c_int32, C.c_int64, C.c_double, _lib.Ptr
    return {   # name: (restype, argtypes), as include/gp_kmeans.h declares them (tests/test_kmeans_host.py compares the two)
        "gp_kmeans_abi_version": (i32, []),
        "gp_kmeans_scratch_bytes": (i64, [i64, i32, i32]),
        "gp_kmeans_assign": (i32, [i64, i32, P, i32, P, P, P, P]),
        "gp_cluster_mean": (i32, [i64, i32, P, P, i32, P, P, P, P]),
        "gp_kmeans_run": (i32, [i64, i32, P, i32, P, i32, f64, P, P, P, i32, P, P, P, P]),
    }


PROTOTYPES = _prototypes()
ABI = _lib.Abi("gp_kmeans.h", "gp_kmeans_abi_version", GP_KMEANS_ABI_VERSION, PROTOTYPES)
lib = ABI.lib            # the handle of _lib.lib() with this table applied (once)


def _device_rows(t, name, dtypes=(torch.float32,), cols=None):
    """A contiguous 2-D device tensor [rows][1 .. MAX_D] of one of `dtypes`."""
    if not torch.is_tensor(t):
        raise TypeError(f"kmeans_ops: {name} must be a tensor (got {type(t).__name__})")
    if not t.is_cuda:
        raise RuntimeError(f"kmeans_ops: {name} is on {t.device} -- HIP kernels only (no CPU fallback)")
    if t.dtype not in dtypes or not t.is_contiguous():
        raise RuntimeError(f"kmeans_ops: {name} must be a contiguous {' or '.join(str(d) for d in dtypes)} tensor "
                           f"(got {t.dtype}, contiguous={t.is_contiguous()})")
    if cols is not None and (t.dim() != 2 or t.shape[1] != cols):
        raise RuntimeError(f"kmeans_ops: {name} must be [rows, {cols}] (got {tuple(t.shape)})")
    return t


def _matrix(X, name):
    _device_rows(X, name)
    if X.dim() != 2 or not 1 <= X.shape[0] <= MAX_ROWS or not 1 <= X.shape[1] <= MAX_D:
        raise RuntimeError(f"kmeans_ops: {name} must be [1 .. 2^31 - 1, 1 .. {MAX_D}] (got {tuple(X.shape)})")
    return X


def _check_k(K):
    if not 1 <= int(K) <= MAX_K:
        raise ValueError(f"kmeans_ops: K = {K} outside [1, {MAX_K}]")
    return int(K)


def _scratch(n, d, k, dev):
    return _lib.scratch(lib().gp_kmeans_scratch_bytes, n, d, k, device=dev)


def assign(X, centres, return_d2=False):
    """ids [N] int64: the nearest centre of every row (squared Euclidean distance summed in fp32 in dimension order; ties to the lower
    index).  return_d2: also that distance, [N] fp32.  K > N is fine here."""
    _matrix(X, "X")
    _device_rows(centres, "centres", cols=X.shape[1])
    K = _check_k(centres.shape[0])
    n, d, dev = X.shape[0], X.shape[1], X.device
    ids = torch.empty(n, dtype=torch.int32, device=dev)
    d2 = torch.empty(n, dtype=torch.float32, device=dev) if return_d2 else None
    with _lib.on_device(dev):
        _lib.check(lib().gp_kmeans_assign(n, d, X, K, centres, ids, d2, _lib.stream_ptr(dev)), "gp_kmeans_assign")
    return (ids.long(), d2) if return_d2 else ids.long()


def _ids32(ids, n, K):
    _device_rows(ids, "ids", dtypes=(torch.int64, torch.int32))
    if ids.dim() != 1 or ids.shape[0] != n:
        raise RuntimeError(f"kmeans_ops: ids must be [{n}] (got {tuple(ids.shape)})")
    if ids.dtype == torch.int32:
        return ids
    return torch.where((ids >= 0) & (ids < K), ids, torch.full_like(ids, -1)).to(torch.int32)     # (an id outside [0, K) stays outside)


def cluster_mean(X, ids, K):
    """(mean [K, D] fp32, counts [K] int64): the per-cluster mean of the rows of X by ids, sums in double in a fixed order, rounded
    once; zeros for a cluster without rows; an id outside [0, K) is ignored."""
    _matrix(X, "X")
    K = _check_k(K)
    n, d, dev = X.shape[0], X.shape[1], X.device
    i32 = _ids32(ids, n, K)
    mean = torch.empty(K, d, dtype=torch.float32, device=dev)
    counts = torch.empty(K, dtype=torch.int32, device=dev)
    scratch = _scratch(n, d, K, dev)
    with _lib.on_device(dev):
        _lib.check(lib().gp_cluster_mean(n, d, X, i32, K, mean, counts, scratch, _lib.stream_ptr(dev)), "gp_cluster_mean")
    return mean, counts.long()


class KMeansResult:
    """ids [N] int64, centres [K, D], counts [K] int64, aux_mean [K, A] or None: all describe the centres returned.  `iterations`,
    `converged` and `shift2` read the status block (once) when first asked for."""

    def __init__(self, ids, centres, counts, aux_mean, status):
        self.ids, self.centres, self.counts, self.aux_mean, self.status = ids, centres, counts, aux_mean, status
        self._host = None

    def _read(self):
        if self._host is None:
            words = self.status.cpu()
            self._host = (int(words[ST_ITERATIONS]), bool(words[ST_CONVERGED]), float(words[ST_SHIFT2:ST_SHIFT2 + 2].clone().view(torch.float64)[0]))
        return self._host

    @property
    def iterations(self):
        return self._read()[0]

    @property
    def converged(self):
        return self._read()[1]

    @property
    def shift2(self):
        return self._read()[2]

    def __iter__(self):
        return iter((self.ids, self.centres, self.counts, self.aux_mean, self.iterations, self.converged))


def kmeans(X, K, iters=20, tol=0.0, seed=0, init=None, aux=None) -> KMeansResult:
    """Up to `iters` Lloyd iterations (stop once shift^2 <= tol; tol = 0: an exact fixed point only), then one assignment against
    the final centres.  Initial centres: `init` [K, D], or X[randperm(N, seeded)[:K]] -- the rows training.kmeans starts from.
    aux [N, A] (A <= D): its per-cluster mean by the final ids comes back as aux_mean.  Nothing is read from the device."""
    K = _check_k(K)
    if torch.is_tensor(X) and X.dim() == 2 and K > X.shape[0]:
        raise ValueError(f"kmeans_ops.kmeans: K = {K} > N = {X.shape[0]} rows")
    _matrix(X, "X")
    n, d, dev = X.shape[0], X.shape[1], X.device
    if not 1 <= int(iters) <= MAX_ITERS:
        raise ValueError(f"kmeans_ops.kmeans: iters = {iters} outside [1, {MAX_ITERS}]")
    if not float(tol) >= 0:
        raise ValueError(f"kmeans_ops.kmeans: tol = {tol} must be >= 0")
    if init is not None:
        _device_rows(init, "init", cols=d)
        if init.shape[0] != K:
            raise RuntimeError(f"kmeans_ops: init must be [{K}, {d}] (got {tuple(init.shape)})")
    if aux is not None:
        _device_rows(aux, "aux")
        if aux.dim() != 2 or aux.shape[0] != n or not 1 <= aux.shape[1] <= d:
            raise RuntimeError(f"kmeans_ops: aux must be [{n}, 1 .. {d}] (got {tuple(aux.shape)})")
    if init is not None:
        centres = init.clone()
    else:
        g = torch.Generator().manual_seed(int(seed))
        centres = X[torch.randperm(n, generator=g)[:K].to(dev)].clone()
    ids = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(K, dtype=torch.int32, device=dev)
    aux_mean = torch.empty(K, aux.shape[1], dtype=torch.float32, device=dev) if aux is not None else None
    status = torch.empty(STATUS_WORDS, dtype=torch.int32, device=dev)
    scratch = _scratch(n, d, K, dev)
    with _lib.on_device(dev):
        _lib.check(lib().gp_kmeans_run(n, d, X, K, centres, int(iters), float(tol), ids, counts, aux, aux.shape[1] if aux is not None else 0,
                                       aux_mean, status, scratch, _lib.stream_ptr(dev)), "gp_kmeans_run")
    return KMeansResult(ids.long(), centres, counts.long(), aux_mean, status)
