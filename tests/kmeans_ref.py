"""The float64 torch restatement of include/gp_kmeans.h that tests/test_kmeans_host.py and tests/test_gpu_kmeans.py compare against,
the seeded inputs both use, and `ambiguous_rows`: the rows whose nearest and second-nearest centres are too close for an fp32
distance to order them."""
import torch

# (N, K, D, kind): the shapes of the assignment and mean tests.  The first five are the ones the ambiguity cap was checked on.
CAPPED = [(5000, 37, 35, "uniform"), (5000, 150, 35, "model"), (4099, 512, 35, "model"), (5000, 150, 64, "uniform"), (257, 2, 3, "uniform")]
SHAPES = [(1, 1, 1, "uniform"), (63, 2, 3, "uniform"), (257, 2, 3, "uniform"), (5000, 37, 35, "uniform"), (5000, 150, 35, "model"),
          (4099, 512, 35, "model"), (5000, 150, 64, "uniform"), (2000, 1024, 64, "uniform")]      # the last: the centres go through LDS in tiles
AMBIGUOUS_REL = 1e-4      # fp32 accumulation of D <= 64 non-negative terms errs by <= ~2 D 2^-24 = 8e-6 relative: an order of magnitude of margin
AMBIGUOUS_CAP = 0.005     # at most 0.5 % of the rows may be left out of an id comparison


def make_input(n, k, d, kind, seed=0):
    """(X [n, d] fp32, centres [k, d] fp32) on the CPU: uniform rows in [-1, 1), or model-like ones (xyz in +-1.3, features +-1e-3);
    the centres are a seeded row subset (rows repeat where k > n)."""
    g = torch.Generator().manual_seed(1000 * seed + n + 7 * k + 13 * d)
    X = torch.rand(n, d, generator=g) * 2 - 1
    if kind == "model":
        X[:, :3] *= 1.3
        X[:, 3:] *= 1e-3
    rows = torch.randperm(n, generator=g)[:k] if k <= n else torch.randint(0, n, (k,), generator=g)
    return X.contiguous(), X[rows].clone().contiguous()


def dist2(X, centres, chunk=1024):
    """[N, K] float64 squared distances."""
    X, C = X.double().cpu(), centres.double().cpu()
    out = torch.empty(X.shape[0], C.shape[0], dtype=torch.float64)
    for s in range(0, X.shape[0], chunk):
        out[s:s + chunk] = ((X[s:s + chunk, None, :] - C[None, :, :]) ** 2).sum(-1)
    return out


def assign(X, centres):
    """(ids [N] int64: the float64 argmin, the lower index on a tie; d2 [N] float64)."""
    d2 = dist2(X, centres)
    best = d2.min(dim=1).values
    ids = (d2 == best[:, None]).int().argmax(dim=1)          # the FIRST minimum
    return ids, best


def ambiguous_rows(X, centres):
    """[N] bool: (d2_second - d2_best) <= 1e-4 * d2_second in float64 (never with one centre)."""
    d2 = dist2(X, centres)
    if d2.shape[1] < 2:
        return torch.zeros(d2.shape[0], dtype=torch.bool)
    two = d2.topk(2, dim=1, largest=False).values
    return (two[:, 1] - two[:, 0]) <= AMBIGUOUS_REL * two[:, 1]


def cluster_mean(X, ids, K):
    """(mean [K, D] float64, zeros for an empty cluster; counts [K] int64); ids outside [0, K) are ignored."""
    X, ids = X.double().cpu(), ids.cpu().long()
    ok = (ids >= 0) & (ids < K)
    sums = torch.zeros(K, X.shape[1], dtype=torch.float64).index_add_(0, ids[ok], X[ok])
    counts = torch.bincount(ids[ok], minlength=K)
    return torch.where(counts[:, None] > 0, sums / counts[:, None].clamp_min(1), torch.zeros_like(sums)), counts


def update(X, ids, centres):
    """One Lloyd update in float64 from given ids: (new centres -- the old one for an empty cluster --, counts, shift^2)."""
    mean, counts = cluster_mean(X, ids, centres.shape[0])
    new = torch.where(counts[:, None] > 0, mean, centres.double().cpu())
    shift = (new.float().double() - centres.double().cpu()).norm(dim=1).sum()
    return new, counts, float(shift * shift)


def kmeans(X, init, iters, tol=0.0):
    """Lloyd from `init`, as gp_kmeans_run states it, centres rounded to fp32 after every update: (ids to the centres returned,
    centres fp32, counts, iterations run, converged)."""
    centres = init.float().cpu().clone()
    ran, converged = 0, False
    for _ in range(iters):
        ids, _ = assign(X, centres)
        new, _, s2 = update(X, ids, centres)
        centres = new.float()
        ran += 1
        if s2 <= tol:
            converged = True
            break
    ids, _ = assign(X, centres)
    return ids, centres, torch.bincount(ids, minlength=centres.shape[0]), ran, converged


def inertia(X, ids, centres):
    return float(((X.double().cpu() - centres.double().cpu()[ids.cpu()]) ** 2).sum())


def blobs(n=3000, k=20, d=35, sigma=0.01, seed=3):
    """k well-separated blobs: (X fp32, labels, one jittered row per blob as the initial centres)."""
    g = torch.Generator().manual_seed(seed)
    means = torch.rand(k, d, generator=g) * 4 - 2             # pairwise distance ~ sqrt(d * 8 / 3) >> sigma * sqrt(d)
    labels = torch.arange(n) % k
    X = (means[labels] + sigma * torch.randn(n, d, generator=g)).float().contiguous()
    first = torch.stack([X[(labels == j).nonzero()[0, 0]] for j in range(k)])
    init = (first + 0.5 * sigma * torch.randn(k, d, generator=g)).float().contiguous()
    return X, labels, init
