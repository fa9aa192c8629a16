"""The PCA colouring of gaussianprediction_amd/csrc/gp_pca.h restated in float64 numpy, independently of csrc/pca_core.h: np.linalg.eigh
for the eigenvectors, np.percentile and np.partition for the order statistics.  Everything is float64 (the device's float32 roundings
are what the GPU tests' tolerances are for), except `project32`, the float32 projection in the definition's own order."""
import numpy as np


def sign_rule(components):
    """Each row times +-1 so that its entry of largest magnitude is positive, the first such entry on a tie."""
    c = np.array(components, dtype=np.float64)
    first = np.argmax(np.abs(c), axis=1)                    # (argmax returns the first maximum)
    s = np.where(c[np.arange(len(c)), first] < 0, -1.0, 1.0)
    return c * s[:, None]


def fit(X, dim):
    """(mean [D], components [dim, D], explained_variance [dim], all eigenvalues descending [D]) in float64."""
    X = np.asarray(X, dtype=np.float64)
    mean = X.mean(axis=0)
    d = X - mean
    C = d.T @ d / (len(X) - 1)
    lam, vec = np.linalg.eigh(C)                             # ascending
    order = np.argsort(-lam, kind="stable")
    return mean, sign_rule(vec[:, order[:dim]].T), lam[order[:dim]], lam[order]


def project(X, mean, components):
    return (np.asarray(X, dtype=np.float64) - np.asarray(mean, dtype=np.float64)) @ np.asarray(components, dtype=np.float64).T


def project32(X, mean, components):
    """y_ik = sum_j (x_ij - mean_j) * c_kj in float32, j ascending from y = 0, one rounding per operation."""
    X, mean, components = (np.asarray(a, dtype=np.float32) for a in (X, mean, components))
    y = np.zeros((len(X), len(components)), np.float32)
    for j in range(X.shape[1]):
        y = y + (X[:, j] - mean[j])[:, None] * components[None, :, j]
    return y


def percentiles(values, qs):
    return np.percentile(np.asarray(values, dtype=np.float64).reshape(-1), qs)


def order_statistics(values, qs):
    """[len(qs), 2]: the floor and ceil order statistics of each percentile, in the values' own dtype, by np.partition."""
    v = np.asarray(values).reshape(-1)
    out = []
    for q in qs:
        pos = q / 100 * (len(v) - 1)
        lo, hi = int(np.floor(pos)), int(np.ceil(pos))
        part = np.partition(v, sorted({lo, hi}))
        out.append([part[lo], part[hi]])
    return np.array(out, dtype=v.dtype)


def interpolate(v_lo, v_hi, q, M):
    """(float32)(v_lo + (v_hi - v_lo) * (pos - lo)) in float64."""
    pos = q / 100 * (M - 1)
    return np.float32(np.float64(v_lo) + (np.float64(v_hi) - np.float64(v_lo)) * (pos - np.floor(pos)))


def colors_of(Y, q1, q99):
    """(positions or None, colours) of transformed values Y [N, dim], dim 3 or 5."""
    vis = (np.asarray(Y, dtype=np.float64) - q1) / (q99 - q1)
    if vis.shape[1] == 3:
        return None, np.clip(vis, 0.0, 1.0)
    pos = np.concatenate([vis[:, :2], np.ones((len(vis), 1))], axis=-1)
    return pos, np.clip(vis[:, 2:5], 0.0, 1.0)


def pca_vis(X, dim):
    """The whole recipe on samples X (for dim 5: [xyz, features] already concatenated): a dict of mean, components,
    explained_variance, q1, q99, positions (None for dim 3) and colors."""
    mean, comp, var, _ = fit(X, dim)
    Y = project(X, mean, comp)
    q1, q99 = percentiles(Y, [1, 99])
    pos, col = colors_of(Y, q1, q99)
    return dict(mean=mean, components=comp, explained_variance=var, q1=q1, q99=q99, positions=pos, colors=col, Y=Y)


def generate(N, D, seed):
    """The GPU grid's input: normal(N, D) @ A^T + 3 * offset, the columns of A scaled by linspace(2, 0.1, D)."""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(D, D)) * np.linspace(2.0, 0.1, D)[None, :]
    return (rng.normal(size=(N, D)) @ A.T + 3.0 * rng.normal(size=D)).astype(np.float32)


def lut_index(x):
    """Row of the 256-entry table for each x, -1 for a NaN."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        idx = np.where(x < 0, 0, np.where(x >= 1, 255, (np.nan_to_num(x) * np.float32(256)).astype(np.int64)))
    idx = np.clip(idx, 0, 255)
    return np.where(np.isnan(x), -1, idx)
