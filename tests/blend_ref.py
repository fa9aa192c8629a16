"""float64 reference of the keypoint blend (csrc/deform_kernels.hip, "keypoint blend + pose composition") in GATHER form, with the
magnitude sums the per-element bounds of tests/test_gpu_blend_direct.py are built from, the neighbour-index pattern builders of
that file and its input specs (shared with tests/test_blend_ref_host.py, which checks all three on the CPU).

Semantics (the reference model's blend): softmax over each half of raw_w; optionally F.normalize of every keypoint quaternion
(eps 1e-12); weighted sums over the nn gathered keypoint rows; xyz_t = xyz + dxyz, q_t = normalize(quat_mul(normalize(dq), rot)).
Stage 1 (nn == 0): delta is per Gaussian.  Never an N x K matrix: delta[idx] is N x nn x 7.  Gradients by autograd of
L = <xyz_t, gx> + <q_t, gq>.

Every index row handed out has DISTINCT entries in [0, K), as a kNN gives them (check_indices): the reference model's dense scatter
overwrites on duplicates, so they have no defined answer, and an index outside [0, K) must never reach a kernel.

The bound.  |got - want| <= RTOL * A + ATOL per element, A the sum of the MAGNITUDES of the terms that make the element (with the
factors that amplify an upstream rounding error, below), so a keypoint whose gradient cancels to nearly nothing is held to the size
of what was added, not to the size of what is left, and one wrong row among thousands is not averaged away.
  w~   = w * (1 + max(raw) - raw): a softmax weight with the relative error of its exponent's argument
  cond = sum_j wr_j |v_j| / |dq|  (>= 1): cancellation in the blended quaternion, which every later step divides by
  xyz_t  : |xyz| + sum_j wx~_j |dxyz_j|                q_t : cond
  M(gp)  : (|gq_c| + |y_c| sum |y| |gq|) / |pq|   (normalize_bwd written with magnitudes), m = |M(gp)|_2
  g_rot  : m * cond            (each component is a signed permutation of q against gp: Cauchy-Schwarz, |q| = 1)
  M(gdq) : m |rot| (1 + |y_c| sum |y|) / |dq| * cond
  g_delta[k, 0:3] : sum wx~ |gx|;  g_delta[k, 3:7] : sum wr~ M(gdq), then normalize_bwd in magnitudes when norm_rotation
  g_raw_w: w~_j (M(gw_j) + sum_j w~_j M(gw_j)),  M(gwx_j) = sum_c |dxyz_jc| |gx_c|,  M(gwr_j) = sum_c |v_jc| M(gdq)_c
RTOL is not chosen: test_blend_ref_host.py restates the blend in float32 torch, takes the worst err / A over every input spec and
holds RTOL to four times that (the kernel's summation order differs from the restatement's).
ATOL covers float32 underflow only (a weight exp(-120) is 0 in float32 and 8e-53 in float64)."""
import numpy as np
import torch

F = torch.nn.functional

CHUNK = 256          # Gaussians per chunk of the backward (one counting sort each)
BB_LONG = 20         # a keypoint's list within a chunk beyond this length is summed by a wave
MAX_BLOCKS = 1024    # workgroups of the backward: beyond CHUNK * MAX_BLOCKS Gaussians a workgroup takes a second chunk
THRESH_LENGTHS = (1, 2, 19, 20, 21, 63, 64, 65)     # list lengths of the 'threshold' chunk (they add up to 255 of its 256 rows)

# float32 restatement (torch, CPU) against float64 over every input spec of test_gpu_blend_direct.py at CPU scale, worst err / A:
# xyz_t 1.74e-7, q_t 1.27e-7, g_delta 2.13e-7, g_raw_w 1.69e-7, g_rot 1.66e-7 (test_blend_ref_host.py measures it on every run and
# holds RTOL between four and eight times the worst).  The kernels on the MI355X, all 97 cases of test_gpu_blend_direct.py: 2.74e-7 (g_rot).
RTOL = 4 * 2.14e-7
ATOL = 1e-30


def quat_mul(q1, q2):
    """Hamilton product q1 (x) q2, (w, x, y, z)."""
    w1, x1, y1, z1 = q1.unbind(-1)
    w2, x2, y2, z2 = q2.unbind(-1)
    return torch.stack([w2 * w1 - x2 * x1 - y2 * y1 - z2 * z1, x2 * w1 + w2 * x1 + z2 * y1 - y2 * z1,
                        y2 * w1 - z2 * x1 + w2 * y1 + x2 * z1, z2 * w1 + y2 * x1 - x2 * y1 + w2 * z1], dim=-1)


def _normalize_bwd_mag(y, g_mag, n):
    """magnitudes of normalize_bwd: dv = (g - y (y . g)) / n, every product taken by absolute value."""
    ya = y.abs()
    return (g_mag + ya * (ya * g_mag).sum(-1, keepdim=True)) / n.unsqueeze(-1)


def blend_reference(inp, dtype=torch.float64, magnitudes=True):
    """inp: dict(delta [K or N, od], raw_w [N, 2 nn] | None, idx [N, nn] int64 | None, xyz, rot, gx, gq, nn, norm).  Returns numpy
    arrays xyz_t, q_t, g_delta, g_raw_w (nn > 0), g_xyz, g_rot, and A_<name> for each but g_xyz (which is gx, bit for bit)."""
    nn, norm = int(inp["nn"]), bool(inp["norm"])
    leaf = lambda t: t.detach().to(dtype, copy=True).requires_grad_(True)          # (a copy: the inputs stay as they are)
    d, x, r = leaf(inp["delta"]), leaf(inp["xyz"]), leaf(inp["rot"])
    gx, gq = inp["gx"].to(dtype), inp["gq"].to(dtype)
    idx = inp["idx"]
    dxyz_k, v_raw = d[:, 0:3], d[:, 3:7]
    v_k = F.normalize(v_raw, dim=-1, eps=1e-12) if norm else v_raw
    leaves = [d, x, r]
    if nn:
        check_indices(idx.numpy(), d.shape[0])
        w = leaf(inp["raw_w"])
        leaves.append(w)
        wx, wr = torch.softmax(w[:, :nn], dim=-1), torch.softmax(w[:, nn:], dim=-1)
        dxyz = (wx.unsqueeze(-1) * dxyz_k[idx]).sum(1)
        dq = (wr.unsqueeze(-1) * v_k[idx]).sum(1)
    else:
        dxyz, dq = dxyz_k, v_k
    xt = x + dxyz
    qn = F.normalize(dq, dim=-1, eps=1e-12)
    pq = quat_mul(qn, r)
    qt = F.normalize(pq, dim=-1, eps=1e-12)
    grads = torch.autograd.grad((xt * gx).sum() + (qt * gq).sum(), leaves)
    np_ = lambda t: t.detach().numpy()
    out = {"xyz_t": np_(xt), "q_t": np_(qt), "g_delta": np_(grads[0]), "g_xyz": np_(grads[1]), "g_rot": np_(grads[2])}
    if nn:
        out["g_raw_w"] = np_(grads[3])
    if not magnitudes:
        return out
    with torch.no_grad():
        N = x.shape[0]
        n_dq = dq.norm(dim=-1).clamp_min(1e-12)
        if nn:
            raw = w.detach()
            wxm = wx * (1 + raw[:, :nn].max(-1, keepdim=True).values - raw[:, :nn])
            wrm = wr * (1 + raw[:, nn:].max(-1, keepdim=True).values - raw[:, nn:])
            dg, vg = dxyz_k[idx].abs(), v_k[idx]
            cond = ((wr * vg.norm(dim=-1)).sum(1) / n_dq).clamp_min(1.0)
            out["A_xyz_t"] = np_(x.abs() + (wxm.unsqueeze(-1) * dg).sum(1))
        else:
            cond = torch.ones(N, dtype=dtype)
            out["A_xyz_t"] = np_(x.abs() + dxyz_k.abs())
        out["A_q_t"] = np_(cond.unsqueeze(-1).expand(N, 4))
        m = _normalize_bwd_mag(qt, gq.abs(), pq.norm(dim=-1).clamp_min(1e-12)).norm(dim=-1)
        out["A_g_rot"] = np_((m * cond).unsqueeze(-1).expand(N, 4))
        M_gdq = _normalize_bwd_mag(qn, (m * r.norm(dim=-1)).unsqueeze(-1).expand(N, 4), n_dq) * cond.unsqueeze(-1)
        if nn:
            K = d.shape[0]
            terms = torch.cat([wxm.unsqueeze(-1) * gx.abs().unsqueeze(1), wrm.unsqueeze(-1) * M_gdq.unsqueeze(1)], dim=-1)
            A_acc = torch.zeros(K, 7, dtype=dtype).index_add_(0, idx.reshape(-1), terms.reshape(-1, 7))
            del terms
            if norm:
                A_acc[:, 3:7] = _normalize_bwd_mag(v_k, A_acc[:, 3:7], v_raw.norm(dim=-1).clamp_min(1e-12))
            M_gwx = (dg * gx.abs().unsqueeze(1)).sum(-1)
            M_gwr = (vg.abs() * M_gdq.unsqueeze(1)).sum(-1)
            out["A_g_raw_w"] = np_(torch.cat([wxm * (M_gwx + (wxm * M_gwx).sum(1, keepdim=True)),
                                              wrm * (M_gwr + (wrm * M_gwr).sum(1, keepdim=True))], dim=-1))
        else:
            A_acc = torch.cat([gx.abs(), _normalize_bwd_mag(v_k, M_gdq, v_raw.norm(dim=-1).clamp_min(1e-12)) if norm else M_gdq], dim=-1)
        A_delta = torch.zeros(d.shape[0], d.shape[1], dtype=dtype)
        A_delta[:, :7] = A_acc
        out["A_g_delta"] = np_(A_delta)
    return out


COMPARED = ("xyz_t", "q_t", "g_delta", "g_raw_w", "g_rot")


def worst_ratio(got, want, A, atol=ATOL):
    """max over elements of max(|got - want| - atol, 0) / A; an error above atol where A is 0 counts as inf."""
    err = np.maximum(np.abs(np.asarray(got, np.float64) - want) - atol, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err > 0, err / A, 0.0)
    return float(np.nanmax(q)) if q.size else 0.0


def within_bound(got, want, A, rtol=RTOL, atol=ATOL):
    return bool(np.all(np.abs(np.asarray(got, np.float64) - want) <= rtol * A + atol))


# ------------------------------------------------------------------------------------------------
# neighbour-index patterns
# ------------------------------------------------------------------------------------------------
def check_indices(idx, K):
    """every row distinct, every entry in [0, K): asserted by every builder and again before a launch."""
    idx = np.asarray(idx)
    assert idx.dtype == np.int64 and idx.ndim == 2
    if idx.size == 0:
        return idx
    assert idx.min() >= 0 and idx.max() < K, "neighbour index outside [0, K)"
    s = np.sort(idx, axis=1)
    assert not (s[:, 1:] == s[:, :-1]).any(), "duplicate neighbour in a row"
    return idx


def _distinct(rng, n, pool, m):
    """n rows of m distinct integers of [0, pool), uniformly."""
    assert 0 < m <= pool
    if pool < 4 * m:
        return np.argsort(rng.random((n, pool)), axis=1)[:, :m].astype(np.int64)
    out = rng.integers(0, pool, size=(n, m), dtype=np.int64)
    while True:
        s = np.sort(out, axis=1)
        bad = np.nonzero((s[:, 1:] == s[:, :-1]).any(axis=1))[0]
        if bad.size == 0:
            return out
        out[bad] = rng.integers(0, pool, size=(bad.size, m), dtype=np.int64)


def _rotate_columns(block):
    """row r rotated by r columns: whatever a builder puts into one column lands in every neighbour slot."""
    n, m = block.shape
    return np.take_along_axis(block, (np.arange(m)[None, :] + np.arange(n)[:, None]) % m, axis=1)


def uniform_rows(rng, N, K, nn):
    return check_indices(_distinct(rng, N, K, nn), K)


def coherent_block(rng, rows, K, nn):
    """all rows share one neighbour set: every one of its nn lists is `rows` long."""
    return _rotate_columns(np.tile(_distinct(rng, 1, K, nn), (rows, 1)))


def even_block(rng, rows, K, nn):
    """lists as even as they get: ceil(rows nn / K) at most."""
    assert K >= nn
    start = int(rng.integers(0, K))
    return (start + np.arange(rows)[:, None] * nn + np.arange(nn)[None, :]) % K


def coherent_rows(rng, N, K, nn):
    idx = np.empty((N, nn), dtype=np.int64)
    for lo in range(0, N, CHUNK):
        idx[lo:lo + CHUNK] = coherent_block(rng, min(CHUNK, N - lo), K, nn)
    return check_indices(idx, K)


def hot_rows(rng, N, K, nn, hot):
    """keypoint `hot` in every row (in every slot in turn), the other nn - 1 random."""
    assert 0 <= hot < K and K >= nn
    idx = np.empty((N, nn), dtype=np.int64)
    idx[:, 0] = hot
    if nn > 1:
        rest = _distinct(rng, N, K - 1, nn - 1)
        idx[:, 1:] = rest + (rest >= hot)
    return check_indices(_rotate_columns(idx), K)


def threshold_rows(rng, N, K, nn, chunk=0, lengths=THRESH_LENGTHS):
    """uniform rows, but chunk `chunk` holds one list of each length of `lengths` and a keypoint with none.  Returns
    (idx, targets, empty): targets[j] has exactly lengths[j] entries in that chunk, `empty` has none."""
    lo = chunk * CHUNK
    assert lo + CHUNK <= N and sum(lengths) <= CHUNK and K >= len(lengths) + 1 + nn
    idx = _distinct(rng, N, K, nn)
    special = rng.permutation(K)[:len(lengths) + 1].astype(np.int64)
    targets, empty = special[:-1], int(special[-1])
    filler = np.setdiff1d(np.arange(K, dtype=np.int64), special)
    block = filler[_distinct(rng, CHUNK, filler.size, nn)]
    col0 = np.repeat(targets, lengths)
    block[rng.permutation(CHUNK)[:col0.size], 0] = col0
    idx[lo:lo + CHUNK] = _rotate_columns(block)
    return check_indices(idx, K), targets, empty


def coherent_then_uniform_rows(rng, N, K, nn, period=MAX_BLOCKS):
    """uniform rows; chunk 0 and chunk period + 1 coherent.  With period = MAX_BLOCKS workgroup 0 takes chunks 0 and MAX_BLOCKS
    (nlong = nn, then 0) and workgroup 1 chunks 1 and MAX_BLOCKS + 1 (0, then nn).  The chunks that promise nlong = 0 are uniform
    when the draw has no list beyond BB_LONG there and spread evenly (even_block) when it has.  (period = 1: the same three kinds of
    chunk in 768 rows, for the CPU.)"""
    assert N >= (period + 2) * CHUNK and CHUNK * nn <= BB_LONG * K
    idx = _distinct(rng, N, K, nn)
    for c in (0, period + 1):
        idx[c * CHUNK:(c + 1) * CHUNK] = coherent_block(rng, CHUNK, K, nn)
    for c in {1, period}:
        blk = idx[c * CHUNK:(c + 1) * CHUNK]
        if np.bincount(blk.reshape(-1), minlength=K).max() > BB_LONG:
            idx[c * CHUNK:(c + 1) * CHUNK] = even_block(rng, CHUNK, K, nn)
    return check_indices(idx, K)


def list_lengths(idx, K):
    """[chunks, K]: entries of keypoint k in chunk c -- what the backward's counting sort counts."""
    N, nn = idx.shape
    chunks = (N + CHUNK - 1) // CHUNK
    flat = (np.arange(N)[:, None] // CHUNK) * K + idx
    return np.bincount(flat.reshape(-1), minlength=chunks * K).reshape(chunks, K)


# ------------------------------------------------------------------------------------------------
# the backward's LDS budget (gp_blend_backward_impl) and the grid
# ------------------------------------------------------------------------------------------------
def bwd_lds_bytes(K, nn, od):
    """acc[K*7] | delta[K*od] | cnt[K] | base[K+1] | g[7*256] | inv[K] | w[256*2*nn] | sorted u16 [256*nn], as the dispatch adds it up."""
    return (K * (7 + od + 3) + 1 + 256 * 7 + 256 * 2 * nn) * 4 + 256 * nn * 2 + 16 if nn > 0 else 256 * 8 * 4


def max_keypoints(nn, od):
    """the largest K gp_blend_backward accepts: LDS <= 64 KiB (make_blend's K * 7 * 4 <= 60000 is the looser one for every nn)."""
    K = 1
    while bwd_lds_bytes(K + 1, nn, od) <= 64 * 1024 and (K + 1) * 7 * 4 <= 60000:
        K += 1
    return K


def bwd_blocks(N, nn):
    b = (N + CHUNK - 1) // CHUNK
    return min(b, MAX_BLOCKS) if nn > 0 else b


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
class Spec(tuple):
    """(pattern, N, K, nn, od, norm, values): hashable, one set of inputs each."""
    __slots__ = ()
    pattern, N, K, nn, od, norm, values = (property(lambda s, i=i: s[i]) for i in range(7))


def spec(pattern, N, K, nn, od=8, norm=True, values="normal"):
    return Spec((pattern, int(N), int(K), int(nn), int(od), bool(norm), values))


def cpu_scale(sp, rows=600):
    """the same spec at a size the CPU tests afford: at most `rows` Gaussians (768 for 'coh_uni', which needs three chunks)."""
    pattern, N, K, nn, od, norm, values = sp
    return spec(pattern, 3 * CHUNK if pattern == "coh_uni" else min(N, rows), K, nn, od, norm, values)


def make_inputs(sp):
    """float32 / int64 CPU tensors of one spec, seeded by the spec.  `meta` carries what the pattern promises."""
    pattern, N, K, nn, od, norm, values = sp
    seed = [N, K, nn, od, int(norm), sum(map(ord, pattern + values))]
    rng = np.random.default_rng(seed)
    f32 = lambda a: torch.tensor(np.asarray(a, dtype=np.float32))
    delta = rng.normal(size=(K if nn else N, od)).astype(np.float32) * 0.3
    meta = {}
    idx = raw_w = None
    if nn:
        raw_w = rng.normal(size=(N, 2 * nn)).astype(np.float32)
        if pattern == "uniform":
            idx = uniform_rows(rng, N, K, nn)
        elif pattern == "coherent":
            idx = coherent_rows(rng, N, K, nn)
        elif pattern == "threshold":
            meta["chunk"] = (N // CHUNK) // 2          # (a chunk in the middle; N spans at least two)
            idx, meta["targets"], meta["empty"] = threshold_rows(rng, N, K, nn, chunk=meta["chunk"])
        elif pattern == "hot":
            meta["hot"] = int(rng.integers(0, K))
            idx = hot_rows(rng, N, K, nn, meta["hot"])
        elif pattern == "perm":
            assert K == nn
            idx = uniform_rows(rng, N, K, nn)
        elif pattern == "coh_uni":
            meta["period"] = MAX_BLOCKS if N >= (MAX_BLOCKS + 2) * CHUNK else 1
            idx = coherent_then_uniform_rows(rng, N, K, nn, period=meta["period"])
        else:
            raise ValueError(pattern)
        if values == "big60" and N:          # rows of +-60: exp(raw - max) spans e^-120 .. 1; without the max subtraction exp(60) squared overflows the sum's reciprocal
            rows = np.arange(0, N, 7)
            raw_w[rows] = 60.0 * rng.choice([-1.0, 1.0], size=(rows.size, 2 * nn)).astype(np.float32)
            raw_w[rows[0]] = 60.0            # (a row of equal weights at +60, and one at -60)
            raw_w[rows[-1]] = -60.0
        if values == "zeroquat":
            assert norm
            meta["zero_kp"] = int(idx[N // 2, 0])
            delta[meta["zero_kp"], 3:7] = 0.0
    else:
        assert pattern == "stage1"
        if values == "zeroquat":
            meta["zero_kp"] = N // 2
            delta[meta["zero_kp"], 3:7] = 0.0
    return {"delta": f32(delta), "raw_w": f32(raw_w) if nn else None, "idx": torch.from_numpy(idx) if nn else None,
            "xyz": f32(rng.uniform(-1, 1, size=(N, 3))), "rot": f32(rng.normal(size=(N, 4))), "gx": f32(rng.normal(size=(N, 3))),
            "gq": f32(rng.normal(size=(N, 4))), "nn": nn, "norm": norm, "K": K, "od": od, "meta": meta}
