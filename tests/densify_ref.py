"""The sequence densify -> reset_opacity -> prune of training.TrainingMixin restated as ONE function of explicit inputs, with the torch
operations the model's methods use (so that on equal inputs it equals them bit for bit: tests/test_densify_plan_host.py), torch only.
With dtype=torch.float64 every input is widened first: the result is the float64 shadow of the computed fields (split xyz, split
scaling, reset opacity), valid wherever no selection sits within rounding distance of its threshold (margins())."""
from types import SimpleNamespace

import torch

STATS = ("accum", "denom", "accum_max", "max_radii2D")


def build_rotation(r):
    q = r / torch.sqrt((r * r).sum(-1, keepdim=True))
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)


def densify_reset_prune(state, moments, stats, normals, *, grad_threshold, percent_dense, extent, min_opacity, max_screen_size,
                        do_densify, do_reset, do_prune=True, dtype=torch.float32):
    """state: name -> [N, ...] (needs xyz, scaling, rotation, opacity); moments: name -> (exp_avg, exp_avg_sq) for the optimized ones;
    stats: the four of STATS (accum, denom, accum_max [N,1]; max_radii2D [N]); normals [2,N,3]: copy c of split source i is placed
    with normals[c, i].  Returns a namespace: state, moments, stats of the result, n_clone, n_src, n_pruned, the masks `clone` and
    `split` over the input rows, and per output row `source` (input row) and `segment` (0 survivor, 1 clone, 2 / 3 split copies)."""
    P = {k: v.detach().to(dtype) for k, v in state.items()}
    M = {k: (m.detach().to(dtype), v.detach().to(dtype)) for k, (m, v) in moments.items()}
    S = {k: stats[k].detach().to(dtype) for k in STATS}
    N, dev = P["xyz"].shape[0], P["xyz"].device
    source = torch.arange(N, device=dev)
    segment = torch.zeros(N, dtype=torch.long, device=dev)
    clone = torch.zeros(N, dtype=torch.bool, device=dev)
    split = torch.zeros(N, dtype=torch.bool, device=dev)
    n_clone = n_src = n_pruned = 0

    def append(new, src, seg):
        nonlocal P, M, source, segment
        P = {k: torch.cat([P[k], new[k]]) for k in P}
        M = {k: tuple(torch.cat([t, torch.zeros_like(new[k])]) for t in mv) for k, mv in M.items()}
        source, segment = torch.cat([source, src]), torch.cat([segment, seg])

    def remove(mask):
        nonlocal P, M, S, source, segment
        keep = ~mask
        P = {k: v[keep] for k, v in P.items()}
        M = {k: (m[keep], v[keep]) for k, (m, v) in M.items()}
        S = {k: v[keep] for k, v in S.items()}
        source, segment = source[keep], segment[keep]

    def zero_stats():
        nonlocal S
        n = P["xyz"].shape[0]
        S = {k: torch.zeros((n, 1) if k != "max_radii2D" else (n,), dtype=dtype, device=dev) for k in STATS}

    if do_densify:
        grads = torch.where(S["denom"] > 0, S["accum"] / S["denom"].clamp_min(1), torch.zeros_like(S["accum"]))
        # densify_and_clone
        clone = torch.norm(grads, dim=-1) >= grad_threshold
        clone = clone & (torch.exp(P["scaling"]).max(dim=1).values <= percent_dense * extent)
        n_clone = int(clone.sum())
        append({k: v[clone] for k, v in P.items()}, source[clone], torch.ones(n_clone, dtype=torch.long, device=dev))
        zero_stats()
        # densify_and_split: the gradients are zero-padded for the cloned rows
        n = P["xyz"].shape[0]
        padded = torch.zeros(n, dtype=dtype, device=dev)
        padded[:N] = grads.squeeze()
        scaling = torch.exp(P["scaling"])
        sel = (padded >= grad_threshold) & (scaling.max(dim=1).values > percent_dense * extent)
        split = sel[:N].clone()
        assert not bool(sel[N:].any())
        stds = scaling[sel].repeat(2, 1)
        samples = normals.to(dtype)[:, split].reshape(-1, 3) * stds
        rots = build_rotation(P["rotation"][sel]).repeat(2, 1, 1)
        new = {k: v[sel].repeat(2, *([1] * (v.dim() - 1))) for k, v in P.items()}
        new["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + P["xyz"][sel].repeat(2, 1)
        new["scaling"] = torch.log(scaling[sel].repeat(2, 1) / (0.8 * 2))
        n_src = int(sel.sum())
        src = source[sel]
        append(new, torch.cat([src, src]), torch.cat([torch.full_like(src, 2), torch.full_like(src, 3)]))
        zero_stats()
        remove(torch.cat([sel, torch.zeros(2 * n_src, dtype=torch.bool, device=dev)]))
    if do_reset:
        o = torch.sigmoid(P["opacity"])
        new = torch.minimum(o, torch.full_like(o, 0.01))
        P["opacity"] = torch.log(new / (1 - new))
        if "opacity" in M:
            M["opacity"] = tuple(torch.zeros_like(t) for t in M["opacity"])
    if do_prune:
        o = torch.sigmoid(P["opacity"])
        mask = (o < min_opacity).squeeze(-1)
        if max_screen_size:
            big_vs = S["max_radii2D"] > max_screen_size
            big_ws = torch.exp(P["scaling"]).max(dim=1).values > 0.1 * extent
            mask = mask | big_vs | big_ws
        n_pruned = int(mask.sum())
        remove(mask)
    return SimpleNamespace(state=P, moments=M, stats=S, n_clone=n_clone, n_src=n_src, n_pruned=n_pruned, clone=clone, split=split,
                           source=source, segment=segment)


def margins(state, stats, *, grad_threshold, percent_dense, extent, min_opacity, max_screen_size, do_densify, do_reset):
    """Every quantity a selection compares, as its ratio to the threshold it is compared with, in float64: [N, k].  A test whose
    ratios are all <= 0.5 or >= 2 can not have a selection flip on the rounding of exp / sigmoid / the division."""
    f = lambda t: t.detach().double()       # noqa: E731
    smax = torch.exp(f(state["scaling"])).max(dim=1).values
    cols = []
    if do_densify:
        accum, denom = f(stats["accum"]).squeeze(-1), f(stats["denom"]).squeeze(-1)
        cols += [torch.where(denom > 0, accum / denom.clamp_min(1), torch.zeros_like(accum)) / grad_threshold, smax / (percent_dense * extent)]
    o = torch.sigmoid(f(state["opacity"]).squeeze(-1))
    if do_reset:
        o = torch.minimum(o, torch.full_like(o, 0.01))
    cols.append(o / min_opacity)
    if max_screen_size:
        cols += [smax / (0.1 * extent), smax / 1.6 / (0.1 * extent)]
        if not do_densify:
            cols.append(f(stats["max_radii2D"]) / max_screen_size)
    return torch.stack(cols, dim=1)
