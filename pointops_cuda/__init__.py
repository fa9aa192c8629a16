"""Import-name shim: `import pointops_cuda` [REF utils/fps.py:8] resolves to HIP kernels.  Only the two entry points the reference
reaches exist: `furthestsampling_cuda` [REF utils/fps.py:84] (gp_furthest_point_sampling_batched) and `knnquery_cuda`
[REF utils/fps.py:104] (gp_knn_points on the batches of the offsets).  Both write into their output tensors, as pointops does.

pointops' conventions: offsets are cumulative ends, indices are global, every batch of the sampling starts at its first point;
knnquery pads missing neighbours with the batch's first index and dist2 1e10.  Parity with the real pointops is unpinned: the
compiled package is absent, so this follows its source's semantics and has never been compared against it."""


def furthestsampling_cuda(b, n_max, xyz, offset, new_offset, tmp, idx):
    """idx[new_offset[-1]] (int32) <- furthest-point samples of each batch.  n_max (the largest batch) is not needed."""
    from gaussianprediction_amd.knn_ops import furthest_point_sampling_batched
    if int(b) != offset.shape[0] or int(b) != new_offset.shape[0]:
        raise ValueError("furthestsampling_cuda: b must equal len(offset) == len(new_offset)")
    furthest_point_sampling_batched(xyz, offset, new_offset, tmp=tmp, idx=idx)


def knnquery_cuda(m, nsample, xyz, new_xyz, offset, new_offset, idx, dist2):
    """idx[m, nsample] (int32, global) / dist2[m, nsample] <- the nsample nearest points of xyz's batch to every new_xyz point."""
    import torch
    from gaussianprediction_amd.knn_ops import knn_points
    ends = [int(v) for v in offset.cpu()]
    new_ends = [int(v) for v in new_offset.cpu()]
    if len(ends) != len(new_ends) or new_ends[-1] != int(m) or new_xyz.shape[0] != int(m):
        raise ValueError("knnquery_cuda: offsets disagree with m")
    starts, new_starts = [0] + ends[:-1], [0] + new_ends[:-1]
    cand = torch.nn.utils.rnn.pad_sequence([xyz[s:e] for s, e in zip(starts, ends)], batch_first=True).contiguous()
    qry = torch.nn.utils.rnn.pad_sequence([new_xyz[s:e] for s, e in zip(new_starts, new_ends)], batch_first=True).contiguous()
    l1 = torch.tensor([e - s for s, e in zip(new_starts, new_ends)], dtype=torch.int64, device=xyz.device)
    l2 = torch.tensor([e - s for s, e in zip(starts, ends)], dtype=torch.int64, device=xyz.device)
    d, i = knn_points(qry, cand, lengths1=l1, lengths2=l2, K=int(nsample), pad_idx=0, pad_dist=1e10)
    i = i + torch.tensor(starts, dtype=torch.int64, device=xyz.device).view(-1, 1, 1)
    rows = torch.cat([torch.arange(e - s, device=xyz.device) + bi * qry.shape[1] for bi, (s, e) in enumerate(zip(new_starts, new_ends))])
    idx.copy_(i.reshape(-1, int(nsample))[rows].to(torch.int32))
    dist2.copy_(d.reshape(-1, int(nsample))[rows])
