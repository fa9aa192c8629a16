"""The keypoint motion predictor: the reference's GCN_xyzr on this package's HIP layer kernels, its dataset, its training loop, the
autoregressive rollout and the render of predicted keypoints.

  [REF motion_model/gcn.py:108-286]      GraphConvolution, GC_Block, GCN, Channel_GCN, GCN_xyzr, get_dct_matrix
  [REF motion_model/dataset.py:11-192]   GCN3DDataset (train / test windows; the `val` split, which nothing reads, is not built)
  [REF train_GCN.py:19-43, 55-176]       operate(), the training loop, the prediction loops (-> GCN_xyzr.rollout)
  [REF eval.py:120-157]                  render_kpts

Constructor signatures, parameter / buffer names and the state_dict() key order are the reference's: a `ckpt.pth` written by either side
loads on the other.  Every layer runs through gcn_ops.layer (gp_gcn_layer_forward / _backward); train() / eval() select the BatchNorm
mode; a gradient through eval mode raises.  Not provided: SemskeConv, _GraphConv, Generator (no entry point reaches them), dropout
(p_dropout > 0 raises NotImplementedError; the reference ships 0)."""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.parameter import Parameter

from . import gcn_ops
from .gcn_ops import ACT_NONE, ACT_RELU, ACT_TANH


def _no_dropout(p_dropout):
    if p_dropout is not None and p_dropout > 0:
        raise NotImplementedError(f"p_dropout = {p_dropout}: dropout is not implemented on the HIP layer (the reference ships p_dropout = 0)")


def _bn(bn: nn.BatchNorm1d):
    return bn.weight, bn.bias, bn.running_mean, bn.running_var


def _bn_layer(x, gc, bn, residual=None):
    """tanh(bn(gc(x))) [+ residual] in one layer call; train mode counts the batch as nn.BatchNorm1d does."""
    y = gcn_ops.layer(x, gc.weight, gc.att, gc.bias, bn=_bn(bn), training=bn.training, act=ACT_TANH, residual=residual)
    if bn.training:
        bn.num_batches_tracked += 1
    return y


class GraphConvolution(nn.Module):
    """att @ (input @ weight) + bias [REF motion_model/gcn.py:108-143]."""

    def __init__(self, in_features, out_features, bias=True, node_n=48):
        super(GraphConvolution, self).__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.weight = Parameter(torch.empty(in_features, out_features))
        self.att = Parameter(torch.empty(node_n, node_n))
        if bias:
            self.bias = Parameter(torch.empty(out_features))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        """U(-s, s) with s = 1 / sqrt(out_features) for the weight, the adjacency and the bias, drawn in that order."""
        bound = 1.0 / math.sqrt(self.out_features)
        with torch.no_grad():
            for p in (self.weight, self.att, self.bias):
                if p is not None:
                    p.uniform_(-bound, bound)

    def forward(self, input):
        return gcn_ops.layer(input.contiguous(), self.weight, self.att, self.bias)

    def __repr__(self):
        return f"{type(self).__name__} ({self.in_features} -> {self.out_features})"


class GC_Block(nn.Module):
    def __init__(self, in_features, p_dropout, bias=True, node_n=48):
        """A residual block of two graph convolutions [REF motion_model/gcn.py:146-182]."""
        super(GC_Block, self).__init__()
        _no_dropout(p_dropout)
        self.in_features = in_features
        self.out_features = in_features
        self.gc1 = GraphConvolution(in_features, in_features, node_n=node_n, bias=bias)
        self.bn1 = nn.BatchNorm1d(node_n * in_features)
        self.gc2 = GraphConvolution(in_features, in_features, node_n=node_n, bias=bias)
        self.bn2 = nn.BatchNorm1d(node_n * in_features)
        self.do = nn.Dropout(p_dropout)
        self.act_f = nn.Tanh()

    def forward(self, x):
        x = x.contiguous()
        y = _bn_layer(x, self.gc1, self.bn1)
        return _bn_layer(y, self.gc2, self.bn2, residual=x)

    def __repr__(self):
        return f"{type(self).__name__} ({self.in_features} -> {self.out_features})"


class GCN(nn.Module):
    def __init__(self, input_feature, hidden_feature, output_feature, p_dropout, num_stage=1, node_n=48, no_mapping=False):
        """[REF motion_model/gcn.py:185-235]"""
        super(GCN, self).__init__()
        _no_dropout(p_dropout)
        self.num_stage = num_stage
        self.gc1 = GraphConvolution(input_feature, hidden_feature, node_n=node_n)
        self.bn1 = nn.BatchNorm1d(node_n * hidden_feature)
        self.gcbs = nn.ModuleList(GC_Block(hidden_feature, p_dropout=p_dropout, node_n=node_n) for _ in range(num_stage))
        # the head: keys gc_out.{weight, att, bias} under no_mapping, gc_out.0.* / gc_out.2.* otherwise
        self.gc_out = (GraphConvolution(hidden_feature, output_feature, node_n=node_n) if no_mapping else
                       nn.Sequential(nn.Linear(hidden_feature, hidden_feature), nn.ReLU(), nn.Linear(hidden_feature, output_feature)))
        self.do = nn.Dropout(p_dropout)
        self.act_f = nn.Tanh()

    @property
    def no_mapping(self):
        return isinstance(self.gc_out, GraphConvolution)

    def forward(self, x):
        y = _bn_layer(x.contiguous(), self.gc1, self.bn1)
        for i in range(self.num_stage):
            y = self.gcbs[i](y)
        if self.no_mapping:
            return self.gc_out(y)
        l0, l2 = self.gc_out[0], self.gc_out[2]
        y = gcn_ops.layer(y, l0.weight, None, l0.bias, act=ACT_RELU, w_transposed=True)
        return gcn_ops.layer(y, l2.weight, None, l2.bias, act=ACT_NONE, w_transposed=True)

    def rollout_entries(self):
        """The rows of gp_gcn_rollout's pointer table for this network (include/gp_gcn.h)."""
        rows = [(self.gc1.weight, self.gc1.att, self.gc1.bias) + _bn(self.bn1)]
        for blk in self.gcbs:
            rows.append((blk.gc1.weight, blk.gc1.att, blk.gc1.bias) + _bn(blk.bn1))
            rows.append((blk.gc2.weight, blk.gc2.att, blk.gc2.bias) + _bn(blk.bn2))
        if self.no_mapping:
            rows.append((self.gc_out.weight, self.gc_out.att, self.gc_out.bias, None, None, None, None))
        else:
            for lin in (self.gc_out[0], self.gc_out[2]):
                rows.append((lin.weight, None, lin.bias, None, None, None, None))
        return [tuple(None if t is None else t.detach() for t in r) for r in rows]


class Channel_GCN(nn.Module):
    def __init__(self, input_feature, hidden_feature, output_feature, p_dropout, num_stage=1, node_n=48, channel=3, no_mapping=False):
        super().__init__()
        self.channel = channel
        self.output_feature = output_feature
        self.GCN = GCN(input_feature, hidden_feature, output_feature, p_dropout, num_stage, node_n*channel, no_mapping)

    def forward(self, x):
        """x (B, channel, nodes, input_feature) -> (B, channel, nodes, output_feature): one graph over channel * nodes vertices."""
        B, C, N, T = x.shape
        return self.GCN(x.reshape(B, C * N, T)).reshape(B, C, N, self.output_feature)


class GCN_xyzr(nn.Module):
    def __init__(self, input_feature, hidden_feature, output_feature, p_dropout, num_stage=1, node_n=48, no_mapping=False):
        super().__init__()
        self.output_feature = output_feature
        self.GCN_xyz = Channel_GCN(input_feature, hidden_feature, output_feature, p_dropout, num_stage, node_n, 3, no_mapping)
        self.GCN_r = Channel_GCN(input_feature, hidden_feature, output_feature, p_dropout, num_stage, node_n, 4, no_mapping)

    def forward(self, x, r):
        """x (B, 3, nodes, T), r (B, 4, nodes, T) -> (B, 3, nodes, out), (B, 4, nodes, out); the rotation is normalised over its
        four channels (torch: F.normalize(dim=1))."""
        return self.GCN_xyz(x), F.normalize(self.GCN_r(r), dim=1)

    @torch.no_grad()
    def rollout(self, xyz_inputs, rotation_inputs, frames, output_size, norm_rotation, base_xyz=None):
        """The prediction loop of [REF train_GCN.py:126-143, 165-176] in one call of gp_gcn_rollout: from the last window
        xyz_inputs [T, K, 3] / rotation_inputs [T, K, 4] (a leading batch dimension of 1 is accepted), `frames` times: predict
        `output_size` rows, append them to the window.  Returns (kpts [frames * output_size, K, 3], kpts_rotation [.., K, 4]) and, with
        base_xyz [K, 3] (the model's super_gaussians), also delta [.., K, 7] = (kpts - base_xyz, kpts_rotation): the rows
        KeypointBlend reads.  Needs eval mode."""
        if self.training:
            raise RuntimeError("GCN_xyzr.rollout needs eval mode (call .eval()): the rollout runs on the running statistics")
        if int(output_size) != self.output_feature:
            raise ValueError(f"GCN_xyzr.rollout: output_size = {output_size}, the model predicts {self.output_feature} rows per frame")
        g = self.GCN_xyz.GCN
        if xyz_inputs.dim() == 4 and xyz_inputs.shape[0] == 1:
            xyz_inputs, rotation_inputs = xyz_inputs[0], rotation_inputs[0]
        T, K = g.gc1.in_features, g.gc1.att.shape[0] // 3
        keep = [g.rollout_entries(), self.GCN_r.GCN.rollout_entries()]
        table = gcn_ops.rollout_table(keep)
        out = gcn_ops.rollout(table, K, T, g.gc1.out_features, g.num_stage, self.output_feature, g.no_mapping,
                              xyz_inputs.float().contiguous(), rotation_inputs.float().contiguous(), frames, norm_rotation,
                              None if base_xyz is None else base_xyz.detach().float().contiguous())
        return out if base_xyz is not None else out[:2]


def get_dct_matrix(N):
    """(dct, idct): the orthonormal DCT-II matrix of size N, dct[k, i] = w_k cos(pi (i + 1/2) k / N) with w_0 = sqrt(1 / N) and
    w_k = sqrt(2 / N), and its inverse (float64 numpy) [REF motion_model/gcn.py:277-286; train_GCN.py:69 builds both]."""
    k, i = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    scale = np.where(k == 0, np.sqrt(1 / N), np.sqrt(2 / N))
    dct_m = scale * np.cos(np.pi * (i + 1 / 2) * k / N)
    return dct_m, np.linalg.inv(dct_m)


# ---- the dataset [REF motion_model/dataset.py] ----------------------------------------------------------------------------------------
@torch.no_grad()
def keypoint_trajectories(model, times, iteration):
    """(kpts_xyz [len(times), K, 3], kpts_r [len(times), K, 4]): the keypoints' positions and rotations at every time, from the K-row
    MLP pass alone (GaussianModel.keypoint_motion) -- the values the reference reads off a whole forward per time
    [REF motion_model/dataset.py:117-135]."""
    dev = model.super_gaussians.device
    xyz, rot = [], []
    for t in times:
        x, r = model.keypoint_motion(torch.tensor([float(t)], dtype=torch.float32, device=dev), iteration)
        xyz.append(x), rot.append(r)
    return torch.stack(xyz, dim=0), torch.stack(rot, dim=0)


def load_dnerf_times(source_path, max_time):
    """[REF motion_model/dataset.py:76-85]: transforms_train.json, split at max_time, in file order."""
    with open(os.path.join(source_path, "transforms_train.json"), "r") as f:
        frames = json.load(f)["frames"]
    times = [float(fr["time"]) for fr in frames]
    return [t for t in times if t < max_time], [t for t in times if not t < max_time]


def load_hyper_times(source_path, max_time):
    """[REF motion_model/dataset.py:31-74]: metadata.json + dataset.json; time = warp_id / max warp_id; without val_ids every fourth
    image trains (idx % 4 == 0) and the images two after them test; with val_ids the train_ids / val_ids lists decide."""
    with open(os.path.join(source_path, "metadata.json"), "r") as f:
        meta = json.load(f)
    with open(os.path.join(source_path, "dataset.json"), "r") as f:
        ds = json.load(f)
    ids, val_ids = ds["ids"], ds["val_ids"]
    train_ids = ds["train_ids"] if len(val_ids) else None
    top = max(meta[i]["warp_id"] for i in ids)
    all_time, i_train, i_test = [], [], []
    for idx, i in enumerate(ids):
        time = meta[i]["warp_id"] / top
        all_time.append(time)
        if train_ids is None:
            if idx % 4 == 0 and time < max_time:
                i_train.append(idx)
            if (idx - 2) % 4 == 0 and time >= max_time:
                i_test.append(idx)
        else:
            if i in val_ids and time >= max_time:
                i_test.append(idx)
            if i in train_ids and time < max_time:
                i_train.append(idx)
    if not i_train or not i_test:
        raise ValueError(f"GCN3DDataset: max_time = {max_time} leaves {len(i_train)} training and {len(i_test)} test times")
    return [all_time[i] for i in i_train], [all_time[i] for i in i_test]


class GCN3DDataset(torch.utils.data.Dataset):
    """The reference's constructor arguments, `nodes_num`, train / test windows and item keys.  A D-NeRF scene is recognised as the
    reference does ("d-nerf" or "white" in model_path), or by a transforms_train.json beside no metadata.json."""

    def __init__(self, gaussians, time_freq, iteration, model_path, source_path, max_time=0.8, input_size=20, output_size=5, split="train"):
        super().__init__()
        self.gaussians = gaussians
        self.time_freq = time_freq
        self.iteration = iteration
        self.split = split
        self.max_time = max_time
        assert self.max_time < 1.0
        if split not in ("train", "test"):
            raise NotImplementedError(f"GCN3DDataset: split = {split!r} (the reference's 'val' split is read by nothing and is not built)")
        self.input_size = input_size
        self.output_size = output_size
        self.model_path = model_path
        self.source_path = source_path
        self.train_data, self.test_data, self.val_data = [], [], []
        self.load_times()
        self.generate_data()
        self.get_lens()
        self.prepare_item()

    def load_times(self):
        dnerf = "d-nerf" in self.model_path or "white" in self.model_path
        if not dnerf and not os.path.exists(os.path.join(self.source_path, "metadata.json")):
            dnerf = os.path.exists(os.path.join(self.source_path, "transforms_train.json"))
        self.train_times, self.test_times = (load_dnerf_times if dnerf else load_hyper_times)(self.source_path, self.max_time)

    @property
    def nodes_num(self):
        return self.gaussians.super_gaussians.shape[0]

    def generate_data(self):
        self.kpts_xyz_train, self.kpts_r_train = keypoint_trajectories(self.gaussians, self.train_times, self.iteration)
        self.kpts_xyz_test, self.kpts_r_test = keypoint_trajectories(self.gaussians, self.test_times, self.iteration)

    def get_lens(self):
        self.train_lens = len(self.kpts_xyz_train) - self.input_size - self.output_size
        self.test_lens = len(self.kpts_xyz_test)
        self.val_lens = 2

    def prepare_item(self):
        T, O = self.input_size, self.output_size
        if self.split == "train":
            xyz, rot, times, n, step, dst = self.kpts_xyz_train, self.kpts_r_train, self.train_times, self.train_lens, 1, self.train_data
        else:
            xyz = torch.cat([self.kpts_xyz_train[-T:], self.kpts_xyz_test], dim=0)
            rot = torch.cat([self.kpts_r_train[-T:], self.kpts_r_test], dim=0)
            times, n, step, dst = self.train_times[-T:] + self.test_times, self.test_lens, O, self.test_data
        for i in range(0, n, step):
            dst.append({"xyz_inputs": xyz[i:i + T], "xyz_gt": xyz[i + T:i + T + O], "rotation_inputs": rot[i:i + T],
                        "rotation_gt": rot[i + T:i + T + O], "time": times[i + T] - times[i + T - 1]})

    def __len__(self):
        return len(self.train_data) if self.split == "train" else len(self.test_data)

    def __getitem__(self, index):
        return self.train_data[index] if self.split == "train" else self.test_data[index]


# ---- training [REF train_GCN.py:19-43, 76-114] ------------------------------------------------------------------------------------------
def operate(args, batch, model, eval=False, noise_xyz=0, noise_r=0):
    """[REF train_GCN.py:19-43].  The permutes and the normalise are torch."""
    if eval:
        model.eval()
    xyz_inputs, xyz_gt = batch["xyz_inputs"], batch["xyz_gt"]
    r_inputs, r_gt = batch["rotation_inputs"], batch["rotation_gt"]
    if noise_xyz > 0:
        xyz_inputs = xyz_inputs + (2 * torch.rand_like(xyz_inputs) - 1) * noise_xyz
    if noise_r > 0:
        r_inputs = r_inputs + (2 * torch.rand_like(r_inputs) - 1) * noise_r
        if args.norm_rotation:
            r_inputs = F.normalize(r_inputs, dim=-1)
    xyz_pred, r_pred = model(xyz_inputs.permute((0, 3, 2, 1)), r_inputs.permute((0, 3, 2, 1)))
    xyz_pred = xyz_pred.permute((0, 3, 2, 1))
    r_pred = r_pred.permute((0, 3, 2, 1))
    if args.norm_rotation:
        r_pred = F.normalize(r_pred, dim=-1)
    if eval:
        model.train()
    return xyz_pred, xyz_gt, r_pred, r_gt


def gcn_loss(xyz_pred, xyz_gt, r_pred, r_gt):
    """mean ||d xyz||_2 + mean ||d r||_2 [REF train_GCN.py:101]"""
    return torch.mean(torch.norm(xyz_pred - xyz_gt, 2, -1)) + torch.mean(torch.norm(r_pred - r_gt, 2, -1))


def train_iteration(args, model, optimizer, batch, noise_xyz=0., noise_r=0.):
    """One pass of the inner loop [REF train_GCN.py:100-105]; returns the loss (a device scalar)."""
    xyz_pred, xyz_gt, r_pred, r_gt = operate(args, batch, model, noise_xyz=noise_xyz, noise_r=noise_r)
    loss = gcn_loss(xyz_pred, xyz_gt, r_pred, r_gt)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return loss.detach()


def make_optimizer(args, model):
    """Adam(lr 0.01, eps 1e-15) with CosineAnnealingLR(T_max = epoch, eta_min 1e-4) [REF train_GCN.py:77-79]"""
    optimizer = torch.optim.Adam(model.parameters(), lr=0.01, eps=1e-15)
    return optimizer, torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=args.epoch, eta_min=1.e-4)


def train_gcn(args, dataset, model=None, device="cuda", generator=None, checkpoint=True, log=None):
    """The loop of [REF train_GCN.py:61-114] over a GCN3DDataset (split "train"): a shuffled DataLoader with drop_last, the decaying
    input noise, one scheduler step per epoch; the state_dict goes to <model_path>/<exp_name>/ckpt.pth (`checkpoint=False`: not
    written).  args: input_size, linear_size, output_size, dropout, num_stage, no_mapping, batch_size, epoch, noise_init, noise_step,
    norm_rotation (+ model_path, exp_name for the checkpoint).  `generator`: the DataLoader's shuffle generator.  `log` (a list):
    receives every epoch's mean loss.  Returns the model, in train mode."""
    loader = torch.utils.data.DataLoader(dataset, batch_size=args.batch_size, shuffle=True, drop_last=True, num_workers=0, generator=generator)
    if model is None:
        model = GCN_xyzr(input_feature=args.input_size, hidden_feature=args.linear_size, output_feature=args.output_size,
                         p_dropout=args.dropout, num_stage=args.num_stage, node_n=dataset.nodes_num,
                         no_mapping=args.no_mapping).to(device)
    model.train()
    optimizer, scheduler = make_optimizer(args, model)
    for epoch in range(args.epoch):
        loss_sum, count = None, 0
        for batch in loader:
            noise_xyz = noise_r = 0.
            if args.noise_init > 0:
                noise_xyz = args.noise_init * max(1. - epoch / args.noise_step, 0.)
                noise_r = args.noise_init * max((1. - epoch / args.noise_step), 0.) * 0.5
            loss = train_iteration(args, model, optimizer, batch, noise_xyz, noise_r)
            loss_sum = loss if loss_sum is None else loss_sum + loss
            count += 1
        if log is not None and count:
            log.append(float(loss_sum) / count)
        scheduler.step()
    if checkpoint:
        os.makedirs(os.path.join(args.model_path, args.exp_name), exist_ok=True)
        torch.save(model.state_dict(), os.path.join(args.model_path, args.exp_name, "ckpt.pth"))
    return model


# ---- rendering predicted keypoints [REF eval.py:120-157] ---------------------------------------------------------------------------
def _save_png(image, path):
    from PIL import Image
    a = (image.detach().clamp(0, 1).mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy())
    Image.fromarray(a).save(path)


@torch.no_grad()
def render_kpts(views, gaussians, pipeline, background, kpts, kpts_rotation, iteration, metrics=False, view_id=None, out_dir=None,
                delta=None, writer=None, video=None, fps=10):
    """Render every predicted frame: frame i's per-keypoint delta (kpts[i] - super_gaussians, kpts_rotation[i]) goes through the SPARSE
    blend (KeypointBlend, gp_blend_forward) with the weights and neighbour indices of ONE forward at views[0].time, then through
    render_motion with that forward's lifecycle opacity.  The reference multiplies two dense [N, K] weight matrices per frame
    [REF eval.py:140-141]; the sparse blend computes the same sums over the nearest_num non-zero weights.
    `delta` [F, K, 7] (GCN_xyzr.rollout's third output) replaces the subtraction and concatenation.
    View of frame i: views[i] with `metrics`, views[view_id] with `view_id`, else the reference's back-and-forth sweep over the first
    half of the views (its formula reads the builtin `id`; the frame index is what it means).
    Returns the list of images [3, H, W]; with out_dir also writes <out_dir>/renders[/view<id>]/%05d.png (and gt/ with metrics).
    writer: a png_ops.PngWriter; the files are then encoded on the device and written behind the loop (complete after the caller's
    writer.close()) instead of through the host encoder, frame by frame.
    video: True for <out_dir>/renders[/view<id>]/video.avi [REF train_GCN.py:45-53: renders/video.mp4 at 10 fps], or a path: the
    renderings then also go into a Motion-JPEG video at `fps`, encoded on the device (jpeg_ops.VideoWriter), complete on return."""
    from .deform_ops import KeypointBlend
    from .renderer import render_motion
    dev = gaussians.get_xyz.device
    time_ = torch.from_numpy(np.asarray(views[0].time)).to(torch.float32).to(dev)
    gaussians(time_, iteration)
    if gaussians._last_blend is None:
        raise RuntimeError("render_kpts needs a model past its second stage (iteration > second_stage_iter): keypoints drive the motion")
    raw_w, knn_idx, _ = gaussians._last_blend
    life_opacity = gaussians.lifecycle_opacity
    base = gaussians.super_gaussians.detach()
    render_path = gts_path = None
    if out_dir is not None:
        render_path = os.path.join(out_dir, "renders") if view_id is None else os.path.join(out_dir, "renders", f"view{view_id}")
        os.makedirs(render_path, exist_ok=True)
        if metrics:
            gts_path = os.path.join(out_dir, "gt")
            os.makedirs(gts_path, exist_ok=True)
    images = []
    vw = None
    if video is not None and video is not False:
        from .jpeg_ops import VideoWriter
        if video is True and render_path is None:
            raise ValueError("render_kpts: video=True needs out_dir (or pass the video's path)")
        vw = VideoWriter(os.path.join(render_path, "video.avi") if video is True else os.fspath(video), fps)
    save = _save_png if writer is None else writer.submit
    n = len(delta) if delta is not None else len(kpts)
    try:
        for i in range(n):
            d = delta[i] if delta is not None else torch.cat([kpts[i] - base, kpts_rotation[i]], dim=-1)
            xyz_final, delta_r = KeypointBlend.apply(d.contiguous(), raw_w, knn_idx, gaussians._xyz.detach(), gaussians._rotation.detach(), False)
            if metrics:
                view = views[i]
                if gts_path is not None:
                    save(view.original_image[0:3, :, :], os.path.join(gts_path, '{0:05d}'.format(i) + ".png"))
            elif view_id is not None:
                view = views[view_id]
            else:
                half = max(len(views) // 2, 1)
                position = 2 if ((i // half) % 2 == 0) else -2
                view = views[(i % half) * position]
            rendering = render_motion(view, gaussians, pipeline, background, xyz_t=xyz_final, r_t=delta_r, opacity=life_opacity)["render"]
            if render_path is not None:
                save(rendering, os.path.join(render_path, '{0:05d}'.format(i) + ".png"))
            images.append(rendering)
            if vw is not None and (len(images) % vw.slots == 0 or i == n - 1):
                vw.submit(images[len(images) - 1 - (len(images) - 1) % vw.slots:])       # (a ring of frames per encode)
    finally:
        if vw is not None:
            vw.close()
    return images
