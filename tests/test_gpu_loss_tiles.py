"""-m gpu: the one-kernel loss (gp_loss_l1_ssim_fused) against the pair of kernels at the sizes where its staging and its item
layout can go wrong: images smaller than a tile, one pixel short of and past a tile edge in each direction, workgroups whose staged
rectangle lies inside the image (they stage whole rows without bounds work) next to workgroups at the image's edges in one launch,
and the benchmark's size, where the interior path dominates.  Same body as test_one_kernel_loss_equals_the_pair_of_kernels: image
gradient, L1 sums and the regulariser's gradient bit-equal, SSIM sums within 2e-6 relative.

(74, 75) has exactly ONE interior workgroup (tile (1, 1): staged rows 22 .. 73 end on the image's last row, staged columns 22 .. 73
one short of its last column); at (70, 129) every workgroup is an edge workgroup, two of them with all staged columns inside."""
import ctypes as C

import pytest
import torch

from gaussianprediction_amd import _lib

pytestmark = pytest.mark.gpu

N_FEAT = 250 * 32


def _fused_equals_pair(H, W):
    gen = torch.Generator().manual_seed(H * 1000 + W)
    img = torch.rand(3, H, W, generator=gen).cuda()
    gt = (img.cpu() + 0.1 * torch.randn(3, H, W, generator=gen)).clamp(0, 1).cuda()
    x = (torch.randn(N_FEAT, generator=gen) * 1e-3).cuda()
    L = _lib.lib()
    slots = 3 * ((W + 31) // 32) * ((H + 31) // 32)
    s = _lib.stream_ptr(img.device)
    i32, f32 = C.c_int32, C.c_float
    sums_a = torch.full((2 * slots,), float("nan"), dtype=torch.float64, device="cuda")
    sums_b = torch.full((2 * slots,), float("nan"), dtype=torch.float64, device="cuda")
    dmaps = torch.empty(9 * H * W, device="cuda")
    d_a, d_b = torch.full_like(img, float("nan")), torch.full_like(img, float("nan"))
    gx_a, gx_b = torch.empty_like(x), torch.empty_like(x)
    up = torch.tensor([3.0], device="cuda")
    _lib.check(L.gp_loss_l1_ssim_forward(_lib.ptr(img), _lib.ptr(gt), i32(3), i32(H), i32(W), _lib.ptr(sums_a), _lib.ptr(dmaps), s), "fwd")
    _lib.check(L.gp_loss_l1_ssim_backward_reg(_lib.ptr(img), _lib.ptr(gt), _lib.ptr(dmaps), i32(3), i32(H), i32(W), f32(0.2), _lib.ptr(up), _lib.ptr(d_a),
                                              _lib.ptr(x), C.c_int64(N_FEAT), f32(1e-5), _lib.ptr(gx_a), s), "bwd")
    _lib.check(L.gp_loss_l1_ssim_fused(_lib.ptr(img), _lib.ptr(gt), i32(3), i32(H), i32(W), f32(0.2), _lib.ptr(up), _lib.ptr(sums_b), _lib.ptr(d_b),
                                       _lib.ptr(x), C.c_int64(N_FEAT), f32(1e-5), _lib.ptr(gx_b), s), "fused")
    torch.cuda.synchronize()
    ssim_rel = float(((sums_a[1::2] - sums_b[1::2]).abs() / sums_a[1::2].abs().clamp_min(1.0)).max())
    print(H, W, "ssim sums rel", ssim_rel)
    assert torch.equal(sums_a[0::2], sums_b[0::2])      # sum |a - b| per tile: same pixels per thread, same order
    assert ssim_rel < 2e-6                              # sum ssim per tile: fp32, another order
    assert torch.equal(d_a, d_b)
    assert torch.equal(gx_a, gx_b)


@pytest.mark.parametrize("H,W", [(5, 7), (63, 65), (65, 63), (96, 40), (40, 96), (70, 129), (74, 75)])
def test_fused_loss_equals_the_pair_at_tile_and_image_edges(H, W):
    _fused_equals_pair(H, W)


def test_fused_loss_equals_the_pair_where_interior_workgroups_dominate():
    _fused_equals_pair(1014, 1352)


def test_fused_loss_carries_the_backward_prologue_through_the_fused_step():
    """The kernel inside gp_train_step_run at a small size with rider A armed (gp_debug_option(15, 6): the composite backward's tile
    order as the launch's first workgroup, its accumulators zeroed by the loss workgroups) against the schedule with every rider off
    (the stand-alone prologue: gp_tile_order_kernel and a fill).  Neither the accumulators nor the order are reachable through the C
    ABI after a step -- the backward has consumed them -- so this checks what they decide: the loss bit for bit, and the gradients (read
    as Adam's moments at zero learning rates) up to the order of the backward's float atomics.  An accumulator left unzeroed, or an
    order that is no permutation of the tiles, moves the moments by far more than the bound (5e-5 relative, test_gpu_step_riders.py)."""
    from test_gpu_step_riders import _fused_steps, _riders
    try:
        loss_on, mom_on = _fused_steps(250, 6, steps=2)
        loss_off, mom_off = _fused_steps(250, 7, steps=2)
    finally:
        _riders(0)
    assert loss_on == loss_off
    assert mom_on.keys() == mom_off.keys()
    for k in mom_on:
        for which, a, b in zip(("exp_avg", "exp_avg_sq"), mom_on[k], mom_off[k]):
            e = float((a - b).norm() / b.norm().clamp_min(1e-30))
            print(k, which, e)
            assert e < 5e-5, (k, which, e)
