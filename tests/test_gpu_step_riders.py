"""-m gpu: the riders of the fused train step (gp_train_step_run; gp_debug_option(15, bits): bit 0 / 1 / 2 switch rider A / B / C off).
A = the composite backward's prologue inside the fused loss launch, B = the loss finalize as a workgroup of the keypoint blend's
backward launch, C = the Adam chunks of _scaling / _opacity inside that same launch.  The riders move work between launches and
change no arithmetic: losses are bit-identical, gradients agree up to the order of the backward's float atomics, the optimizer's
element-wise update is bit-identical to gp_adam_step_multi_steps."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from gaussianprediction_amd import _lib  # noqa: E402
from gaussianprediction_amd.fused_step import FusedStage3  # noqa: E402
from gaussianprediction_amd.train_step import TrainStep  # noqa: E402
from test_gpu_training_api import build  # noqa: E402

ZERO = dict(xyz=0.0, f_dc=0.0, opacity=0.0, scaling=0.0, rotation=0.0, kpts=0.0, mlp=0.0)
ALL_ON, ALL_OFF = 0, 7


def _riders(bits):
    _lib.check(_lib.lib().gp_debug_option(15, int(bits)), "gp_debug_option")


@pytest.fixture(autouse=True)
def _riders_back_on():
    yield
    _riders(ALL_ON)


def _train_step(K, lrs, n=6000):
    pc, cams, gts, raw, rw, idx, args = build(n=n, K=K, max_points=K)
    ts = TrainStep(pc, cams, gts, 50000, lrs=lrs, speculative=True, fused=True)
    pre = len(cams) + TrainStep.SPEC_SLOTS                     # exact-mode set-up steps (graph path)
    for i in range(pre):
        ts.step(i)
    assert ts.fused_steps == 0
    return pc, ts, pre, len(cams)


def _fused_steps(K, bits, steps=3):
    pc, ts, pre, _ = _train_step(K, ZERO)
    _riders(bits)
    losses = [float(ts.step(pre + i)[0]) for i in range(steps)]
    torch.cuda.synchronize()
    assert ts.fused_steps == steps and ts.redone == 0
    sd = pc.optimizer.state_dict()
    return losses, {k: (v["exp_avg"].clone(), v["exp_avg_sq"].clone()) for k, v in sd["state"].items()}


@pytest.mark.parametrize("K", [250, 600])       # (600: the K > 512 Adam rider of the MLP's data backward travels too)
def test_riders_change_no_loss_and_no_gradient(K):
    """Zero learning rates, three fused steps from one seeded state: all riders on against all riders off."""
    loss_on, mom_on = _fused_steps(K, ALL_ON)
    loss_off, mom_off = _fused_steps(K, ALL_OFF)
    print("losses", loss_on, loss_off)
    assert loss_on == loss_off
    assert mom_on.keys() == mom_off.keys()
    for k in mom_on:
        for which, x, y in zip(("exp_avg", "exp_avg_sq"), mom_on[k], mom_off[k]):
            e = float((x - y).norm() / y.norm().clamp_min(1e-30))
            print(K, k, which, e)
            assert e < 5e-5, (k, which, e)


def _items_of(pc, opt):
    return {id(p): (g, p, off, m, v) for g, p, off, m, v in opt.items if p is pc._scaling or p is pc._opacity}


def test_adam_through_the_blend_carrier_equals_the_optimizer_launch():
    """Real learning rates, one step: _scaling / _opacity updated inside the blend backward's launch against gp_adam_step_multi_steps on
    copies of the same (p, g, m, v).  (The fused step keeps these gradients -- keep_grad_mask -- so g can be read back after the step.)"""
    pc, ts, pre, _ = _train_step(250, None)
    _riders(ALL_ON)
    ts.step(pre)                                    # (moments away from zero)
    torch.cuda.synchronize()
    opt = pc.optimizer
    items = _items_of(pc, opt)
    assert len(items) == 2
    before = {k: (p.detach().clone(), m.clone(), v.clone()) for k, (g, p, off, m, v) in items.items()}
    ts.step(pre + 1)
    torch.cuda.synchronize()
    assert ts.fused_steps == 2 and ts.redone == 0
    b1, b2 = opt.betas
    for k, (g, p, off, m, v) in items.items():
        p0, m0, v0 = before[k]
        assert m.shape == p.shape and not torch.equal(p0, p.detach())
        g0 = opt.bucket.flat[off:off + p.numel()].clone()
        assert float(g0.abs().max()) > 0.0
        step = opt.step_count - opt.lag_of(g)
        arr = lambda t: (C.c_void_p * 1)(t.data_ptr())
        rc = _lib.lib().gp_adam_step_multi_steps(C.c_int32(1), arr(p0), arr(g0), arr(m0), arr(v0), (C.c_int64 * 1)(p.numel()),
                                                 (C.c_float * 1)(float(g["lr"])), (C.c_int64 * 1)(step), C.c_float(b1), C.c_float(b2),
                                                 C.c_float(opt.eps), C.c_int32(1), C.c_uint32(0), None, _lib.stream_ptr(p.device))
        _lib.check(rc, "gp_adam_step_multi_steps")
        torch.cuda.synchronize()
        assert torch.equal(p0, p.detach()) and torch.equal(m0, m) and torch.equal(v0, v), g.get("name")
        assert float(g0.abs().max()) == 0.0


def test_adam_through_the_blend_carrier_zeroes_the_gradients_it_owns(monkeypatch):
    """The same step with _scaling / _opacity taken out of the kept gradients: the carrier's chunks zero them, as the optimizer launch does."""
    pc, ts, pre, _ = _train_step(250, None)
    _riders(ALL_ON)
    orig = FusedStage3.run

    def run(self, view, time_tensor, capacity, status, skip_flag, keep, depth_key=None):
        keep = tuple(t for t in keep if t is not pc._scaling and t is not pc._opacity)
        return orig(self, view, time_tensor, capacity, status, skip_flag, keep, depth_key=depth_key)

    monkeypatch.setattr(FusedStage3, "run", run)
    before = {id(p): p.detach().clone() for p in (pc._scaling, pc._opacity)}
    ts.step(pre)
    torch.cuda.synchronize()
    assert ts.fused_steps == 1 and ts.redone == 0
    for k, (g, p, off, m, v) in _items_of(pc, pc.optimizer).items():
        assert float(pc.optimizer.bucket.flat[off:off + p.numel()].abs().max()) == 0.0, g.get("name")
        assert not torch.equal(before[k], p.detach())


def test_each_rider_alone():
    """Every bit of option 15 on its own: the step runs, nothing is redone, and -- at zero learning rates, on one view -- the loss is the
    all-off schedule's (a disabled rider must not leave a half-armed slot behind for the next step)."""
    pc, ts, pre, ncam = _train_step(250, ZERO)
    losses = {}
    for j, bits in enumerate((ALL_OFF, 1, 2, 4, 3, 5, 6, ALL_ON, ALL_OFF)):
        _riders(bits)
        losses[(j, bits)] = float(ts.step(pre + j * ncam)[0])          # (the same view every time)
    torch.cuda.synchronize()
    print(losses)
    assert ts.fused_steps == 9 and ts.redone == 0
    ref = losses[(0, ALL_OFF)]
    assert ref > 0.0 and all(v == ref for v in losses.values()), losses


def test_skipped_frame_keeps_its_loss_and_leaves_the_parameters():
    """Capacity below R: the skip flag is raised on the device.  Parameters untouched, the loss is still written, the next step is a
    normal one."""
    pc, ts, pre, ncam = _train_step(250, None)
    _riders(ALL_ON)
    loss, _ = ts.step(pre)
    torch.cuda.synchronize()
    params = {n: p.detach().clone() for n, p in pc.named_parameters()}
    margin, pad = ts.SPEC_MARGIN, ts.SPEC_PAD
    ts.SPEC_MARGIN, ts.SPEC_PAD = 0.5, 0
    ts._fused_plan.buf["loss"].fill_(float("nan"))  # (the plan's own loss buffer: the skipped frame must overwrite it)
    loss2, _ = ts.step(pre + 1)
    torch.cuda.synchronize()
    ts.SPEC_MARGIN, ts.SPEC_PAD = margin, pad
    assert ts.fused_steps == 2
    assert int(ts._status[(ts._n_steps - 1) % ts.SPEC_SLOTS, 1]) != 0            # the frame did overflow
    assert bool(torch.isfinite(loss2)) and float(loss2) > 0.0
    for n, p in pc.named_parameters():
        assert torch.equal(params[n], p.detach()), n
    loss3, _ = ts.step(pre + 2)
    torch.cuda.synchronize()
    assert ts.fused_steps == 3 and bool(torch.isfinite(loss3)) and float(loss3) > 0.0
    assert int(ts._status[(ts._n_steps - 1) % ts.SPEC_SLOTS, 1]) == 0
    assert not torch.equal(params["_xyz"], pc._xyz.detach()) and not torch.equal(params["_scaling"], pc._scaling.detach())


def test_finalize_reads_the_keypoint_features_before_the_optimizer_moves_them():
    """Real learning rates, regulariser on (iteration >= jointly_iteration): the loss of a step with the riders equals, bit for bit, the
    loss the all-off schedule gives from the same parameters on the same view."""
    pc, ts, pre, ncam = _train_step(250, None)
    assert ts.iteration >= pc.args.jointly_iteration
    _riders(ALL_ON)
    ts.step(pre)
    torch.cuda.synchronize()
    params = {n: p.detach().clone() for n, p in pc.named_parameters()}
    feat = pc.super_gaussians_feature.detach().clone()
    loss_on = float(ts.step(pre + 1)[0])
    torch.cuda.synchronize()
    assert not torch.equal(feat, pc.super_gaussians_feature.detach())            # (the optimizer did move them)
    with torch.no_grad():
        for n, p in pc.named_parameters():
            p.copy_(params[n])
    _riders(ALL_OFF)
    loss_off = float(ts.step(pre + 1 + ncam)[0])
    torch.cuda.synchronize()
    print(loss_on, loss_off)
    assert ts.fused_steps == 3 and ts.redone == 0
    assert loss_on == loss_off
