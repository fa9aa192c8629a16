"""The projection backward with the SH coefficients' Adam step inside it (gp_adam_fuse) takes the coefficients from its LDS copy and
forms every gradient from its two per-Gaussian factors in the update's stream.  It must give, bit for bit, what the gradient-writing
path followed by the library's own Adam (gp_adam_step_multi, the shared device function) gives.

Determinism premise: with an 8 x 8 image there is one tile and one quadrant wave with pixels, every splat sits in exactly one of its
batches, so an accumulator line receives at most one atomic add and two backward calls agree in every bit (asserted first)."""
import ctypes as C

import numpy as np
import pytest
import torch

import gaussianprediction_amd as gpa
from gaussianprediction_amd import _lib, grad_sink
from gpu_util import torch_settings
from util import small_scene

pytestmark = pytest.mark.gpu

LR_DC, LR_REST, B1, B2, EPS = 2.5e-3, 1.25e-4, 0.9, 0.999, 1e-15
OTHER = ("means3D", "means2D", "opacities", "scales", "rotations")


def _scene(n, degree):
    """Fixed geometry, the SH pair with non-zero moments, image weights.  From 255 Gaussians on: one behind the camera, one exactly at
    the camera centre (zero-length view direction), ten whose colour clamps in one or two channels."""
    scene, st, _ = small_scene(n=n, W=8, H=8, seed=40 + n, sh_degree=degree)
    rs = torch_settings(st)
    fix = {k: scene[k].to(torch.float32).cuda() for k in ("means3D", "opacities", "scales", "rotations")}
    dc = scene["shs"][:, :1].to(torch.float32).cuda().contiguous()
    rest = scene["shs"][:, 1:].to(torch.float32).cuda().contiguous()
    if n == 1:
        fix["means3D"][0] = 0.0                  # (the cameras look at the origin)
    if n >= 255:
        fix["means3D"][0] = 2.0 * rs.campos
        fix["means3D"][1] = rs.campos
        for j in range(2, 12):
            fix["means3D"][j] = torch.tensor([0.15 * (j - 7), 0.1 * (j % 3 - 1), 0.0])
            dc[j, 0, j % 3] = -4.0
            if j % 2:
                dc[j, 0, (j + 1) % 3] = -4.0
    gen = torch.Generator(device="cuda").manual_seed(n)
    mom = {}
    for name, p in (("dc", dc), ("rest", rest)):
        mom["m_" + name] = 1e-3 * torch.randn(p.shape, device="cuda", generator=gen)
        mom["v_" + name] = 1e-6 * torch.rand(p.shape, device="cuda", generator=gen)
    w = torch.randn(3, 8, 8, device="cuda", generator=gen)
    return rs, fix, dict(dc=dc, rest=rest, **mom), w


def _backward(rs, fix, dc, rest, w, fuse=None):
    """One render + backward.  `fuse`: the payload of the in-kernel Adam step (dc / rest are then updated in place, no SH gradient)."""
    leaves = {k: v.clone().requires_grad_(True) for k, v in fix.items()}
    leaves["means2D"] = torch.zeros(dc.shape[0], 3, device="cuda", requires_grad=True)
    dc.requires_grad_(True); rest.requires_grad_(True)
    dc.grad = rest.grad = None
    if fuse is not None:
        grad_sink.arm_fused_update((dc, rest), fuse)
    try:
        img, radii, _, _ = gpa.GaussianRasterizer(raster_settings=rs)(
            means3D=leaves["means3D"], means2D=leaves["means2D"], opacities=leaves["opacities"], shs=dc, shs_rest=rest,
            scales=leaves["scales"], rotations=leaves["rotations"])
        (img * w).sum().backward()
    finally:
        taken = fuse is not None and not grad_sink.disarm_fused_update((dc, rest))
    torch.cuda.synchronize()
    assert taken == (fuse is not None), "the backward did not take the fused update"
    out = {k: leaves[k].grad.clone() for k in OTHER}
    if fuse is None:
        out["dc"], out["rest"] = dc.grad.clone(), rest.grad.clone()
    else:
        assert dc.grad is None and rest.grad is None
    dc.requires_grad_(False); rest.requires_grad_(False)
    return out, radii


def _library_adam(s, g_dc, g_rest, step):
    arr = lambda *t: (C.c_void_p * 2)(*[x.data_ptr() for x in t])
    rc = _lib.lib().gp_adam_step_multi(C.c_int32(2), arr(s["dc"], s["rest"]), arr(g_dc, g_rest), arr(s["m_dc"], s["m_rest"]),
                                       arr(s["v_dc"], s["v_rest"]), (C.c_int64 * 2)(s["dc"].numel(), s["rest"].numel()),
                                       (C.c_float * 2)(LR_DC, LR_REST), C.c_float(B1), C.c_float(B2), C.c_float(EPS), C.c_int64(step),
                                       C.c_int32(0), C.c_uint32(0), None, _lib.stream_ptr(s["dc"].device))
    _lib.check(rc, "gp_adam_step_multi")
    torch.cuda.synchronize()


def _payload(s, step, skip_flag=None):
    return dict(m_dc=s["m_dc"], v_dc=s["v_dc"], m_rest=s["m_rest"], v_rest=s["v_rest"], lr_dc=LR_DC, lr_rest=LR_REST, beta1=B1, beta2=B2,
                eps=EPS, step=step, skip_flag=skip_flag)


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 700])      # (a workgroup of the fused kernel: 64 Gaussians)
def test_fused_sh_adam_equals_the_gradient_path_and_the_library_step(n, degree):
    rs, fix, state, w = _scene(n, degree)
    exp = {k: v.clone() for k, v in state.items()}
    got = {k: v.clone() for k, v in state.items()}
    # the premise: two gradient-writing calls on the same inputs agree in every bit
    a, radii = _backward(rs, fix, exp["dc"], exp["rest"], w)
    b, _ = _backward(rs, fix, exp["dc"], exp["rest"], w)
    assert torch.equal(a["dc"], b["dc"]) and torch.equal(a["rest"], b["rest"]), "the backward is not deterministic at 8 x 8"
    # what the scene is there for
    vis = radii > 0
    assert int(vis.sum()) >= max(1, n // 2)
    assert float(a["dc"].abs().max()) > 0.0 and (degree == 0) == (float(a["rest"].abs().max()) == 0.0)
    used = 3 * ((degree + 1) ** 2 - 1)
    assert float(a["rest"].reshape(n, 45)[:, used:].abs().max() if used < 45 else 0.0) == 0.0
    if n >= 255:
        assert not bool(vis[0]) and not bool(vis[1])
        cl = a["dc"][2:12, 0]
        assert bool(vis[2:12].all()) and bool((cl == 0).any(dim=1).all()) and bool((cl != 0).any()), "no clamp flag set"
    for step in (5, 6, 7):      # three consecutive steps from one state
        e, _ = _backward(rs, fix, exp["dc"], exp["rest"], w)
        _library_adam(exp, e["dc"], e["rest"], step)
        g, _ = _backward(rs, fix, got["dc"], got["rest"], w, fuse=_payload(got, step))
        for k in state:
            assert torch.equal(got[k], exp[k]), (k, step, float((got[k] - exp[k]).abs().max()))
            assert bool(torch.isfinite(got[k]).all()), (k, step)
        for k in OTHER:
            assert torch.equal(g[k], e[k]), (k, step)
    assert not torch.equal(got["dc"], state["dc"]) and not torch.equal(got["rest"], state["rest"])
    assert not torch.equal(got["m_rest"], state["m_rest"]) and not torch.equal(got["v_rest"], state["v_rest"])


@pytest.mark.parametrize("n,degree", [(257, 0), (700, 3)])
def test_skip_flag_leaves_parameters_and_moments_untouched(n, degree):
    rs, fix, state, w = _scene(n, degree)
    got = {k: v.clone() for k, v in state.items()}
    flag = torch.ones(1, dtype=torch.int32, device="cuda")
    e, _ = _backward(rs, fix, state["dc"].clone(), state["rest"].clone(), w)
    g, _ = _backward(rs, fix, got["dc"], got["rest"], w, fuse=_payload(got, 5, flag))
    for k in state:
        assert torch.equal(got[k], state[k]), k
    for k in OTHER:
        assert torch.equal(g[k], e[k]), k
