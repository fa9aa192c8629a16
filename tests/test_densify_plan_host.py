"""No GPU: the one-function restatement of densify -> reset_opacity -> prune (tests/densify_ref.py) against the EXISTING methods of a
CPU GaussianModel, bit for bit (this pins what the device path of tests/test_gpu_densify_device.py is compared with to current
behaviour); include/gp_densify.h against the binding's table; the refusals that need no device."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import abi_check
import densify_ref as R
import gaussianprediction_amd as gpa
from gaussianprediction_amd import _lib, densify_ops as D
from gaussianprediction_amd.scene_synth import SceneSpec, make_gaussians
from gaussianprediction_amd.training import default_training_args

TH = dict(grad_threshold=0.0002, percent_dense=0.01, extent=5.0, min_opacity=0.005)


def _setup(n=40):
    from types import SimpleNamespace
    margs = SimpleNamespace(beta=0.1, d=4, w=256, feature_dim=32, second_stage_iteration=30000, third_stage_iteration=40000,
                            jointly_iteration=1000, nearest_num=6, norm_rotation=True, step_opacity=False, step_opacity_iteration=5000,
                            opacity_type="implicit", xyz_noise_iteration=0, max_points=8, adaptive_points_num=6)
    raw = make_gaussians(SceneSpec(n_gaussians=n, extent=(1.3, 1.3, 1.3), scale_lo=0.01, scale_hi=0.2, seed=5))
    pc = gpa.GaussianModel(3, margs)
    pc.set_inputDim(12, 60)
    pc.create_from_tensors(raw["xyz"], raw["features_dc"], raw["features_rest"], raw["scaling"], raw["rotation"], raw["opacity"],
                           raw["motion_feature"], None, None)
    pc.training_setup(default_training_args())
    return pc


def _fake_adam_state(pc, step=17):
    pc.optimizer.step_count = step
    for k, g in enumerate(pc.optimizer.param_groups):
        for p in g["params"]:
            m = torch.arange(p.numel(), dtype=torch.float32).reshape(p.shape) + 1000 * k
            pc.optimizer.load_full_moments(p, m.clone(), 2 * m + 1)


def _model():
    """40 rows: split sources, clone sources, transparent rows, rows large on screen and one large in the world; distinct moments."""
    pc = _setup()
    _fake_adam_state(pc)
    n = pc._xyz.shape[0]
    hot = torch.zeros(n, dtype=torch.bool); hot[[1, 4, 7, 20, 21, 33]] = True
    pc.denom += 1
    pc.denom[10] = 0                                        # never seen: mean gradient 0
    pc.xyz_gradient_accum[hot] = 1.0
    pc.xyz_gradient_accum_max[:] = torch.rand(n, 1, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        pc._scaling[:] = np.log(0.02)
        pc._opacity[:] = 2.0
        pc._opacity[30:34] = -10.0                          # transparent; 33 is a clone source whose clone goes too
        pc._scaling[[1, 4]] = np.log(0.2)                   # > percent_dense * extent: split
        pc._scaling[1, 1] = np.log(0.11)
        pc._scaling[5] = np.log(0.6)                        # > 0.1 * extent: the world-size test
    pc.max_radii2D[[0, 2, 3]] = 50.0
    return pc


def _snapshot(pc):
    per = pc._per_gaussian()
    mom = pc.adam_moments()
    state = {k: v.detach().clone() for k, v in per.items()}
    moments = {k: tuple(t.clone() for t in mom[id(p)]) for k, p in per.items() if id(p) in mom}
    stats = dict(accum=pc.xyz_gradient_accum.clone(), denom=pc.denom.clone(), accum_max=pc.xyz_gradient_accum_max.clone(),
                 max_radii2D=pc.max_radii2D.clone())
    return state, moments, stats


@pytest.mark.parametrize("case", ["densify+prune", "densify+reset+prune", "prune alone, live radii", "no screen size"])
def test_restatement_equals_the_existing_methods(case, monkeypatch):
    pc = _model()
    n = pc._xyz.shape[0]
    do_densify = case != "prune alone, live radii"
    do_reset = case == "densify+reset+prune"
    screen = None if case == "no screen size" else 20
    normals = torch.randn(2, n, 3, generator=torch.Generator().manual_seed(7))
    state, moments, stats = _snapshot(pc)
    want = R.densify_reset_prune(state, moments, stats, normals, max_screen_size=screen, do_densify=do_densify, do_reset=do_reset, **TH)
    # the existing path draws torch.normal(std=stds[sel]): give it the same draws, copy c of source i from normals[c, i]
    monkeypatch.setattr(torch, "normal", lambda mean, std, generator=None: normals[:, want.split].reshape(-1, 3) * std)
    n_clone = n_src = 0
    if do_densify:
        n_clone, n_src = pc.densify(TH["grad_threshold"], TH["min_opacity"], TH["extent"], screen)
    if do_reset:
        pc.reset_opacity()
    n_pruned = pc.prune(TH["grad_threshold"], TH["min_opacity"], TH["extent"], screen)
    assert (n_clone, n_src, n_pruned) == (want.n_clone, want.n_src, want.n_pruned)
    if do_densify:
        assert (n_clone, n_src) == (4, 2) and n_pruned == (6 if screen else 5)     # 30..33, the clone of 33 (+ the world-size row)
    else:
        assert n_pruned == 4 + 3 + 1
    got_state, got_mom, got_stats = _snapshot(pc)
    assert set(got_state) == set(want.state) and "motion_feature" in got_state and set(got_mom) == set(want.moments)
    for k in got_state:                 # copied fields, split xyz and scaling (the same torch ops) and the row order: the same bits
        assert torch.equal(got_state[k], want.state[k]), k
    for k in got_mom:
        assert torch.equal(got_mom[k][0], want.moments[k][0]) and torch.equal(got_mom[k][1], want.moments[k][1]), k
    for k in R.STATS:
        assert got_stats[k].shape == want.stats[k].shape and torch.equal(got_stats[k], want.stats[k]), k
    # the order the header promises: survivors in order, clones in source order, first copies, second copies
    seg, src = want.segment, want.source
    assert torch.equal(seg, seg.sort(stable=True).values)
    for j in range(4):
        s = src[seg == j]
        assert torch.equal(s, s.sort().values) and s.unique().numel() == s.numel()
    assert torch.equal(src[seg == 2], src[seg == 3])
    if not do_densify:
        assert float(want.stats["accum_max"].sum()) > 0          # compacted, not zeroed


# ---- one signature per entry point, two statements of it: include/gp_densify.h and densify_ops.PROTOTYPES ----
_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "float": C.c_float, "gp_stream_t": _lib.Ptr}
_POINTEES = {"float", "void", "int32_t", "uint32_t", "uint8_t", "gp_densify_tensor"}


def test_prototype_table_equals_the_header():
    abi_check.check_table(D.ABI, 5, _SCALARS, _POINTEES)
    assert D.ABI.prototypes is D.PROTOTYPES and D.ABI.header == "gp_densify.h"


def test_symbols_constants_and_the_table_entry_layout():
    hdr = abi_check.header_text("gp_densify.h")
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_DENSIFY_[A-Z0-9_]+) (\d+)u?\b", hdr)}
    assert defs["GP_DENSIFY_ABI_VERSION"] == D.GP_DENSIFY_ABI_VERSION == D.ABI.version == 1
    l = abi_check.check_applied(D.ABI)
    assert (defs["GP_DENSIFY_BLOCK"], defs["GP_DENSIFY_MAX_TENSORS"], defs["GP_DENSIFY_MAX_ROWS"]) == (D.BLOCK, D.MAX_TENSORS, D.MAX_ROWS)
    assert tuple(defs["GP_DENSIFY_" + k] for k in ("DENSIFY", "RESET", "PRUNE", "SCREEN")) == (D.DENSIFY, D.RESET, D.PRUNE, D.SCREEN)
    assert tuple(defs["GP_DENSIFY_ST_" + k] for k in ("CLONED", "SPLIT", "PRUNED", "ROWS", "BASE")) == \
        (D.ST_CLONED, D.ST_SPLIT, D.ST_PRUNED, D.ST_ROWS, D.ST_BASE) and defs["GP_DENSIFY_STATUS_WORDS"] == D.STATUS_WORDS == D.ST_BASE + 4
    assert {k: defs["GP_DENSIFY_ROLE_" + k.upper()] for k in D.ROLES} == D.ROLES and defs["GP_DENSIFY_ROLE_NONE"] == D.ROLE_NONE
    # gp_densify_tensor: six pointers, two int32, in the header's order
    body = re.search(r"typedef struct gp_densify_tensor \{(.*?)\}", hdr, flags=re.S).group(1)
    fields = [re.sub(r"^in$", "in_", f) for f in re.findall(r"(\w+);", body)]
    assert fields == [f[0] for f in D.DensifyTensorC._fields_] and C.sizeof(D.DensifyTensorC) == 6 * 8 + 2 * 4
    # the scratch query: keep bytes + six counts per block, every part rounded to 256 bytes; the row limits
    q = lambda n: int(l.gp_densify_scratch_bytes(n))        # noqa: E731
    assert q(1) == 512 and q(256 * 64 + 1) == (256 * 64 + 256) + (6 * 65 * 4 + 255) // 256 * 256
    assert q(0) == -1 and b"N = 0" in l.gp_last_error() and q(D.MAX_ROWS + 1) == -1 and q(D.MAX_ROWS) > 0


def test_refusals_need_no_gpu():
    l = D.lib()
    null = [None] * 5
    for bad in (0.0, -1e-4, float("nan")):       # the C entry refuses before it looks at a pointer
        assert l.gp_densify_plan(10, *null, bad, 0.05, 0.005, 20.0, 0.5, D.DENSIFY | D.PRUNE, None, None, None) == 1
        assert b"grad_threshold" in l.gp_last_error()
    assert l.gp_densify_plan(10, *null, 2e-4, 0.05, 0.005, 20.0, 0.5, D.DENSIFY, None, None, None) == 1 and b"null" in l.gp_last_error()
    assert l.gp_densify_plan(10, *null, 2e-4, 0.05, 0.005, 20.0, 0.5, 16, None, None, None) == 1 and b"flags" in l.gp_last_error()
    assert l.gp_densify_apply(10, 9, None, None, None, None, 10, 0, None, None, None) == 1 and b"num_tensors" in l.gp_last_error()
    assert l.gp_densify_stats(10, *([None] * 7), None) == 1 and b"null" in l.gp_last_error()
    n = 8
    z = lambda *s: torch.zeros(*s)               # noqa: E731
    with pytest.raises(ValueError, match="grad_threshold"):
        D.plan(z(n, 1), z(n, 1), z(n), z(n, 3), z(n, 1), 0.0, 0.05, 0.005, 20, 0.5, do_densify=True, do_reset=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.plan(z(n, 1), z(n, 1), z(n), z(n, 3), z(n, 1), 2e-4, 0.05, 0.005, 20, 0.5, do_densify=True, do_reset=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.stats(z(n).bool(), z(n).int(), z(n, 3), z(n), z(n, 1), z(n, 1), z(n, 1))
    # the model entry: a CPU model is refused and left as it was
    pc = _model()
    before = _snapshot(pc)
    from gaussianprediction_amd import densify as dn
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pc.densify_prune_device(2e-4, 0.005, 5.0, 20, True, False)
    vs = torch.zeros(n, 3, requires_grad=True)
    vs.grad = torch.ones(n, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dn.track_view_device(pc, {"viewspace_points": vs, "visibility_filter": z(n).bool(), "radii": z(n).int()})
    after = _snapshot(pc)
    assert all(torch.equal(before[0][k], after[0][k]) for k in before[0]) and all(torch.equal(before[2][k], after[2][k]) for k in R.STATS)
    assert pc._surgery_no == 0
