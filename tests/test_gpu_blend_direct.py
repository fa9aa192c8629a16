"""-m gpu: the keypoint blend on its own, through the C ABI (gp_blend_forward / gp_blend_backward with _lib.BlendArgsC), so that each
case picks the kernel itself -- knn_idx16 set or NULL, tensors aligned or not, dL_draw_w set or NULL, nearest_num, out_dim,
norm_rotation -- against tests/blend_ref.py (float64, gather form).  Every case id names the kernels the dispatch of
csrc/gp_capi_deform.hip reaches (kernels_reached restates its choice) and the regime: `nb` workgroups of the backward (at most 1024;
beyond 262 144 Gaussians a workgroup takes a second chunk), which decides the loops of gp_blend_bwd_reduce_kernel (16-wide from
nb > 240, 4-wide from nb > 48, tail).

Per case:
  * per-element bounds |got - want| <= RTOL * A + ATOL (blend_ref: A = magnitude sums) on xyz_t, q_t, g_delta, g_raw_w, g_rot;
    RTOL = 4 * 2.14e-7: four times the worst err / A of a float32 torch restatement over the inputs of every case here at CPU
    scale (2.13e-7, g_delta; test_blend_ref_host.py measures it on every run).  Worst err / A of the kernels on the MI355X over
    all 97 cases: xyz_t 2.57e-7, q_t 1.79e-7, g_delta 2.66e-7, g_raw_w 2.38e-7, g_rot 2.74e-7 (each case prints its own with -s)
  * the bars of test_gpu_deform.test_blend_forward_backward as a second, whole-tensor assertion
  * g_delta[:, 7:od] exactly zero, g_xyz bit-equal to the incoming gradient
  * every output is a view into a NaN-filled buffer with 64 guard floats on either side and is NaN itself before the call: after
    it the guards are NaN, the outputs are not
  * the same call again gives the same bits (no atomics on floats), and int64 indices give the bits of the packed 16-bit ones"""
import ctypes as C

import numpy as np
import pytest
import torch

import blend_ref as BR
from blend_ref import spec
from util import rel_l2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64


def _lib():
    from gaussianprediction_amd import _lib as m
    return m


def kernels_reached(nn, i16, al_fwd, al_bwd):
    """the launches of gp_blend_forward / gp_blend_backward_impl by name."""
    if nn in (6, 8):
        f = f"fwd{nn}{'_i16' if i16 else ''}" if al_fwd else f"fwd[{'knn16' if i16 else 'i64'}]"
        b = f"bwd{nn}{'_i16' if i16 else ''}" if al_bwd else f"bwd[{'knn16' if i16 else 'i64'}]"
    else:
        f, b = (f"fwd[{'knn16' if i16 else 'i64'}]", f"bwd[{'knn16' if i16 else 'i64'}]") if nn else ("fwd[stage1]", "bwd[stage1]")
    return f"{f}+{b}"


# ------------------------------------------------------------------------------------------------
# inputs and references, built once per spec (the last two are kept: cases that share a spec are neighbours)
# ------------------------------------------------------------------------------------------------
_cache = {}


def inputs_and_reference(sp):
    if sp not in _cache:
        while len(_cache) >= 2:
            _cache.pop(next(iter(_cache)))
        inp = BR.make_inputs(sp)
        _cache[sp] = (inp, BR.blend_reference(inp))
    return _cache[sp]


def guarded(shape, shift=0):
    """(buffer, view): the view is NaN like the GUARD (+ shift) floats in front of it and the GUARD behind it."""
    n = int(np.prod(shape))
    buf = torch.full((GUARD + shift + n + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    return buf, buf[GUARD + shift:GUARD + shift + n].view(*shape)


def read_guarded(buf, view, name, written=True):
    h = buf.cpu().numpy()
    n, lo = view.numel(), (view.data_ptr() - buf.data_ptr()) // 4
    assert np.isnan(h[:lo]).all() and np.isnan(h[lo + n:]).all(), f"{name}: guard words around the output were overwritten"
    out = h[lo:lo + n].reshape(tuple(view.shape))
    if written:
        assert not np.isnan(out).any(), f"{name}: {int(np.isnan(out).sum())} output elements were not written (or are NaN)"
    else:
        assert np.isnan(out).all(), f"{name}: written although the call was refused"
    return out


def shifted(t, elems):
    """a copy of t on the device whose address is `elems` elements past an aligned one."""
    flat = torch.empty(t.numel() + elems, dtype=t.dtype, device=DEV)
    v = flat[elems:].view(*t.shape)
    v.copy_(t)
    return v


class Variant(tuple):
    """(i16, mis_raw, mis_idx, mis_graw, graw_null): knn_idx16 set; raw_w 4 bytes, knn_idx 8 bytes, dL_draw_w 4 bytes off 16-byte
    alignment; dL_draw_w NULL."""
    __slots__ = ()
    i16, mis_raw, mis_idx, mis_graw, graw_null = (property(lambda s, i=i: s[i]) for i in range(5))


def variant(i16, mis_raw=False, mis_idx=False, mis_graw=False, graw_null=False):
    return Variant((bool(i16), bool(mis_raw), bool(mis_idx), bool(mis_graw), bool(graw_null)))


def reached(sp, v):
    return kernels_reached(sp.nn, v.i16, not (v.mis_raw or v.mis_idx), not (v.mis_raw or v.mis_idx or (v.mis_graw and not v.graw_null)))


def blend_args(inp, v, K=None, nn=None, od=None, idx16_shift=0):
    """(BlendArgsC, tensors kept alive)."""
    m = _lib()
    nn_ = inp["nn"] if nn is None else nn
    dev = lambda t: t.to(DEV).contiguous()
    keep = {"delta": dev(inp["delta"]), "xyz": dev(inp["xyz"]), "rot": dev(inp["rot"])}
    if inp["nn"]:
        BR.check_indices(inp["idx"].numpy(), inp["K"])
        keep["raw_w"] = shifted(inp["raw_w"], 1) if v.mis_raw else dev(inp["raw_w"])
        keep["idx"] = shifted(inp["idx"], 1) if v.mis_idx else dev(inp["idx"])
        if v.i16:
            assert inp["K"] <= 65535
            keep["idx16"] = shifted(inp["idx"].to(torch.int32).to(torch.int16), idx16_shift)
        assert (keep["raw_w"].data_ptr() % 16 == 4) == v.mis_raw and (keep["idx"].data_ptr() % 16 == 8) == v.mis_idx
        assert keep["raw_w"].data_ptr() % 16 in (0, 4) and keep["idx"].data_ptr() % 16 in (0, 8)
    p = lambda k: keep[k].data_ptr() if k in keep else None
    args = m.BlendArgsC(inp["xyz"].shape[0], inp["K"] if K is None else K, nn_, inp["od"] if od is None else od, int(inp["norm"]),
                        p("delta"), p("raw_w"), p("idx"), p("xyz"), p("rot"), p("idx16"))
    return args, keep


def run_blend(inp, v, expect_bwd_refused=False, K=None):
    """forward and backward once; dict of numpy outputs, guards checked."""
    m = _lib()
    N, nn, od = inp["xyz"].shape[0], inp["nn"], inp["od"]
    rows = inp["delta"].shape[0]
    args, keep = blend_args(inp, v, K=K)
    gx, gq = inp["gx"].to(DEV), inp["gq"].to(DEV)
    bufs = {"xyz_t": guarded((N, 3)), "q_t": guarded((N, 4)), "g_delta": guarded((rows, od)), "g_xyz": guarded((N, 3)),
            "g_rot": guarded((N, 4))}
    if nn:
        bufs["g_raw_w"] = guarded((N, 2 * nn), shift=1 if v.mis_graw else 0)
        assert bufs["g_raw_w"][1].data_ptr() % 16 == (4 if v.mis_graw else 0)
    dev = torch.device(DEV)
    out = {}
    if not expect_bwd_refused:
        m.check(m.lib().gp_blend_forward(args, bufs["xyz_t"][1], bufs["q_t"][1], m.stream_ptr(dev)), "gp_blend_forward")
    with m.TorchAllocator(dev) as alloc:
        rc = m.lib().gp_blend_backward(args, gx, gq, bufs["g_delta"][1], None if (v.graw_null or not nn) else bufs["g_raw_w"][1],
                                       bufs["g_xyz"][1], bufs["g_rot"][1], alloc.cb, None, m.stream_ptr(dev))
    torch.cuda.synchronize()
    if expect_bwd_refused:
        assert rc != 0
        out["error"] = m.lib().gp_last_error().decode(errors="replace")
    else:
        m.check(rc, "gp_blend_backward")
    for k, (buf, view) in bufs.items():
        written = not expect_bwd_refused and not (k == "g_raw_w" and v.graw_null)
        out[k] = read_guarded(buf, view, k, written=written)
    del keep
    return out


_worst = {}


def assert_matches_reference(got, ref, inp, skip_delta_rows=()):
    nn, od = inp["nn"], inp["od"]
    names = [k for k in BR.COMPARED if k in got and k in ref and not np.isnan(got[k]).all()]
    ratios = {}
    for k in names:
        g, w, A = got[k], ref[k], ref["A_" + k]
        if k == "g_delta" and len(skip_delta_rows):
            keep = np.ones(g.shape[0], dtype=bool)
            keep[list(skip_delta_rows)] = False
            assert np.isfinite(g).all()
            g, w, A = g[keep], w[keep], A[keep]
        ratios[k] = BR.worst_ratio(g, w, A)
        _worst[k] = max(_worst.get(k, 0.0), ratios[k])
    print("blend err/A: " + "  ".join(f"{k} {r:.3g}" for k, r in ratios.items()) + "   | worst so far: "
          + "  ".join(f"{k} {r:.3g}" for k, r in _worst.items()))
    for k in names:
        g, w, A = got[k], ref[k], ref["A_" + k]
        if k == "g_delta" and len(skip_delta_rows):
            g, w, A = g[keep], w[keep], A[keep]
        bad = np.abs(g.astype(np.float64) - w) > BR.RTOL * A + BR.ATOL
        if bad.any():
            at = tuple(int(i) for i in np.argwhere(bad)[0])
            raise AssertionError(f"{k}: {int(bad.sum())} elements beyond RTOL * A + ATOL, worst err / A {ratios[k]:.3g}; first at {at}: "
                                 f"got {g[at]!r}, want {w[at]!r}, A {A[at]!r}")
    # the whole-tensor bars of test_gpu_deform.test_blend_forward_backward
    assert np.abs(got["xyz_t"] - ref["xyz_t"]).max(initial=0.0) < 1e-5
    assert np.abs(got["q_t"] - ref["q_t"]).max(initial=0.0) < 1e-5
    if not len(skip_delta_rows):
        assert rel_l2(got["g_delta"][:, :7], ref["g_delta"][:, :7]) < 1e-4
    assert rel_l2(got["g_rot"], ref["g_rot"]) < 1e-4
    if "g_raw_w" in names:
        assert rel_l2(got["g_raw_w"], ref["g_raw_w"]) < 1e-4
    assert np.array_equal(got["g_xyz"].view(np.uint32), inp["gx"].numpy().view(np.uint32)), "g_xyz is not the incoming gradient bit for bit"
    assert not got["g_delta"][:, 7:od].any(), "g_delta[:, 7:od] is not zero"


def assert_same_bits(a, b, what, names=None):
    for k in names or a:
        if k in a and k in b and isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), f"{k}: {what}"


def check_case(sp, v, twin=None, skip_delta_rows=()):
    """one case: run twice (same bits), compare with the reference; `twin`: a second variant that must give the same bits."""
    inp, ref = inputs_and_reference(sp)
    got = run_blend(inp, v)
    assert_same_bits(got, run_blend(inp, v), "the same call twice gave different bits")
    assert_matches_reference(got, ref, inp, skip_delta_rows)
    if twin is not None:
        assert_same_bits(got, run_blend(inp, twin), "differs from its twin variant")
    return got


def N_of(nblocks):
    return BR.CHUNK * nblocks - 3


N_CAPPED = BR.CHUNK * BR.MAX_BLOCKS + 77      # 1025 chunks on 1024 workgroups: workgroup 0 takes a second, ragged one
SIZES = (N_of(1), N_of(65), N_CAPPED)


def _id(sp, v, extra=""):
    nb = BR.bwd_blocks(sp.N, sp.nn)
    loops = "r16" if nb > 240 else "r4" if nb > 48 else "rtail"
    two = "-2chunks" if sp.nn and sp.N > BR.CHUNK * BR.MAX_BLOCKS else ""
    mis = "".join(t for t, f in (("-misraw", v.mis_raw), ("-misidx", v.mis_idx), ("-misgraw", v.mis_graw), ("-nograw", v.graw_null)) if f)
    return (f"{reached(sp, v)}-nn{sp.nn}-K{sp.K}-od{sp.od}-norm{int(sp.norm)}-{sp.pattern}{'-' + sp.values if sp.values != 'normal' else ''}"
            f"-N{sp.N}-nb{nb}-{loops if sp.nn else 'noreduce'}{two}{mis}{extra}")


def _params(cases):
    return [pytest.param(*c, id=_id(c[0], c[1])) for c in cases]


# ------------------------------------------------------------------------------------------------
# variants x {1, 65, capped} workgroups
# ------------------------------------------------------------------------------------------------
def _variant_cases():
    cases = []
    for N in SIZES:
        # misaligned: one tensor at a time -- raw_w at nb 1, knn_idx at nb 65, dL_draw_w (forward stays on the fixed kernel) at the cap
        mis = {SIZES[0]: dict(mis_raw=True), SIZES[1]: dict(mis_idx=True), SIZES[2]: dict(mis_graw=True)}[N]
        for nn, od, norm in ((6, 8, True), (8, 7, False)):
            sp = spec("uniform", N, 300, nn, od, norm)
            cases += [(sp, variant(True), None), (sp, variant(False), variant(True)),        # int64: the bits of i16
                      (sp, variant(True, **mis), None), (sp, variant(False, **mis), None)]
        cases += [(spec("uniform", N, 300, 1, 7, True), variant(False), None), (spec("uniform", N, 300, 3, 8, False), variant(True), None),
                  (spec("uniform", N, 300, 5, 8, True), variant(True), None), (spec("uniform", N, 240, 16, 7, True), variant(False), None)]
        cases += [(spec("stage1", N, 0, 0, od, norm), variant(False), None) for od in (7, 8) for norm in (True, False)]
    return cases


VARIANT_CASES = _variant_cases()


@pytest.mark.parametrize("sp,v,twin", _params(VARIANT_CASES))
def test_variant(sp, v, twin):
    check_case(sp, v, twin)


NOGRAW_CASES = [(spec("uniform", N_of(65), 300, 6, 8, True), variant(True, graw_null=True), variant(True)),
                (spec("uniform", N_of(65), 300, 5, 8, True), variant(True, graw_null=True), variant(True))]


@pytest.mark.parametrize("sp,v,full", _params(NOGRAW_CASES))
def test_frozen_weights_leave_the_other_outputs_bit_identical(sp, v, full):
    inp, ref = inputs_and_reference(sp)
    got = run_blend(inp, v)
    assert np.isnan(got["g_raw_w"]).all()             # (read_guarded: the buffer that was not passed stayed NaN)
    assert_matches_reference(got, ref, inp)
    assert_same_bits(got, run_blend(inp, full), "changes when dL_draw_w is passed", names=("xyz_t", "q_t", "g_delta", "g_xyz", "g_rot"))


# ------------------------------------------------------------------------------------------------
# grid and reduce sweep on the shipped path
# ------------------------------------------------------------------------------------------------
GRID_N = [N_of(nb) for nb in (1, 16, 17, 49, 64, 65, 240, 241, 256, 257, 300)] + [262144, 262145, 256 * 1500 + 77]
GRID_CASES = [(spec("uniform", N, 300, 6, 8, True), variant(True), None) for N in GRID_N]


@pytest.mark.parametrize("sp,v,twin", _params(GRID_CASES))
def test_grid_and_reduce_sweep(sp, v, twin):
    check_case(sp, v, twin)


# ------------------------------------------------------------------------------------------------
# list regimes
# ------------------------------------------------------------------------------------------------
N_LISTS = 3 * BR.CHUNK - 59                      # two full chunks and a ragged one
N_COH_UNI = (BR.MAX_BLOCKS + 2) * BR.CHUNK       # chunks 0 .. 1025: workgroups 0 and 1 take two each


def _list_cases():
    cases = []
    for nn, K, od, norm, v, twin in ((6, 300, 8, True, variant(True), None), (8, 300, 7, True, variant(False), variant(True)),
                                     (16, 240, 8, True, variant(True), None)):
        cases += [(spec(p, N_LISTS, K, nn, od, norm), v, twin) for p in ("uniform", "coherent", "threshold", "hot")]
        cases += [(spec("perm", N_LISTS, nn, nn, od, norm), v, twin), (spec("coh_uni", N_COH_UNI, K, nn, od, norm), v, twin)]
    return cases


LIST_CASES = _list_cases()


@pytest.mark.parametrize("sp,v,twin", _params(LIST_CASES))
def test_list_regime(sp, v, twin):
    check_case(sp, v, twin)


# ------------------------------------------------------------------------------------------------
# K edges, the LDS limit, refusals
# ------------------------------------------------------------------------------------------------
K_EDGE_CASES = [(spec("uniform", N_of(3), K, 6, 8, True), variant(True), None) for K in (255, 256, 257, 512)]      # (K = nn: 'perm' above)
MAX_K_SHAPES = ((6, 7), (8, 8), (16, 8))


@pytest.mark.parametrize("sp,v,twin", _params(K_EDGE_CASES))
def test_k_edge(sp, v, twin):
    check_case(sp, v, twin)


@pytest.mark.parametrize("nn,od", MAX_K_SHAPES, ids=[f"nn{nn}-od{od}-K{BR.max_keypoints(nn, od)}" for nn, od in MAX_K_SHAPES])
def test_largest_accepted_k(nn, od):
    K = BR.max_keypoints(nn, od)
    assert BR.bwd_lds_bytes(K, nn, od) <= 65536 < BR.bwd_lds_bytes(K + 1, nn, od)
    check_case(spec("uniform", N_of(3), K, nn, od, True), variant(nn != 16), variant(False) if nn != 16 else None)


@pytest.mark.parametrize("nn,od", MAX_K_SHAPES, ids=[f"nn{nn}-od{od}-K{BR.max_keypoints(nn, od) + 1}" for nn, od in MAX_K_SHAPES])
def test_one_keypoint_more_is_refused_and_nothing_written(nn, od):
    sp = spec("uniform", N_of(3), BR.max_keypoints(nn, od) + 1, nn, od, True)
    out = run_blend(BR.make_inputs(sp), variant(True), expect_bwd_refused=True)
    assert "LDS" in out["error"], out["error"]


def test_make_blend_refusals_launch_nothing():
    m = _lib()
    sp = spec("uniform", N_of(1), 300, 6, 8, True)
    inp = BR.make_inputs(sp)
    dev = torch.device(DEV)

    def refused(expect, **kw):
        args, keep = blend_args(inp, variant(True), **kw)
        bufs = {k: guarded(s) for k, s in (("xyz_t", (sp.N, 3)), ("q_t", (sp.N, 4)), ("g_delta", (sp.K, 9)), ("g_raw_w", (sp.N, 2 * 17)),
                                          ("g_xyz", (sp.N, 3)), ("g_rot", (sp.N, 4)))}
        assert m.lib().gp_blend_forward(args, bufs["xyz_t"][1], bufs["q_t"][1], m.stream_ptr(dev)) != 0
        err = m.lib().gp_last_error().decode(errors="replace")
        assert expect in err, err
        with m.TorchAllocator(dev) as alloc:
            rc = m.lib().gp_blend_backward(args, inp["gx"].to(DEV), inp["gq"].to(DEV), bufs["g_delta"][1], bufs["g_raw_w"][1], bufs["g_xyz"][1],
                                           bufs["g_rot"][1], alloc.cb, None, m.stream_ptr(dev))
            assert rc != 0 and not alloc.bufs[m.GP_BUF_TEMP], "refused, but scratch was asked for"
        assert expect in m.lib().gp_last_error().decode(errors="replace")
        torch.cuda.synchronize()
        for k, (buf, view) in bufs.items():
            read_guarded(buf, view, k, written=False)

    K_fwd = 60000 // 28 + 1            # make_blend: K * 7 * 4 > 60000 (the count alone is refused: no row beyond inp's K is read)
    assert K_fwd * 28 > 60000 >= (K_fwd - 1) * 28
    refused("too many keypoints", K=K_fwd)
    refused("out_dim", od=6)
    refused("out_dim", od=9)
    refused("nearest_num", nn=17)
    args, keep = blend_args(inp, variant(True), idx16_shift=1)
    assert keep["idx16"].data_ptr() % 4 == 2
    refused("knn_idx16", idx16_shift=1)


# ------------------------------------------------------------------------------------------------
# values
# ------------------------------------------------------------------------------------------------
VALUE_CASES = [(spec("uniform", N_of(3), 300, 6, 8, True, "big60"), variant(True), None),
               (spec("uniform", N_of(3), 300, 5, 8, True, "big60"), variant(False), None)]


@pytest.mark.parametrize("sp,v,twin", _params(VALUE_CASES))
def test_weights_of_magnitude_60(sp, v, twin):
    inp, _ = inputs_and_reference(sp)
    assert float(inp["raw_w"].abs().max()) == 60.0
    check_case(sp, v, twin)


ZERO_QUAT_SPEC = spec("uniform", N_of(3), 300, 6, 8, True, "zeroquat")


def test_keypoint_with_a_zero_quaternion():
    """F.normalize of a zero quaternion is zero (eps 1e-12): the forward is defined and compared; that keypoint's gradient goes
    through 1 / eps and is only required to be finite.  Everything else is compared as usual."""
    inp, ref = inputs_and_reference(ZERO_QUAT_SPEC)
    kz = inp["meta"]["zero_kp"]
    assert not inp["delta"][kz, 3:7].any() and (inp["idx"] == kz).any()
    got = check_case(ZERO_QUAT_SPEC, variant(True), skip_delta_rows=(kz,))
    assert np.isfinite(got["g_delta"][kz]).all()


def test_no_gaussians():
    m = _lib()
    sp = spec("uniform", N_of(1), 300, 6, 8, True)
    inp = BR.make_inputs(sp)
    args, keep = blend_args(inp, variant(True))
    args.num_gaussians = 0
    dev = torch.device(DEV)
    bufs = {k: guarded(s) for k, s in (("xyz_t", (sp.N, 3)), ("q_t", (sp.N, 4)), ("g_delta", (sp.K, 8)), ("g_raw_w", (sp.N, 12)),
                                      ("g_xyz", (sp.N, 3)), ("g_rot", (sp.N, 4)))}
    assert m.lib().gp_blend_forward(args, bufs["xyz_t"][1], bufs["q_t"][1], m.stream_ptr(dev)) == 0
    with m.TorchAllocator(dev) as alloc:
        assert m.lib().gp_blend_backward(args, inp["gx"].to(DEV), inp["gq"].to(DEV), bufs["g_delta"][1], bufs["g_raw_w"][1], bufs["g_xyz"][1],
                                         bufs["g_rot"][1], alloc.cb, None, m.stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        read_guarded(buf, view, k, written=False)


# every input spec of this file, for tests/test_blend_ref_host.py (pattern promises, float32 restatement, teeth check at CPU scale)
ALL_SPECS = sorted({c[0] for c in VARIANT_CASES + NOGRAW_CASES + GRID_CASES + LIST_CASES + K_EDGE_CASES + VALUE_CASES}
                   | {ZERO_QUAT_SPEC} | {spec("uniform", N_of(3), BR.max_keypoints(nn, od), nn, od, True) for nn, od in MAX_K_SHAPES})
