"""No GPU: csrc/gp_trajectory.h against the binding's table (a binding outside _lib.ABIS); the programs of csrc/trajectory_core.h in a
stand-alone build (tests/trajectory_emulate.cpp, under the sanitizers where the host compiler can link them) against the numpy
restatement tests/trajectory_ref.py on every case of tests/trajectory_cases.py, bit for bit; the closed form of the line against the
incremental one; the refusals that need no device; the projection against the reference's own functions (tests/golden)."""
import ctypes as C
import os
import re
import struct
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import abi_check
import emulate_build
import trajectory_cases as cases
import trajectory_ref as ref
from gaussianprediction_amd import _lib, trajectory_ops as T

_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "gp_stream_t": _lib.Ptr}
_POINTEES = {"float", "int32_t", "uint32_t"}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trajectory_projection.npz")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the header, the table, the registry ----
def test_prototype_table_equals_the_header_and_stays_out_of_the_registry():
    before = len(_lib.ABIS)
    protos = abi_check.check_table(T.ABI, 3, _SCALARS, _POINTEES, {"gp_traj_view": T.TrajViewC})
    assert T.ABI.prototypes is T.PROTOTYPES and T.ABI not in _lib.ABIS
    assert os.path.samefile(os.path.join(abi_check.ROOT, "include", T.ABI.header),
                            os.path.join(abi_check.ROOT, "gaussianprediction_amd", "csrc", "gp_trajectory.h"))
    for name in ("gp_traj_step", "gp_traj_resolve"):
        assert protos[name][1][-1] == "gp_stream_t"              # the stream is the last parameter
    extra = _lib.Abi(T.HEADER, "gp_traj_abi_version", T.GP_TRAJ_ABI_VERSION, T.PROTOTYPES, register=False)
    assert len(_lib.ABIS) == before and extra not in _lib.ABIS
    assert extra.lib() is _lib.lib()                              # ... and it still binds and checks the version, on the one handle


def test_symbols_constants_and_the_struct():
    text = abi_check.header_text(T.HEADER)
    defs = dict(re.findall(r"#define (GP_TRAJ_[A-Z0-9_]+) +(\(?-?\d+[^\n/]*?)\s*(?:/\*|\n)", text))
    assert int(defs["GP_TRAJ_ABI_VERSION"]) == T.GP_TRAJ_ABI_VERSION == T.ABI.version == 1
    assert eval(defs["GP_TRAJ_NOT_DRAWABLE"]) == T.NOT_DRAWABLE == ref.NOT_DRAWABLE == -2 ** 31
    assert int(defs["GP_TRAJ_COORD_LIMIT"]) == T.COORD_LIMIT == int(ref.LIMIT) == 2 ** 20
    abi_check.check_applied(T.ABI)
    fields = re.search(r"typedef struct gp_traj_view \{(.*?)\}", text, flags=re.S).group(1)
    assert re.findall(r"(\w+)(?:\[(\d+)\])?\s*[,;]", fields) == [("R", "9"), ("t", "3"), ("f", ""), ("cx", ""), ("cy", "")]
    assert [n for n, _ in T.TrajViewC._fields_] == ["R", "t", "f", "cx", "cy"] and C.sizeof(T.TrajViewC) == 60


def test_view_constants_are_the_restatements():
    for rotated in (False, True):
        view = cases.camera(rotated)
        c, want = T.view_constants(view, cases.H, cases.W), ref.constants(view, cases.H, cases.W)
        assert same(np.array(c.R[:], np.float32), want.R.reshape(9)) and same(np.array(c.t[:], np.float32), want.t)
        assert same(np.array([c.f, c.cx, c.cy], np.float32), np.array([want.f, want.cx, want.cy]))
    a, b = T.default_colors(7, seed=3), T.default_colors(7, seed=3)
    assert a.shape == (7, 3) and a.dtype == torch.float32 and torch.equal(a, b) and not torch.equal(a, T.default_colors(7, seed=4))


# ---- the closed form of the line ----
def closed_form(a, b):
    """The pixels of the header's definition: k = 0 .. dm, minor = a_minor + sn * floor((2 k dn + dm - 1) / (2 dm))."""
    dx, dy = b[0] - a[0], b[1] - a[1]
    xmajor = abs(dx) >= abs(dy)
    dm, dn = (abs(dx), abs(dy)) if xmajor else (abs(dy), abs(dx))
    sign = lambda v: -1 if v < 0 else 1                                                 # noqa: E731
    sm, sn = (sign(dx), sign(dy)) if xmajor else (sign(dy), sign(dx))
    if dm == 0:
        return [tuple(a)]
    out = []
    for k in range(dm + 1):
        major, minor = (a[0] if xmajor else a[1]) + sm * k, (a[1] if xmajor else a[0]) + sn * ((2 * k * dn + dm - 1) // (2 * dm))
        out.append((major, minor) if xmajor else (minor, major))
    return out


def test_closed_form_equals_the_incremental_line():
    for dm in range(0, 65):
        for dn in range(0, dm + 1):
            for dx, dy in ((dm, dn), (dn, dm), (-dm, dn), (dn, -dm), (-dm, -dn), (-dn, -dm), (dm, -dn), (-dn, dm)):
                a, b = (3, -2), (3 + dx, -2 + dy)
                got = list(ref.line(a, b))
                assert got == closed_form(a, b), (a, b)
                assert got[0] == a and got[-1] == b and len(got) == max(dm, 1) + (dm > 0)
                assert all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) == 1 for p, q in zip(got, got[1:]))      # 8-connected


# ---- the programs in a stand-alone build, under the sanitizers ----
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    """run(case fields) -> (px per step, owner, image), or the refusal's code."""
    d = tmp_path_factory.mktemp("trajectory_emulate")
    exe = emulate_build.build("trajectory_emulate", d, sanitize=True)

    def run(view, H, W, steps, idx, P, min_depth, colors, base):
        job, out = str(d / "job.bin"), str(d / "out.bin")
        c = ref.constants(view, H, W)
        N, S = len(steps[0]), len(steps)
        with open(job, "wb") as fp:
            fp.write(struct.pack("<iiqqqiif", H, W, N, P, S, int(idx is not None), int(base is not None), float("nan") if min_depth is None else min_depth))
            fp.write(np.concatenate([c.R.reshape(9), c.t, [c.f, c.cx, c.cy]]).astype(np.float32).tobytes())
            for a in ([] if idx is None else [idx.astype(np.int32)]) + [colors.astype(np.float32)] + ([] if base is None else [base]) + list(steps):
                fp.write(np.ascontiguousarray(a).tobytes())
        subprocess.check_call([exe, job, out], timeout=120)
        raw = open(out, "rb").read()
        if struct.unpack("<i", raw[:4])[0]:
            return 1
        pxs = [np.frombuffer(raw, np.int32, P * 2, 4 + s * P * 8).reshape(P, 2) for s in range(S)]
        off = 4 + S * P * 8
        owner = np.frombuffer(raw, np.uint32, H * W, off).reshape(H, W)
        image = np.frombuffer(raw, np.float32, 3 * H * W, off + 4 * H * W).reshape(3, H, W)
        assert len(raw) == off + 16 * H * W
        return pxs, owner, image

    return run


@pytest.mark.parametrize("name", list(cases.CASES))
def test_emulated_programs_against_the_restatement(emulator, name):
    c = cases.CASES[name]
    want_px, want_owner, want_plain, want_over = cases.reference(name)
    for base, want_image in ((None, want_plain), (c.base, want_over)):
        pxs, owner, image = emulator(c.view, c.H, c.W, c.steps, c.idx, c.P, c.min_depth, c.colors, base)
        assert len(pxs) == len(want_px) and all(same(g, w) for g, w in zip(pxs, want_px))
        assert same(owner, want_owner) and same(image, want_image)
    touched = want_owner != 0
    assert touched.any() == (c.P > 0 and len(c.steps) > 1)
    assert same(want_over[:, ~touched], c.base[:, ~touched]) and (want_over[:, touched] <= 1.0).all()


def test_the_cases_reach_what_they_are_for():
    owner = {n: cases.reference(n)[1] for n in cases.CASES}
    px = {n: cases.reference(n)[0] for n in cases.CASES}
    P = cases.CASES["identical_paths"].P
    assert set(np.unique((owner["identical_paths"][owner["identical_paths"] != 0] - 1) % P)) == {P - 1}        # the highest j owns
    over = owner["later_step_overdraws"]
    assert over[22, 33] == 2 * 2 + 0 + 1 and over[22, 20] == 1 * 2 + 1 + 1            # step 2 of point 0 over step 1 of point 1
    assert (px["coordinate_limit"][1][:2] != ref.NOT_DRAWABLE).all() and (px["coordinate_limit"][1][2:] == ref.NOT_DRAWABLE).all()
    assert (owner["coordinate_limit"] != 0).sum() > 60
    clip = owner["clip_from_far_outside"]
    assert set(np.unique(clip)) >= {2 * 12 + j + 1 for j in range(8)} and not {12 + 9, 12 + 12, 24 + 9, 24 + 12} & set(np.unique(clip))
    assert (owner["behind_the_camera"] != 0).sum() > (owner["behind_the_camera_min_depth"] != 0).sum() > 0
    assert (px["idx_with_duplicates"][0][58:] == ref.NOT_DRAWABLE).all() and same(px["idx_with_duplicates"][2][:10], px["idx_with_duplicates"][2][10:20])


# ---- the refusals that need no device ----
def test_refusals_before_any_pointer_is_looked_at():
    l, view = T.lib(), T.view_constants(cases.camera(True), 45, 67)

    def step(xyz=8, idx=None, N=10, P=10, s=1, px=8, owner=8, H=45, W=67, v=view):
        return l.gp_traj_step(None if v is None else C.byref(v), xyz, idx, N, P, s, px, owner, H, W, float("nan"), None)

    for kw, word in ((dict(H=0), b"H and W"), (dict(W=-3), b"H and W"), (dict(H=2 ** 16, W=2 ** 15), b"H*W"), (dict(N=-1), b">= 0"), (dict(P=-1), b">= 0"),
                     (dict(s=-1), b">= 0"), (dict(P=2 ** 31, N=2 ** 31), b"P must be below"), (dict(N=9), b"at least P rows"),
                     (dict(idx=8, N=0), b"holds no row"), (dict(P=2 ** 20, N=2 ** 20, s=4095), b"2^32 - 1"), (dict(P=65537, N=65537, s=65534), b"2^32 - 1"),
                     (dict(P=1, N=1, s=2 ** 32 - 2), b"2^32 - 1"), (dict(xyz=None), b"null"), (dict(px=None), b"null"), (dict(owner=None), b"null"),
                     (dict(v=None), b"null")):
        assert step(**kw) == 1 and word in l.gp_last_error(), kw          # (nothing was launched: the pointers are not even memory)
        if b"null" not in word:
            a = dict(N=10, P=10, s=1, H=45, W=67)
            a.update({k: v for k, v in kw.items() if k in a})
            assert T.check_sizes(has_idx="idx" in kw, **a).encode() in l.gp_last_error()
    assert T.check_sizes(2 ** 20, 2 ** 20, 4094, 45, 67, False) is None and T.check_sizes(1, 1, 2 ** 32 - 3, 45, 67, False) is None      # S*P = 2^32 - 2
    assert step(P=0, N=0, xyz=None, px=None) == 0                          # no points: nothing to launch, nothing to refuse
    for kw, word in ((dict(H=0), b"H and W"), (dict(P=-1), b">= 0"), (dict(owner=None), b"null"), (dict(out=None), b"null"), (dict(colors=None), b"null")):
        a = dict(owner=8, colors=8, P=5, base=None, out=8, H=45, W=67)
        a.update(kw)
        assert l.gp_traj_resolve(a["owner"], a["colors"], a["P"], a["base"], a["out"], a["H"], a["W"], None) == 1 and word in l.gp_last_error(), kw


def test_the_python_surface_refuses_before_the_device(monkeypatch):
    from gaussianprediction_amd import eval_render as ER
    monkeypatch.setattr(T, "lib", lambda: pytest.fail("a launch was reached"))
    view = cases.camera(True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.TrajectoryCanvas(view, 5, "cpu")
    with pytest.raises(_lib.GpHipError, match="H and W must be > 0"):
        T.TrajectoryCanvas(view, 5, "cuda", H=0)
    with pytest.raises(_lib.GpHipError, match="P must be below"):
        T.TrajectoryCanvas(view, 2 ** 31, "cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ER.keypoint_trails(view, torch.zeros(3, 4, 3))
    with pytest.raises(RuntimeError, match=r"\[S, K, 3\]"):
        ER.keypoint_trails(view, torch.zeros(3, 4))
    g = SimpleNamespace(forward=lambda *a: pytest.fail("the model was evaluated"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ER.project_trajectory(g, view, torch.zeros(45, 67, dtype=torch.int32), 6, 1)
    with pytest.raises(RuntimeError, match="steps"):
        ER.project_trajectory(g, view, torch.zeros(45, 67, dtype=torch.int32), 6, 1, steps=0)


# ---- the projection against the reference's own functions ----
def test_projection_against_the_references_functions(emulator):
    g = np.load(GOLDEN)
    xyz, left_out = g["xyz"], 0
    for k in range(len(g["R"])):
        W, H = (int(v) for v in g["sizes"][k])
        view = SimpleNamespace(R=g["R"][k], T=g["T"][k], FoVx=float(g["FoVx"][k]))
        uv, want = g["uv"][k], g["pixels"][k]
        keep = (np.abs(uv - np.round(uv)) > 1e-3).all(axis=-1)           # (torch.bmm's summation order is not the definition's)
        left_out += int((~keep).sum())
        ours = ref.project(ref.constants(view, H, W), xyz)
        pxs, _, _ = emulator(view, H, W, [xyz], None, len(xyz), None, np.zeros((len(xyz), 3), np.float32), None)
        assert same(pxs[0], ours)                                          # the core's projection is the restatement's, on every point
        assert (ours != ref.NOT_DRAWABLE).all() and np.array_equal(ours[keep], want[keep]), k
        u, v, _ = ref.uv(ref.constants(view, H, W), xyz)
        assert np.abs(np.stack([u, v], axis=-1) - uv).max() <= 2e-3 * max(1.0, np.abs(uv).max() / 1024)      # (a few ulps at the largest coordinate)
    assert left_out <= 0.01 * g["uv"].shape[0] * g["uv"].shape[1], left_out
