"""No GPU: the float64 restatement tests/pca_ref.py against sklearn's recorded output (tests/golden/pca_vis.npz) and against live
sklearn; csrc/gp_pca.h against the binding's table (a binding outside _lib.ABIS); the jet table against matplotlib's; and the programs of
csrc/pca_core.h in a stand-alone build (tests/pca_emulate.cpp, under the sanitizers where the host compiler can link them): the Jacobi
residual contract, order and sign against the restatement, the projection bit for bit, the radix select against np.partition exactly,
the refusals word for word against the Python checks, the colour and table-index rules."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import abi_check
import emulate_build
import pca_ref as ref
from gaussianprediction_amd import _lib, feature_vis as F

_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "gp_stream_t": _lib.Ptr}
_POINTEES = {"float", "double", "void"}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pca_vis.npz")
FIXTURE_CASES = ((33, 32, 3), (257, 32, 3), (4099, 32, 3), (4099, 32, 5))
REF_TO_FIXTURE = 2.3e-5        # the bound the fixture's description states for the restatement alone (1.9e-6 measured)
EDGE_VALUES = np.array([-0.1, 0, 0.5, 0.999, 1.0, 1.1, np.nan], np.float32)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def fixture_samples(g, N, dim):
    f, x = g[f"features_{N}"], g[f"xyz_{N}"]
    return f if dim == 3 else np.concatenate([x, f], axis=-1)


# ---- the restatement against sklearn ----
@pytest.mark.parametrize("case", FIXTURE_CASES)
def test_restatement_against_the_recorded_sklearn_output(case):
    N, D, dim = case
    g = np.load(GOLDEN)
    tag = f"{N}_{D}_{dim}"
    r = ref.pca_vis(fixture_samples(g, N, dim), dim)
    assert g[f"colors_{tag}"].dtype == np.float32 and g[f"colors_{tag}"].shape == (N, 3)
    assert np.abs(r["colors"] - g[f"colors_{tag}"]).max() <= REF_TO_FIXTURE
    assert np.abs(r["components"] - g[f"components_{tag}"]).max() <= 1e-5            # (the same sign on every component)
    assert np.abs(np.array([r["q1"], r["q99"]]) - g[f"q_{tag}"]).max() <= 1e-4 * np.abs(g[f"q_{tag}"]).max()
    if dim == 5:
        assert np.abs(r["positions"] - g[f"positions_{tag}"]).max() <= REF_TO_FIXTURE and (g[f"positions_{tag}"][:, 2] == 1).all()
    else:
        assert same(g[f"positions_{tag}"], g[f"xyz_{N}"])
    if dim == 3:
        assert 0.005 < (g[f"colors_{tag}"] == 0).mean() < 0.02 and 0.005 < (g[f"colors_{tag}"] == 1).mean() < 0.02      # the clipped tails


def test_restatement_against_live_sklearn():
    PCA = pytest.importorskip("sklearn.decomposition").PCA
    for N, D, dim, seed in ((33, 8, 3, 1), (257, 61, 5, 2), (4099, 32, 3, 3)):
        X = ref.generate(N, D, seed)
        pca = PCA(dim, random_state=42)
        transformed = pca.fit_transform(X)
        q1, q99 = np.percentile(transformed, [1, 99])
        vis = ((X - X.mean(0)[None, :]) @ pca.components_.T - q1) / (q99 - q1)
        r = ref.pca_vis(X, dim)
        got = np.concatenate([r["positions"][:, :2], r["colors"]], axis=-1) if dim == 5 else r["colors"]
        want = np.concatenate([vis[:, :2], vis[:, 2:].clip(0, 1)], axis=-1) if dim == 5 else vis.clip(0, 1)
        assert np.abs(got - want).max() <= 3.2e-5, (N, D, dim)
        assert np.abs(r["components"] - pca.components_).max() <= 1e-5 and np.abs(r["explained_variance"] / pca.explained_variance_ - 1).max() <= 1e-5


def test_sign_rule_takes_the_first_of_equal_magnitudes():
    c = ref.sign_rule(np.array([[0.5, -0.5, 0.1], [-0.5, 0.5, 0.1], [0.1, -0.7, 0.7], [0.0, 0.0, 0.0]]))
    assert c.tolist() == [[0.5, -0.5, 0.1], [0.5, -0.5, -0.1], [-0.1, 0.7, -0.7], [0.0, 0.0, 0.0]]


# ---- the header, the table, the registry ----
def test_prototype_table_equals_the_header_and_stays_out_of_the_registry():
    before = len(_lib.ABIS)
    protos = abi_check.check_table(F.ABI, 7, _SCALARS, _POINTEES)
    assert F.ABI.prototypes is F.PROTOTYPES and F.ABI not in _lib.ABIS and len(_lib.ABIS) == before
    assert os.path.samefile(os.path.join(abi_check.ROOT, "include", F.ABI.header),
                            os.path.join(abi_check.ROOT, "gaussianprediction_amd", "csrc", "gp_pca.h"))
    for name in ("gp_pca_fit", "gp_pca_project", "gp_pca_percentiles", "gp_pca_colorize", "gp_colormap_lut"):
        assert protos[name][1][-1] == "gp_stream_t"              # the stream is the last parameter
    text = abi_check.header_text(F.HEADER)
    defs = dict(re.findall(r"#define (GP_PCA_[A-Z0-9_]+) +(\d+)", text))
    assert int(defs["GP_PCA_ABI_VERSION"]) == F.GP_PCA_ABI_VERSION == F.ABI.version == 1
    assert (int(defs["GP_PCA_MAX_D"]), int(defs["GP_PCA_MAX_DIM"]), int(defs["GP_PCA_MAX_Q"]), int(defs["GP_PCA_CHUNK_ROWS"])) == \
        (F.MAX_D, F.MAX_DIM, F.MAX_Q, F.CHUNK_ROWS) == (128, 8, 2, 1024)
    abi_check.check_applied(F.ABI)


# ---- the jet table ----
def test_jet_table_against_matplotlib_and_the_index_rule():
    table = F.jet_table()
    assert table.shape == (256, 3) and table.dtype == np.float32 and table.min() == 0 and table.max() == 1
    assert same(table[0], np.array([0, 0, 0.5], np.float32)) and same(table[255], np.array([0.5, 0, 0], np.float32))
    assert ref.lut_index(EDGE_VALUES).tolist() == [0, 0, 128, 255, 255, 255, -1]
    mpl = pytest.importorskip("matplotlib")
    cmap = mpl.colormaps["jet"]
    want = cmap(np.arange(256))[:, :3]
    assert np.abs(table.astype(np.float64) - want).max() <= 6e-8
    rgba = cmap(EDGE_VALUES)
    idx = ref.lut_index(EDGE_VALUES)
    ours = np.where(idx[:, None] < 0, 0.0, table[np.clip(idx, 0, 255)])
    assert np.abs(ours - rgba[:, :3]).max() <= 6e-8 and rgba[-1].tolist() == [0, 0, 0, 0]


# ---- the programs in a stand-alone build, under the sanitizers ----
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    """run(mode, payload bytes) -> the output bytes."""
    d = tmp_path_factory.mktemp("pca_emulate")
    exe = emulate_build.build("pca_emulate", d, sanitize=True)

    def run(mode, payload):
        job, out = str(d / "job.bin"), str(d / "out.bin")
        with open(job, "wb") as fp:
            fp.write(struct.pack("<i", mode) + payload)
        subprocess.check_call([exe, job, out], timeout=300)
        return open(out, "rb").read()

    return run


def jacobi(emulator, Cm, dim):
    D = len(Cm)
    raw = emulator(0, struct.pack("<ii", D, dim) + np.ascontiguousarray(Cm, dtype=np.float64).tobytes())
    sweeps = struct.unpack_from("<i", raw)[0]
    lam = np.frombuffer(raw, np.float64, D, 4)
    V = np.frombuffer(raw, np.float64, D * D, 4 + 8 * D).reshape(D, D).T          # (the program keeps the eigenvectors in rows)
    picks = [struct.unpack_from("<id", raw, 4 + 8 * D + 8 * D * D + 12 * k) for k in range(dim)]
    assert len(raw) == 4 + 8 * D + 8 * D * D + 12 * dim
    return sweeps, lam, V, picks


@pytest.mark.parametrize("N,D", [(5, 3), (33, 8), (257, 32), (300, 61), (400, 128), (6, 32), (50, 1), (50, 2)])
def test_jacobi_meets_the_residual_contract_and_the_restatements_order_and_sign(emulator, N, D):
    X = ref.generate(N, D, 7 * D + N).astype(np.float64)
    d = X - X.mean(0)
    Cm = d.T @ d / (N - 1)
    dim = min(8, D, N)
    sweeps, lam, V, picks = jacobi(emulator, Cm, dim)
    assert 1 <= sweeps < 30
    fro = np.linalg.norm(Cm)
    assert np.linalg.norm(Cm @ V - V * lam[None, :], axis=0).max() <= 1e-12 * fro              # every pair, not only the returned ones
    assert np.abs(V.T @ V - np.eye(D)).max() <= 1e-13
    _, want_c, want_l, all_l = ref.fit(X, dim)
    cols = [c for c, _ in picks]
    assert np.array_equal(lam[cols], np.sort(lam)[::-1][:dim]) and len(set(cols)) == dim     # descending, and the dim largest
    assert np.abs(lam[cols] - want_l).max() <= 1e-12 * fro
    gaps = -np.diff(all_l[:dim + 1]) if D > dim else np.array([1.0])
    for k, (c, s) in enumerate(picks):
        v = s * V[:, c]
        assert s in (1.0, -1.0) and v[np.argmax(np.abs(v))] > 0
        if D > dim and gaps[k:k + 1].min() > 1e-3 * all_l[0] and (k == 0 or gaps[k - 1] > 1e-3 * all_l[0]):
            assert np.abs(v - want_c[k]).max() <= 1e-9, (k, np.abs(v - want_c[k]).max())


def test_jacobi_on_equal_eigenvalues_zero_and_non_finite_matrices(emulator):
    sweeps, lam, V, picks = jacobi(emulator, np.eye(4) * 2.5, 3)              # nothing to rotate: the lower column first, sign +
    assert sweeps == 1 and same(V, np.eye(4)) and picks == [(0, 1.0), (1, 1.0), (2, 1.0)]
    sweeps, lam, V, picks = jacobi(emulator, np.zeros((5, 5)), 2)
    assert sweeps == 1 and not lam.any() and picks == [(0, 1.0), (1, 1.0)]
    sweeps, lam, V, picks = jacobi(emulator, np.diag([1.0, 3.0, 2.0]) * -1 + 0, 3)
    assert [c for c, _ in picks] == [0, 2, 1]
    for bad in (np.nan, np.inf):                                                # terminates; the results are unspecified
        Cm = np.eye(6)
        Cm[1, 2] = Cm[2, 1] = bad
        assert 1 <= jacobi(emulator, Cm, 3)[0] <= 30
    v = np.array([[0.5, -0.5], [-0.5, 0.5]])                                   # eigenvector (1, -1) / sqrt 2 of magnitudes equal: the first entry decides
    _, lam, V, picks = jacobi(emulator, v, 1)
    c, s = picks[0]
    assert abs(lam[c] - 1.0) <= 1e-15 and abs(V[0, c]) == abs(V[1, c]) and (s * V[:, c])[0] > 0 and (s * V[:, c])[1] < 0


@pytest.mark.parametrize("N,D,dim", [(5, 3, 3), (33, 8, 5), (257, 61, 3), (100, 128, 8), (64, 32, 1)])
def test_projection_equals_a_separately_written_float32_loop(emulator, N, D, dim):
    rng = np.random.default_rng(N + D)
    X, mean, comp = ref.generate(N, D, N), rng.normal(size=D).astype(np.float32), rng.normal(size=(dim, D)).astype(np.float32)
    raw = emulator(1, struct.pack("<qii", N, D, dim) + X.tobytes() + mean.tobytes() + comp.tobytes())
    assert same(np.frombuffer(raw, np.float32).reshape(N, dim), ref.project32(X, mean, comp))


def select(emulator, values, qs):
    values = np.ascontiguousarray(values, dtype=np.float32)
    raw = emulator(2, struct.pack("<qidd", len(values), len(qs), *(list(qs) + [0.0])[:2]) + values.tobytes())
    if struct.unpack_from("<i", raw)[0]:
        return None
    nq = len(qs)
    return np.frombuffer(raw, np.float32, 2 * nq, 4).reshape(nq, 2), np.frombuffer(raw, np.float32, nq, 4 + 8 * nq)


def select_cases():
    rng = np.random.default_rng(5)
    inf = np.inf
    return {
        "M = 1": ([3.25], [1, 99]),
        "all equal": (np.full(1000, -2.5), [1, 99]),
        "two distinct": (rng.permutation(np.r_[np.full(40, 1.5), np.full(61, -7.0)]), [1, 99]),
        "signed zeros": (rng.permutation(np.r_[np.full(50, -0.0), np.full(50, 0.0)]), [49.5, 50.5]),
        "infinities": (rng.permutation(np.r_[np.full(3, -inf), rng.normal(size=200), np.full(3, inf)]), [1, 99]),
        "all infinities": (np.r_[np.full(5, -inf), np.full(5, inf)], [0, 100]),
        "lo == hi": (rng.normal(size=101), [1, 99]),
        "one percentile": (rng.normal(size=777), [37.5]),
        "ends": (rng.normal(size=4099 * 3).astype(np.float32) * 1e-3, [0, 100]),
        "wide range": (rng.normal(size=5000) * 10.0 ** rng.integers(-30, 30, size=5000), [1, 99]),
        "denormals": (rng.integers(-50, 50, size=300).astype(np.float32) * np.float32(1e-45), [1, 99]),
    }


@pytest.mark.parametrize("name", list(select_cases()))
def test_radix_select_equals_np_partition_exactly(emulator, name):
    values, qs = select_cases()[name]
    values = np.asarray(values, dtype=np.float32)
    selected, out = select(emulator, values, qs)
    want = ref.order_statistics(values, qs)
    assert selected.dtype == want.dtype and np.array_equal(selected, want), name
    if name == "signed zeros":                                              # (np.partition does not tell -0 from +0; the total order does)
        assert np.signbit(selected).tolist() == [[True, False], [True, False]]
    else:
        assert same(selected, want), name
    if name == "lo == hi":
        assert (selected[:, 0] == selected[:, 1]).all()
    with np.errstate(invalid="ignore"):
        want_q = np.array([ref.interpolate(lo, hi, q, len(values)) for (lo, hi), q in zip(want, qs)], np.float32)
    assert out.dtype == want_q.dtype and np.array_equal(out, want_q, equal_nan=True)
    if np.isfinite(values).all():
        assert np.allclose(out, np.percentile(values.astype(np.float64), qs), rtol=1e-6, atol=1e-37)


def test_float_keys_keep_the_total_order(emulator):
    values = np.array([-np.inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 2.0, np.inf], np.float32)
    seen = set()
    for k in range(len(values)):
        q = 100.0 * k / (len(values) - 1)
        selected, _ = select(emulator, values[::-1], [q])
        assert np.array_equal(selected, ref.order_statistics(values[::-1].copy(), [q])), k
        seen |= {v.tobytes() for v in selected[0]}
    assert seen == {v.tobytes() for v in values}                              # every value, the two zeros apart


# ---- the refusals, word for word ----
def test_refusals_word_for_word_against_the_python_checks(emulator):
    queries = [(0, (N, D, dim), (0, 0)) for N, D, dim in ((1, 4, 1), (2, 0, 1), (2, 129, 1), (10, 128, 8), (10, 4, 5), (10, 9, 9), (3, 8, 4), (5, 3, 3),
                                                         (2 ** 31, 8, 1), (2 ** 28, 8, 8), (2 ** 28 - 1, 8, 8), (2, 1, 0), (-5, 3, 3))]
    queries += [(1, (M, nq, 0), q) for M, nq, q in ((0, 2, (1, 99)), (2 ** 31, 2, (1, 99)), (2 ** 31 - 1, 2, (1, 99)), (5, 0, (1, 99)), (5, 3, (1, 99)),
                                                    (5, 2, (-1, 99)), (5, 2, (1, 100.5)), (5, 1, (float("nan"), 0)), (5, 2, (0, 100)))]
    queries += [(2, (N, dim, 0), (0, 0)) for N, dim in ((0, 3), (5, 4), (5, 5), (5, 3), (2 ** 31 // 5 + 1, 5), (2 ** 31 // 3, 3), (2 ** 31 // 3 + 1, 3))]
    payload = struct.pack("<i", len(queries)) + b"".join(struct.pack("<iqqqdd", kind, *a, *q) for kind, a, q in queries)
    raw = emulator(3, payload)
    assert len(raw) == 96 * len(queries)
    accepted = 0
    for n, (kind, a, q) in enumerate(queries):
        text = raw[96 * n:96 * n + 96].split(b"\0")[0].decode()
        want = F.check_fit(*a) if kind == 0 else F.check_percentiles(a[0], list(q)[:a[1]] if a[1] <= 2 else [1, 2, 3]) if kind == 1 else F.check_colorize(*a[:2])
        assert text == (want or ""), (kind, a, q)
        accepted += not text
    assert 6 <= accepted <= 10


def test_the_library_words_its_refusals_the_same_way_before_any_pointer_is_looked_at():
    l = F.lib()
    assert l.gp_pca_scratch_size(1, 4) == -1 and F.check_fit(1, 4, 1).encode() in l.gp_last_error()
    assert l.gp_pca_scratch_size(5, 129) == -1 and F.check_fit(5, 129, 1).encode() in l.gp_last_error()
    assert l.gp_pca_scratch_size(2, 1) >= 16 * 1024 and l.gp_pca_scratch_size(10 ** 6, 32) >= 256 * 32 * 32 * 8
    for N, D, dim in ((1, 4, 1), (10, 129, 3), (10, 4, 5), (3, 8, 4), (2 ** 28, 8, 8)):
        assert l.gp_pca_fit(8, N, D, dim, 8, 8, 8, 256, 1 << 40, None) == 1 and F.check_fit(N, D, dim).encode() in l.gp_last_error()
    assert l.gp_pca_fit(8, 10, 4, 3, 8, 8, 8, 256, 16, None) == 1 and b"scratch holds" in l.gp_last_error()
    assert l.gp_pca_fit(8, 10, 4, 3, 8, 8, 8, 264, 1 << 40, None) == 1 and b"aligned" in l.gp_last_error()
    assert l.gp_pca_fit(None, 10, 4, 3, 8, 8, 8, 256, 1 << 40, None) == 1 and b"null" in l.gp_last_error()
    assert l.gp_pca_project(8, 0, 4, 8, 8, 3, 8, None) == 1 and b"N must be >= 1" in l.gp_last_error()
    assert l.gp_pca_project(8, 5, 4, 8, 8, 5, 8, None) == 1 and F.check_fit(8, 4, 5).encode() in l.gp_last_error()
    qs = (C.c_double * 2)(1.0, 101.0)
    assert l.gp_pca_percentiles(8, 5, qs, 2, 8, None, 256, 1 << 20, None) == 1 and F.check_percentiles(5, [1.0, 101.0]).encode() in l.gp_last_error()
    assert l.gp_pca_percentiles(8, 0, qs, 1, 8, None, 256, 1 << 20, None) == 1 and F.check_percentiles(0, [1.0]).encode() in l.gp_last_error()
    assert l.gp_pca_colorize(8, 5, 4, 8, None, 8, None) == 1 and F.check_colorize(5, 4).encode() in l.gp_last_error()
    assert l.gp_pca_colorize(8, 5, 5, 8, None, 8, None) == 1 and b"null" in l.gp_last_error()
    assert l.gp_colormap_lut(8, -1, 8, 8, None) == 1 and l.gp_colormap_lut(None, 0, None, None, None) == 0


def test_the_python_surface_refuses_before_the_device(monkeypatch):
    from gaussianprediction_amd import eval_render as ER
    monkeypatch.setattr(F, "lib", lambda: pytest.fail("a launch was reached"))
    x = torch.zeros(10, 4)
    for call in (lambda: F.pca_fit(x), lambda: F.percentiles(x, [1, 99]), lambda: F.colormap(x), lambda: F.PCA_vis(x[:, :3].contiguous(), x, return_only=True),
                 lambda: F.jet_lut("cpu"), lambda: F.draw_motion_feature(x[:, :3].contiguous(), x), lambda: F.draw_weights(x, x, x, 0),
                 lambda: ER.render_features("m", "test", 1, [], None, None, x, features=x)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(RuntimeError, match="must be 3 or 5"):
        F.PCA_vis(x, x, dim=4)


# ---- the colour rules ----
def test_colour_and_table_index_rules(emulator):
    x = np.r_[EDGE_VALUES, np.array([np.inf, -np.inf, 255 / 256, np.nextafter(np.float32(1), np.float32(0)), 1 / 256, -0.0], np.float32)].astype(np.float32)
    for q1, q99 in ((-0.25, 0.75), (0.5, 0.5)):                                 # q99 == q1: the IEEE result, no special case
        raw = emulator(4, struct.pack("<iff", len(x), q1, q99) + x.tobytes())
        n = len(x)
        vis, clipped, index = np.frombuffer(raw, np.float32, n), np.frombuffer(raw, np.float32, n, 4 * n), np.frombuffer(raw, np.int32, n, 8 * n)
        with np.errstate(all="ignore"):
            want = (x - np.float32(q1)) / (np.float32(q99) - np.float32(q1))
            assert same(vis, want) and same(clipped, np.clip(want, np.float32(0), np.float32(1)))
        assert index.tolist() == ref.lut_index(x).tolist() and index.tolist()[:7] == [0, 0, 128, 255, 255, 255, -1]
