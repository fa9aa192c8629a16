"""No GPU: the numpy restatement tests/meanshift_ref.py against sklearn's recorded output (tests/golden/meanshift.npz) and against live
sklearn; csrc/gp_meanshift.h against the binding's table (a binding outside _lib.ABIS); the programs of csrc/meanshift_core.h in a
stand-alone build (tests/meanshift_emulate.cpp, under the sanitizers where the host compiler can link them), bit for bit against the
restatement; every refusal of the C entries and of the Python surface without a device."""
import ctypes as C
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import abi_check
import emulate_build
import meanshift_ref as ref
from gaussianprediction_amd import _lib, feature_vis as F, meanshift_ops as M

_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "gp_stream_t": _lib.Ptr}
_POINTEES = {"float", "double", "void", "int32_t"}
FIXTURE_CASES = ref.FIXTURE_RUNS
# The bar of the centres against sklearn: 3 x the largest |restatement - sklearn| measured when the fixture was recorded (8.58e-6, on
# coordinates up to about 25 in magnitude; the fixture's description and DESIGN section 23 state it), rounded up to one digit.
REF_TO_FIXTURE = 3e-5
BANDWIDTH_REL = 1e-6               # both sides average N float32 distances; measured: <= 9e-9
EMULATED = ("blobs_33_2_est", "blobs_33_2_fix", "blobs_257_3_est", "lines0_257_2_300", "lines0_257_2_3", "blobs_1031_8_fix", "lines1_1031_3_300",
            "lines2_1031_3_3", "edge1d_300_all", "edge1d_1_all", "edge1d_0_all")
CLUSTER_SIGNATURE = "(features, method='KMeans', k=4)"       # [REF utils/visualizer_utils.py:35]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def against_sklearn(r, centres, labels, n_iter):
    assert r["cluster_centers"].shape == centres.shape                                         # K
    assert np.array_equal(r["labels"], labels)                                                 # every label
    assert r["n_iter"] == int(n_iter)
    assert np.abs(r["cluster_centers"].astype(np.float64) - centres).max() <= REF_TO_FIXTURE


# ---- the restatement against sklearn ----
@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_restatement_against_the_recorded_sklearn_output(name):
    g = np.load(ref.GOLDEN)
    X, _, bw, _, _ = ref.cases()[name]
    xkey = "_".join(re.sub(r"^lines\d", "lines", name).split("_")[:3])
    assert same(X, g[f"X_{xkey}"]) and g[f"labels_{name}"].dtype == np.int16 and len(g[f"labels_{name}"]) == len(X)
    assert float(g["restatement_to_sklearn_centres"]) * 3 <= REF_TO_FIXTURE
    r = ref.run_case(name)
    against_sklearn(r, g[f"centers_{name}"], g[f"labels_{name}"], g[f"n_iter_{name}"])
    if bw is None:
        assert r["bandwidth"] == ref.estimate_bandwidth(X) and abs(r["bandwidth"] / float(g[f"estimate_{xkey}"]) - 1) <= BANDWIDTH_REL
        assert float(g[f"bandwidth_{name}"]) == float(g[f"estimate_{xkey}"])
    else:
        assert float(g[f"bandwidth_{name}"]) == float(bw)


def test_fixture_holds_arrays_and_its_versions():
    g = np.load(ref.GOLDEN, allow_pickle=False)
    assert str(g["sklearn_version"]) == "1.7.2" and str(g["numpy_version"]) and "restatement" in str(g["description"])
    assert os.path.getsize(ref.GOLDEN) < 1 << 20


@pytest.mark.parametrize("name", [n for n in ref.cases() if n not in FIXTURE_CASES])
def test_restatement_against_live_sklearn(name):
    cluster = pytest.importorskip("sklearn.cluster")
    X, seeds, bw, max_iter, cluster_all = ref.cases()[name]
    if bw is None:
        bw = float(cluster.estimate_bandwidth(X))
        assert abs(ref.estimate_bandwidth(X) / bw - 1) <= BANDWIDTH_REL
        bw = ref.estimate_bandwidth(X)
    ms = cluster.MeanShift(bandwidth=bw, seeds=seeds, max_iter=max_iter, cluster_all=cluster_all).fit(X)
    r = ref.mean_shift(X, bw, seeds, max_iter, cluster_all)
    against_sklearn(r, ms.cluster_centers_, ms.labels_, ms.n_iter_)
    if name.startswith("edge1d"):
        assert (r["seed_counts"] == 0).tolist() == [False] * 65 + [True]                        # the far seed is dropped
        assert int((r["labels"] < 0).sum()) == (0 if cluster_all else {300: 18, 1: 17, 0: 19}[max_iter])


def test_the_tables_of_the_cases():
    """K and n_iter of the blob and line cases, as sklearn 1.7.2 gave them."""
    want = {"blobs_33_2": ((2, 2), (7, 2)), "blobs_257_3": ((3, 3), (4, 2)), "blobs_1031_8": ((3, 4), (1, 2)), "blobs_2053_32": ((1, 5), (4, 1)),
            "blobs_777_64": ((3, 3), (2, 1)), "lines0_257_2": ((8, 10), (15, 3)), "lines1_1031_3": ((12, 16), (45, 3)),
            "lines2_1031_3": ((26, 33), (23, 3)), "lines3_2053_8": ((11, 15), (37, 3)), "lines4_1500_32": ((5, 6), (32, 3))}
    for stem, (K, n_iter) in want.items():
        a, b = (ref.run_case(f"{stem}_{v}") for v in (("est", "fix") if stem.startswith("blobs") else (300, 3)))
        assert (len(a["cluster_centers"]), len(b["cluster_centers"])) == K and (a["n_iter"], b["n_iter"]) == n_iter, stem
    r = ref.run_case("subset_2053_32")
    assert len(r["seed_counts"]) == 51 and len(r["cluster_centers"]) == 5


def test_restatement_lone_far_seed_and_estimates_against_live_sklearn():
    cluster = pytest.importorskip("sklearn.cluster")
    X, _ = ref.edge_1d()
    far = np.array([[100.0]], np.float32)
    with pytest.raises(ValueError, match="No point was within bandwidth"):
        ref.mean_shift(X, 0.8, far)
    with pytest.raises(ValueError, match="No point was within bandwidth"):
        cluster.MeanShift(bandwidth=0.8, seeds=far).fit(X)
    X = ref.cases()["blobs_1031_8_est"][0]
    for quantile, n_samples in ((0.3, None), (0.1, 300), (0.5, 64)):
        want = cluster.estimate_bandwidth(X, quantile=quantile, n_samples=n_samples, random_state=0)
        got = ref.estimate_bandwidth(X if n_samples is None else ref.subsample(X, n_samples), quantile)
        assert abs(got / want - 1) <= BANDWIDTH_REL, (quantile, n_samples)
    assert ref.estimate_bandwidth(X, 0.0005) == 0.0 and cluster.estimate_bandwidth(X, quantile=0.0005) == 0.0      # k clamped to 1
    assert M.check_bandwidth(0.0) == "bandwidth must be finite and > 0"


# ---- the header, the table, the registry ----
def test_prototype_table_equals_the_header_and_stays_out_of_the_registry():
    before = len(_lib.ABIS)
    protos = abi_check.check_table(M.ABI, 5, _SCALARS, _POINTEES)
    assert M.ABI.prototypes is M.PROTOTYPES and M.ABI not in _lib.ABIS and len(_lib.ABIS) == before
    assert os.path.samefile(os.path.join(abi_check.ROOT, "include", M.ABI.header),
                            os.path.join(abi_check.ROOT, "gaussianprediction_amd", "csrc", "gp_meanshift.h"))
    for name in ("gp_meanshift_bandwidth", "gp_meanshift_run", "gp_meanshift_merge"):
        assert protos[name][1][-1] == "gp_stream_t"              # the stream is the last parameter
    text = abi_check.header_text(M.HEADER)
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_MEANSHIFT_[A-Z0-9_]+) +(\d+)", text)}
    assert defs["GP_MEANSHIFT_ABI_VERSION"] == M.GP_MEANSHIFT_ABI_VERSION == M.ABI.version == 1
    assert (defs["GP_MEANSHIFT_MAX_D"], defs["GP_MEANSHIFT_MAX_CENTRES"], defs["GP_MEANSHIFT_MAX_ITER"], defs["GP_MEANSHIFT_STATUS_WORDS"]) == \
        (M.MAX_D, M.MAX_CENTRES, M.MAX_ITER, M.STATUS_WORDS) == (64, 4096, 10000, 8)
    from gaussianprediction_amd import kmeans_ops
    assert M.MAX_D == kmeans_ops.MAX_D and M.MAX_CENTRES == kmeans_ops.MAX_K                  # gp_kmeans_assign labels the rows
    assert [defs[f"GP_MEANSHIFT_ST_{w}"] for w in ("UNFINISHED", "KEPT", "EMPTY", "OVERFLOW", "N_ITER", "BAD_BANDWIDTH", "LIVE")] == \
        [M.ST_UNFINISHED, M.ST_KEPT, M.ST_EMPTY, M.ST_OVERFLOW, M.ST_N_ITER, M.ST_BAD_BANDWIDTH, M.ST_LIVE]
    full = open(os.path.join(abi_check.ROOT, "include", M.HEADER)).read()
    for word in ("Distance.", "Bandwidth", "Shift.", "Merge.", "Launches.", "duplicate", "-ffp-contract=off"):
        assert word in full, word
    assert '#include "../../include/gp_hip.h"' in full
    abi_check.check_applied(M.ABI)


# ---- the programs in a stand-alone build, under the sanitizers ----
@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    """run(mode, payload bytes) -> the output bytes."""
    d = tmp_path_factory.mktemp("meanshift_emulate")
    exe = emulate_build.build("meanshift_emulate", d, sanitize=True)

    def run(mode, payload):
        job, out = str(d / "job.bin"), str(d / "out.bin")
        with open(job, "wb") as fp:
            fp.write(struct.pack("<i", mode) + payload)
        subprocess.check_call([exe, job, out], timeout=600)
        return open(out, "rb").read()

    return run


@pytest.mark.parametrize("name", EMULATED)
def test_core_programs_equal_the_restatement_bit_for_bit(emulator, name):
    X, seeds, _, max_iter, _ = ref.cases()[name]
    r = ref.run_case(name)
    seeds = X if seeds is None else seeds
    N, D, S = len(X), X.shape[1], len(seeds)
    raw = emulator(0, struct.pack("<qqiid", N, S, D, max_iter, r["bandwidth"]) + X.tobytes() + seeds.tobytes())
    assert same(np.frombuffer(raw, np.float32, S * D).reshape(S, D), r["seed_centers"])
    assert np.array_equal(np.frombuffer(raw, np.int32, S, 4 * S * D), r["seed_counts"])
    assert np.array_equal(np.frombuffer(raw, np.int32, S, 4 * S * D + 4 * S), r["seed_iterations"])
    at = 4 * S * D + 8 * S
    K = struct.unpack_from("<i", raw, at)[0]
    assert K == len(r["cluster_centers"]) and len(raw) == at + 4 + 4 * K * D + 4 * K
    assert same(np.frombuffer(raw, np.float32, K * D, at + 4).reshape(K, D), r["cluster_centers"])        # the kept centres and their order
    assert np.array_equal(np.frombuffer(raw, np.int32, K, at + 4 + 4 * K * D), r["counts"])


@pytest.mark.parametrize("name,quantile", [("blobs_33_2_est", 0.3), ("blobs_257_3_est", 0.3), ("blobs_1031_8_est", 0.3), ("blobs_1031_8_est", 0.0005),
                                           ("blobs_257_3_est", 1.0), ("edge1d_300_all", 0.5)])
def test_kth_distances_equal_np_partition_exactly_and_the_bandwidth_the_restatement(emulator, name, quantile):
    X = ref.cases()[name][0]
    N, D = X.shape
    raw = emulator(1, struct.pack("<qid", N, D, quantile) + X.tobytes())
    assert len(raw) == 4 * N + 8
    assert same(np.frombuffer(raw, np.float32, N), ref.kth_distances(X, quantile))
    assert struct.unpack_from("<d", raw, 4 * N)[0] == ref.estimate_bandwidth(X, quantile)
    if name.endswith("est") and quantile == 0.3:
        assert ref.run_case(name)["bandwidth"] == ref.estimate_bandwidth(X)


def test_radius_threshold_is_the_largest_square_within_the_bandwidth(emulator):
    rng = np.random.default_rng(3)
    bw = np.concatenate([[0.8, 1.0, 1.5, 2.5, 8.0, 1e-30, 1e30, 3e38, 1e-45, 1.5 * np.sqrt(32)], 10.0 ** rng.uniform(-6, 6, 200)])
    raw = emulator(3, struct.pack("<i", len(bw)) + bw.astype(np.float64).tobytes())
    t, ok = np.frombuffer(raw, np.float32, len(bw)), np.frombuffer(raw, np.int32, len(bw), 4 * len(bw))
    assert ok.all()
    bwf = bw.astype(np.float32)
    with np.errstate(over="ignore"):
        assert (np.sqrt(t) <= bwf).all() and ((np.sqrt(np.nextafter(t, np.float32(np.inf))) > bwf) | (t == np.finfo(np.float32).max)).all()
    assert same(t, np.array([M.radius2(b) for b in bw], np.float32))
    raw = emulator(3, struct.pack("<i", 5) + np.array([0.0, -1.0, np.nan, np.inf, -np.inf]).tobytes())     # refused ones terminate
    assert not np.frombuffer(raw, np.int32, 5, 20).any()


# ---- the refusals, word for word ----
def test_refusals_word_for_word_against_the_python_checks(emulator):
    queries = [(0, (N, S, D), 0.0) for N, S, D in ((1, 1, 1), (5, 5, 0), (5, 5, 65), (5, 5, 64), (0, 5, 3), (2 ** 31, 5, 1), (2 ** 31 - 1, 1, 1),
                                                   (5, 0, 3), (5, 2 ** 31, 1), (2 ** 30, 5, 2), (5, 2 ** 30, 2), (2 ** 25 - 1, 7, 64), (-3, 5, 3))]
    queries += [(1, (a, 0, 0), 0.0) for a in (-1, 0, 300, 10000, 10001)]
    queries += [(2, (a, 0, 0), 0.0) for a in (0, 1, 64, 4096, 4097)]
    queries += [(3, (0, 0, 0), q) for q in (0.0, -0.1, 0.0005, 0.3, 1.0, 1.0001, float("nan"))]
    raw = emulator(2, struct.pack("<i", len(queries)) + b"".join(struct.pack("<iqqqd", kind, *a, q) for kind, a, q in queries))
    assert len(raw) == 96 * len(queries)
    accepted = 0
    for n, (kind, a, q) in enumerate(queries):
        text = raw[96 * n:96 * n + 96].split(b"\0")[0].decode()
        want = M.check_sizes(*a) if kind == 0 else M.check_max_iter(a[0]) if kind == 1 else M.check_rounds(a[0]) if kind == 2 else M.check_quantile(q)
        assert text == (want or ""), (kind, a, q)
        accepted += not text
    assert accepted == 4 + 3 + 3 + 3


def test_c_entries_refuse_without_a_device():
    """Null or dummy pointers are given: every refusal comes before any launch."""
    l = M.lib()
    err = lambda: l.gp_last_error().decode()
    assert l.gp_meanshift_scratch_size(5, 5, 65) == -1 and M.check_sizes(5, 5, 65) in err() and "gp_meanshift_scratch_size" in err()
    assert l.gp_meanshift_scratch_size(0, 5, 3) == -1 and M.check_sizes(0, 5, 3) in err()
    assert l.gp_meanshift_scratch_size(1, 1, 1) >= 256 and l.gp_meanshift_scratch_size(1000, 10, 3) >= 12 * 1000
    big = 1 << 40
    for N, D, q in ((0, 3, 0.3), (5, 65, 0.3), (2 ** 30, 2, 0.3)):
        assert l.gp_meanshift_bandwidth(8, N, D, q, 8, None, 256, big, None) == 1 and M.check_sizes(N, 1, D) in err()
    for q in (0.0, 1.5, float("nan")):
        assert l.gp_meanshift_bandwidth(8, 5, 3, q, 8, None, 256, big, None) == 1 and M.check_quantile(q) in err()
    assert l.gp_meanshift_bandwidth(None, 5, 3, 0.3, 8, None, 256, big, None) == 1 and "null" in err()
    assert l.gp_meanshift_bandwidth(8, 5, 3, 0.3, 8, None, None, big, None) == 1 and "null" in err()
    assert l.gp_meanshift_bandwidth(8, 5, 3, 0.3, 8, None, 256, 16, None) == 1 and "scratch holds" in err()
    assert l.gp_meanshift_bandwidth(8, 5, 3, 0.3, 8, None, 264, big, None) == 1 and "aligned" in err()
    run = lambda N, D, S, max_iter, X=8, scratch=256, nbytes=big: l.gp_meanshift_run(X, N, D, 8, S, 8, max_iter, 8, 8, 8, 8, scratch, nbytes, None)
    for N, S, D in ((5, 5, 0), (5, 5, 65), (0, 5, 3), (5, 0, 3), (2 ** 31, 5, 1), (5, 2 ** 30, 2)):
        assert run(N, D, S, 300) == 1 and M.check_sizes(N, S, D) in err() and "gp_meanshift_run" in err()
    for max_iter in (-1, 10001):
        assert run(5, 3, 5, max_iter) == 1 and M.check_max_iter(max_iter) in err()
    assert run(5, 3, 5, 300, X=None) == 1 and "null" in err()
    assert run(5, 3, 5, 300, nbytes=16) == 1 and "scratch holds" in err()
    assert run(5, 3, 5, 300, scratch=264) == 1 and "aligned" in err()
    merge = lambda S, D, rounds, C=8, scratch=256, nbytes=big: l.gp_meanshift_merge(C, 8, S, D, 8, 1, rounds, 8, 8, 8, scratch, nbytes, None)
    for S, D in ((0, 3), (5, 65), (2 ** 30, 2)):
        assert merge(S, D, 64) == 1 and M.check_sizes(1, S, D) in err()
    for rounds in (0, 4097):
        assert merge(5, 3, rounds) == 1 and M.check_rounds(rounds) in err()
    assert merge(5, 3, 64, C=None) == 1 and "null" in err()
    assert merge(5, 3, 64, nbytes=16) == 1 and "scratch holds" in err()
    assert merge(5, 3, 64, scratch=264) == 1 and "aligned" in err()


def test_the_python_surface_refuses_before_the_device(monkeypatch):
    from gaussianprediction_amd import eval_render as ER
    monkeypatch.setattr(M, "lib", lambda: pytest.fail("a launch was reached"))
    x = torch.zeros(10, 4)
    for call in (lambda: M.mean_shift(x), lambda: M.estimate_bandwidth(x), lambda: M.mean_shift(x, 1.0, seeds=x), lambda: F.cluster(x, "MeanShift"),
                 lambda: F.cluster(x), lambda: F.label_colors(torch.zeros(4, dtype=torch.int64)),
                 lambda: ER.render_segments("m", "test", 1, [], None, None, x, features=x),
                 lambda: ER.render_segments("m", "test", 1, [], None, None, x, labels=torch.zeros(4, dtype=torch.int64))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    # what a device tensor would be refused for, checked on a stand-in that only claims to be on the device
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    with pytest.raises(RuntimeError, match="must be float32"):
        M.mean_shift(x.double(), 1.0)
    with pytest.raises(RuntimeError, match="must be contiguous"):
        M.mean_shift(torch.zeros(4, 10).t(), 1.0)
    with pytest.raises(RuntimeError, match="2 dimension"):
        M.mean_shift(torch.zeros(10), 1.0)
    with pytest.raises(_lib.GpHipError, match=re.escape("D must be in 1 .. 64")):
        M.mean_shift(torch.zeros(10, 65), 1.0)
    with pytest.raises(_lib.GpHipError, match=re.escape("D must be in 1 .. 64")):
        M.estimate_bandwidth(torch.zeros(10, 65))
    with pytest.raises(_lib.GpHipError, match="quantile must be in"):
        M.estimate_bandwidth(x, quantile=0.0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.GpHipError, match="bandwidth must be finite and > 0"):
            M.mean_shift(x, bad)
    for bad in (-1, 10001):
        with pytest.raises(_lib.GpHipError, match=re.escape("max_iter must be in 0 .. 10000")):
            M.mean_shift(x, 1.0, max_iter=bad)
    with pytest.raises(RuntimeError, match="seeds"):
        M.mean_shift(x, 1.0, seeds=torch.zeros(3, 5))


def test_cluster_has_the_references_signature_and_a_stable_palette():
    assert str(inspect.signature(F.cluster)) == CLUSTER_SIGNATURE
    a, b = F.label_palette(3), F.label_palette(40)
    assert same(a, b[:3]) and a.dtype == np.float32 and a.min() >= 0.1 and b.max() <= 1.0 and len({r.tobytes() for r in b}) == 40
    assert not same(F.label_palette(3, seed=1), a)
