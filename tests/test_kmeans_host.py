"""No GPU: include/gp_kmeans.h against the binding's table; the refusals that need no device; the kmeans_pytorch / torch_scatter
shims against the calls the reference makes (tests/golden/kmeans_surface.json); the float64 restatement (tests/kmeans_ref.py) against
training.kmeans; the cap on the rows that `ambiguous_rows` leaves out of an id comparison."""
import ctypes as C
import importlib
import inspect
import json
import os
import re

import pytest
import torch

import abi_check
import kmeans_ref as R
from gaussianprediction_amd import _lib, kmeans_ops as KM
from gaussianprediction_amd.training import kmeans as training_kmeans

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SURFACE = json.load(open(os.path.join(HERE, "golden", "kmeans_surface.json")))
SHIMS = ["kmeans_pytorch", "torch_scatter"]

# ---- one signature per entry point, two statements of it: include/gp_kmeans.h and kmeans_ops.PROTOTYPES ----
_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "float": C.c_float, "double": C.c_double,
            "gp_stream_t": _lib.Ptr}
_POINTEES = {"float", "void", "int32_t", "uint32_t"}


def test_prototype_table_equals_the_header():
    protos = abi_check.check_table(KM.ABI, 5, _SCALARS, _POINTEES)
    assert KM.ABI.prototypes is KM.PROTOTYPES and KM.ABI.header == "gp_kmeans.h"
    for name, (_, params) in protos.items():
        assert params == [] or params[-1] == "gp_stream_t" or name == "gp_kmeans_scratch_bytes", name      # the stream is the last parameter


def test_symbols_and_constants():
    defs = {k: int(v) for k, v in re.findall(r"#define (GP_KMEANS_[A-Z0-9_]+) (\d+)u?\b", abi_check.header_text("gp_kmeans.h"))}
    assert defs["GP_KMEANS_ABI_VERSION"] == KM.GP_KMEANS_ABI_VERSION == KM.ABI.version == 1
    abi_check.check_applied(KM.ABI)
    assert (defs["GP_KMEANS_BLOCK"], defs["GP_KMEANS_MAX_D"], defs["GP_KMEANS_MAX_K"], defs["GP_KMEANS_MAX_ROWS"], defs["GP_KMEANS_MAX_ITERS"]) == \
        (KM.BLOCK, KM.MAX_D, KM.MAX_K, KM.MAX_ROWS, KM.MAX_ITERS) == (256, 64, 4096, 2 ** 31 - 1, 1000)
    assert (defs["GP_KMEANS_STATUS_WORDS"], defs["GP_KMEANS_ST_ITERATIONS"], defs["GP_KMEANS_ST_CONVERGED"], defs["GP_KMEANS_ST_SHIFT2"]) == \
        (KM.STATUS_WORDS, KM.ST_ITERATIONS, KM.ST_CONVERGED, KM.ST_SHIFT2)
    assert KM.ST_SHIFT2 % 2 == 0 and KM.ST_SHIFT2 + 2 == KM.STATUS_WORDS          # the double sits on 8 bytes


def test_scratch_query_and_its_limits():
    q = KM.lib().gp_kmeans_scratch_bytes
    assert q(1, 1, 1) > 0 and q(2 ** 31 - 1, 64, 4096) > 0
    for bad, word in (((0, 35, 150), b"N = 0"), ((2 ** 31, 35, 150), b"N ="), ((1000, 0, 150), b"D = 0"), ((1000, 65, 150), b"D = 65"),
                      ((1000, 35, 0), b"K = 0"), ((1000, 35, 4097), b"K = 4097")):
        assert q(*bad) == -1 and word in KM.lib().gp_last_error(), bad
    # the partial sums stay a few tens of MB: at the bench's size, and at the largest table (fewer workgroups, more rows each)
    assert q(1_000_000, 35, 150) < 32 << 20
    assert q(1_000_000, 64, 4096) < 32 << 20


def test_refusals_need_no_gpu():
    l = KM.lib()
    for args, word in (((0, 3, None, 2, None, None, None, None), b"N = 0"), ((10, 65, None, 2, None, None, None, None), b"D = 65"),
                       ((10, 3, None, 4097, None, None, None, None), b"K = 4097"), ((10, 3, None, 2, None, None, None, None), b"null")):
        assert l.gp_kmeans_assign(*args) == 1 and word in l.gp_last_error(), args       # the C entry refuses before it looks at a pointer
    assert l.gp_cluster_mean(10, 3, None, None, 2, None, None, None, None) == 1 and b"null" in l.gp_last_error()
    assert l.gp_kmeans_run(10, 3, None, 2, None, 0, 0.0, *([None] * 3), 0, *([None] * 4)) == 1 and b"max_iters" in l.gp_last_error()
    assert l.gp_kmeans_run(10, 3, None, 2, None, 1001, 0.0, *([None] * 3), 0, *([None] * 4)) == 1 and b"max_iters" in l.gp_last_error()
    assert l.gp_kmeans_run(10, 3, None, 2, None, 5, -1.0, *([None] * 3), 0, *([None] * 4)) == 1 and b"tol" in l.gp_last_error()
    assert l.gp_kmeans_run(10, 3, None, 2, None, 5, float("nan"), *([None] * 3), 0, *([None] * 4)) == 1 and b"tol" in l.gp_last_error()
    assert l.gp_kmeans_run(10, 3, None, 2, None, 5, 0.0, *([None] * 3), 0, *([None] * 4)) == 1 and b"null" in l.gp_last_error()
    X, c = torch.zeros(8, 3), torch.zeros(2, 3)
    for call in (lambda: KM.assign(X, c), lambda: KM.cluster_mean(X, torch.zeros(8, dtype=torch.int64), 2), lambda: KM.kmeans(X, 2),
                 lambda: KM.kmeans(X, 2, init=c), lambda: KM.kmeans(X, 2, aux=X)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="K = 9 > N = 8"):
        KM.kmeans(X, 9)
    with pytest.raises(ValueError, match="K = 4097"):
        KM.kmeans(X, 4097)
    for kw, word in ((dict(iters=0), "iters"), (dict(iters=1001), "iters"), (dict(tol=-1.0), "tol")):
        with pytest.raises((ValueError, RuntimeError), match=word + "|no CPU fallback"):
            KM.kmeans(X, 2, **kw)


@pytest.mark.parametrize("bad", ["float64", "float16", "non-contiguous", "1-D", "D = 65"])
def test_dtype_and_layout_are_checked_before_any_launch(bad, monkeypatch):
    """The checks run on tensors that claim to be device tensors (is_cuda patched: no GPU is touched); a launch would fail the test."""
    X = {"float64": torch.zeros(8, 3, dtype=torch.float64), "float16": torch.zeros(8, 3, dtype=torch.float16),
         "non-contiguous": torch.zeros(3, 8).t(), "1-D": torch.zeros(8), "D = 65": torch.zeros(8, 65)}[bad]
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(KM, "lib", lambda: pytest.fail("a launch was reached"))
    good = torch.zeros(8, 3)
    for call in (lambda: KM.assign(X, good[:2]), lambda: KM.assign(good, X), lambda: KM.cluster_mean(X, torch.zeros(8, dtype=torch.int64), 2),
                 lambda: KM.kmeans(X, 2), lambda: KM.kmeans(good, 2, init=X), lambda: KM.kmeans(good, 2, aux=X)):
        with pytest.raises(RuntimeError, match="contiguous|must be \\["):
            call()
    with pytest.raises(RuntimeError, match="contiguous|must be \\["):
        KM.cluster_mean(good, torch.zeros(8, dtype=torch.float32), 2)


# ---- the shims ----
@pytest.mark.parametrize("name", SHIMS)
def test_shim_resolves_to_this_repository(name):
    m = importlib.import_module(name)
    assert os.path.realpath(m.__file__).startswith(os.path.realpath(ROOT) + os.sep), m.__file__
    assert "unpinned" in (m.__doc__ or ""), f"{name}: the docstring must state that parity is unpinned"
    assert "absent" in m.__doc__
    top = [l for l in inspect.getsource(m).splitlines() if l.startswith(("import ", "from "))]
    assert top == [], (name, top)                            # nothing is loaded at import: no torch, no library


def test_every_recorded_call_binds_to_the_shims():
    assert {i["import"] for i in SURFACE["imports"]} == {"kmeans_pytorch.kmeans", "torch_scatter.scatter"}
    seen = {}
    for call in SURFACE["calls"]:
        mod, name = call["callee"].rsplit(".", 1)
        fn = getattr(importlib.import_module(mod), name)
        inspect.signature(fn).bind(*range(call["positional"]), **{k: None for k in call["keywords"]})
        seen[call["callee"]] = call["unpacked"]
    assert seen == {"kmeans_pytorch.kmeans": 2, "torch_scatter.scatter": None}, seen
    import kmeans_pytorch
    import torch_scatter
    assert list(inspect.signature(kmeans_pytorch.kmeans).parameters) == ["X", "num_clusters", "distance", "cluster_centers", "tol", "tqdm_flag",
                                                                         "iter_limit", "device", "seed"]
    assert "return res.ids, res.centres" in inspect.getsource(kmeans_pytorch.kmeans)      # the arity the call site unpacks
    assert list(inspect.signature(torch_scatter.scatter).parameters) == ["src", "index", "dim", "out", "dim_size", "reduce"]
    d = {k: p.default for k, p in inspect.signature(kmeans_pytorch.kmeans).parameters.items()}
    assert (d["distance"], d["tol"], d["tqdm_flag"], d["iter_limit"], d["seed"]) == ("euclidean", 1e-4, True, 0, None)
    d = {k: p.default for k, p in inspect.signature(torch_scatter.scatter).parameters.items()}
    assert (d["dim"], d["out"], d["dim_size"], d["reduce"]) == (-1, None, None, "sum")


def test_shims_refuse_what_they_do_not_implement():
    import kmeans_pytorch
    import torch_scatter
    X = torch.zeros(8, 3)
    with pytest.raises(NotImplementedError, match="cosine"):
        kmeans_pytorch.kmeans(X, 2, distance="cosine")
    idx = torch.zeros(8, dtype=torch.int64)
    for kw, word in ((dict(reduce="max"), "max"), (dict(dim=1), "dim=1"), (dict(dim=-1), "dim=-1"), (dict(dim=0, out=X), "out=")):
        with pytest.raises(NotImplementedError, match=word):
            torch_scatter.scatter(X, idx, **{"dim": 0, **kw})
    with pytest.raises(NotImplementedError, match="2-D float"):
        torch_scatter.scatter(torch.zeros(8), idx, dim=0)
    with pytest.raises(NotImplementedError, match="2-D float"):
        torch_scatter.scatter(torch.zeros(8, 3, dtype=torch.int64), idx, dim=0)
    with pytest.raises(NotImplementedError, match="index"):
        torch_scatter.scatter(X, torch.zeros(8, 3, dtype=torch.int64), dim=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # what is implemented has no CPU path
        torch_scatter.scatter(X, idx, dim=0, reduce="mean")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kmeans_pytorch.kmeans(X=X, num_clusters=2, device=X.device)


# ---- the restatement ----
def test_restatement_agrees_with_training_kmeans_on_blobs():
    K = 4
    X, labels, _ = R.blobs(n=600, k=K)
    rows = lambda seed: torch.randperm(X.shape[0], generator=torch.Generator().manual_seed(seed))[:K]      # noqa: E731
    seed = next(s for s in range(1000) if labels[rows(s)].unique().numel() == K)       # the seeded subset holds one row of every blob
    ids_t, centres_t = training_kmeans(X, K, iters=20, seed=seed)
    ids_r, centres_r, counts, ran, _ = R.kmeans(X, X[rows(seed)].clone(), 20)
    assert torch.equal(ids_t, ids_r) and torch.equal(counts, torch.bincount(ids_t, minlength=K))
    assert torch.equal(labels[rows(seed)][ids_r], labels)                  # the clusters are the blobs
    assert (centres_t.double() - centres_r.double()).abs().max() <= 1e-6
    assert 2 <= ran <= 3


@pytest.mark.parametrize("n,k,d,kind", R.CAPPED)
def test_ambiguity_cap_on_the_reference_itself(n, k, d, kind):
    X, centres = R.make_input(n, k, d, kind)
    for it in range(6):
        frac = float(R.ambiguous_rows(X, centres).double().mean())
        assert frac <= R.AMBIGUOUS_CAP, (it, frac)
        ids, _ = R.assign(X, centres)
        centres = R.update(X, ids, centres)[0].float()


def test_ambiguous_rows_marks_a_tie_and_nothing_else():
    X = torch.tensor([[0.0, 0.0], [1.0, 0.0], [0.5, 0.0], [0.49, 0.0]])
    c = torch.tensor([[0.0, 0.0], [1.0, 0.0]])
    assert R.ambiguous_rows(X, c).tolist() == [False, False, True, False]
    assert R.assign(X, c)[0].tolist() == [0, 1, 0, 0]                     # the lower index on the tie
    assert not R.ambiguous_rows(X, c[:1]).any()
