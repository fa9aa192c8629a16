"""The PCA colouring on the device (feature_vis) against the float64 restatement tests/pca_ref.py over a grid of sizes, against sklearn's
recorded output (tests/golden/pca_vis.npz), and against itself: exact order statistics, equal bytes from run to run, the frozen basis
bit for bit; the jet colour map exactly; PCA_vis, draw_weights and draw_motion_feature through their files; render_features on a small
model; the refusals.

The grid's tolerances are 4 x the largest distance measured on an MI355X (DESIGN section 22 lists both); the data are seeded, so the
margin only covers another machine's last bits.  Colours may never need more than 1e-4 (1/39 of an 8-bit step)."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pca_ref as ref
import png_cases as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
NS, DS, DIMS = (5, 33, 257, 4099, 70001), (3, 8, 32, 61), (3, 5)
COLOR_CAP = 1e-4
COLOR_TOL = 1.71e-6        # colours and dim-5 positions against pca_ref: 4 x 4.255e-7 measured (colours 2.935e-7, positions 4.255e-7)
COMPONENT_TOL = 2.22e-7    # components, where the eigenvalues are separated: 4 x 5.548e-8
MEAN_TOL = 3.44e-6         # the mean: 4 x 8.583e-7
Q_TOL = 3.52e-7            # q1 and q99, in colour units, |difference| / (q99 - q1): 4 x 8.778e-8
VARIANCE_TOL = 2.1e-7      # explained_variance, relative to the largest: 4 x 5.241e-8
FIXTURE_TOL = 7.7e-6       # colours against sklearn's recorded output: 4 x 1.922e-6, measured on the device and for pca_ref alike
REF_TO_FIXTURE = 1.922e-6  # pca_ref against the same fixture, computed on the CPU when the fixture was made
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pca_vis.npz")
FIXTURE_CASES = ((33, 32, 3), (257, 32, 3), (4099, 32, 3), (4099, 32, 5))
EDGE_VALUES = [-0.1, 0, 0.5, 0.999, 1.0, 1.1, float("nan")]
GRID = [(N, D, dim) for N in NS for D in DS for dim in DIMS if dim <= min(N, D if dim == 3 else D + 3)]


def same(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else b
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def measured(name, value):
    print(f"PCA_MEASURE {name} {float(value):.3e}")
    return float(value)


@functools.lru_cache(maxsize=None)
def case(N, D, dim):
    """(xyz [N, 3], features [N, D], samples [N, D_total], the restatement's results, which components are well defined)."""
    if dim == 3:
        feats, xyz = ref.generate(N, D, 1000 * D + N), ref.generate(N, 3, 7000 + N)
    else:                                                         # the generator's rows are the samples [xyz, features]
        both = ref.generate(N, D + 3, 100000 + 1000 * D + N)
        xyz, feats = np.ascontiguousarray(both[:, :3]), np.ascontiguousarray(both[:, 3:])
    X = feats if dim == 3 else np.concatenate([xyz, feats], axis=-1)
    r = ref.pca_vis(X, dim)
    lam = ref.fit(X, min(dim + 1, X.shape[1]))[3]
    gaps = -np.diff(np.r_[lam, 0.0]) / lam[0]                    # gaps[k]: between eigenvalue k and k + 1
    defined = [gaps[k] > 1e-3 and (k == 0 or gaps[k - 1] > 1e-3) for k in range(dim)]
    for a in (feats, xyz, X):
        a.setflags(write=False)
    return xyz, feats, X, r, defined


def test_the_grid_is_the_stated_one_and_its_components_are_well_defined():
    assert len(GRID) == 40 and {(N, D) for N, D, _ in GRID} == {(N, D) for N in NS for D in DS}
    for N, D, dim in GRID:
        X, defined = case(N, D, dim)[2], case(N, D, dim)[4]
        # every component is separated from its neighbours by 1e-3 of the largest eigenvalue wherever the data can define it: more
        # columns than components, and more than dim nonzero eigenvalues (N - 1 of them at most: N = 5 with dim = 5 has four, so its
        # fifth component is any vector of the null space -- the colours do not depend on which, and are compared all the same)
        if X.shape[1] > dim and N - 1 > dim:
            assert all(defined), (N, D, dim)


@pytest.mark.parametrize("N,D,dim", GRID)
def test_fit_and_colours_against_the_restatement_and_from_run_to_run(N, D, dim):
    from gaussianprediction_amd import feature_vis as F
    xyz, feats, X, r, defined = case(N, D, dim)
    x = torch.tensor(X, device=DEV)
    model, y = F.pca_fit(x, dim, transformed=True)
    positions, colors = model.positions_colors(x)
    assert model.mean.shape == (X.shape[1],) and model.components.shape == (dim, X.shape[1]) and model.explained_variance.shape == (dim,)
    assert model.q1.shape == () and model.q99.shape == () and all(t.is_cuda and t.dtype == torch.float32 for t in (model.mean, model.q1, colors))
    scale = r["q99"] - r["q1"]
    e_mean = measured("mean", np.abs(model.mean.cpu().numpy() - r["mean"]).max())
    e_q = measured("q", max(abs(float(model.q1) - r["q1"]), abs(float(model.q99) - r["q99"])) / scale)
    e_col = measured("colour", np.abs(colors.cpu().numpy() - r["colors"]).max())
    if dim == 5:
        e_col = max(e_col, measured("position", np.abs(positions.cpu().numpy() - r["positions"]).max()))
        assert (positions[:, 2] == 1).all()
    else:
        assert positions is None
    comp = model.components.cpu().numpy()
    e_comp = measured("component", max([np.abs(comp[k] - r["components"][k]).max() for k in range(dim) if defined[k]], default=0.0))
    if X.shape[1] > dim:
        var = model.explained_variance.cpu().numpy()
        e_var = measured("variance", np.abs(var - r["explained_variance"]).max() / r["explained_variance"][0])
        assert e_var <= VARIANCE_TOL and (np.diff(var) <= 0).all()
    else:                                                          # dim == D: colours only
        e_comp = 0.0
    assert COLOR_TOL <= COLOR_CAP
    assert e_col <= COLOR_TOL and e_mean <= MEAN_TOL and e_q <= Q_TOL and e_comp <= COMPONENT_TOL, (e_col, e_mean, e_q, e_comp)
    for k in range(dim):                                           # the sign rule, on the device's own float32 components
        assert comp[k, np.argmax(np.abs(comp[k]))] > 0 or not defined[k]
    assert np.abs(np.linalg.norm(comp.astype(np.float64), axis=1) - 1).max() <= 1e-6
    # the projection is the definition's float32 loop on the device's own mean and components, and the colours its float32 formula
    assert same(y, ref.project32(X, model.mean.cpu().numpy(), comp))
    q1, q99 = np.float32(model.q1.item()), np.float32(model.q99.item())
    vis = (y.cpu().numpy() - q1) / (q99 - q1)
    assert same(colors, np.clip(vis[:, dim - 3:], np.float32(0), np.float32(1)))
    # exact selection: the order statistics are np.partition's of the device's own Y, the percentile is the definition's interpolation
    q, selected = F.percentiles(y, [1, 99], selected=True)
    want = ref.order_statistics(y.cpu().numpy(), [1, 99])
    assert np.array_equal(selected.cpu().numpy(), want) and same(q, model.q)
    assert same(q, np.array([ref.interpolate(lo, hi, p, y.numel()) for (lo, hi), p in zip(want, (1, 99))], np.float32))
    # two fits of one input give equal bytes in every output
    again, y2 = F.pca_fit(x.clone(), dim, transformed=True)
    for a, b in ((model.mean, again.mean), (model.components, again.components), (model.explained_variance, again.explained_variance),
                 (model.q, again.q), (y, y2), (colors, again.colors(x))):
        assert same(a, b)


@pytest.mark.parametrize("N,D,dim", [(40, 17, 3), (1500, 100, 3), (300, 128, 8), (2100, 65, 1), (200, 96, 3), (200, 97, 3)])
def test_widths_that_take_the_other_kernel_shapes(N, D, dim):
    """Beside the grid: one column past a 16-column lane tile, the widest lane tile, the widths whose Jacobi needs more LDS than a launch
    gets by default, and the last width whose eigenvectors are kept in LDS beside the first whose are not."""
    from gaussianprediction_amd import feature_vis as F
    X = ref.generate(N, D, 31 * D + N)
    mean, comp, var, lam = ref.fit(X, dim)
    model, y = F.pca_fit(torch.tensor(X, device=DEV), dim, transformed=True)
    got = model.components.cpu().numpy()
    assert measured("mean", np.abs(model.mean.cpu().numpy() - mean).max()) <= MEAN_TOL
    assert measured("variance", np.abs(model.explained_variance.cpu().numpy() - var).max() / var[0]) <= VARIANCE_TOL
    gaps = -np.diff(lam[:dim + 1]) / lam[0]
    for k in range(dim):
        if gaps[k] > 1e-3 and (k == 0 or gaps[k - 1] > 1e-3):
            assert measured("component", np.abs(got[k] - comp[k]).max()) <= COMPONENT_TOL, k
    assert same(y, ref.project32(X, model.mean.cpu().numpy(), got))
    if dim == 3:
        r = ref.pca_vis(X, dim)
        assert measured("colour", np.abs(model.colors(torch.tensor(X, device=DEV)).cpu().numpy() - r["colors"]).max()) <= COLOR_TOL


@pytest.mark.parametrize("dim", DIMS)
def test_frozen_basis_on_rows_that_were_not_in_the_fit(dim):
    from gaussianprediction_amd import feature_vis as F
    X = case(4099, 32, dim)[2]
    model = F.pca_fit(torch.tensor(X, device=DEV), dim)
    for rows in (1, 3, 700):
        other = ref.generate(rows, X.shape[1], 99 + rows) * np.float32(1.5)
        y = model.transform(torch.from_numpy(other).to(DEV))
        want = ref.project32(other, model.mean.cpu().numpy(), model.components.cpu().numpy())
        assert y.shape == (rows, dim) and same(y, want)
        q1, q99 = np.float32(model.q1.item()), np.float32(model.q99.item())
        vis = (want - q1) / (q99 - q1)
        positions, colors = model.positions_colors(torch.from_numpy(other).to(DEV))
        assert same(colors, np.clip(vis[:, dim - 3:], np.float32(0), np.float32(1))) and same(colors, model.colors(torch.from_numpy(other).to(DEV)))
        if dim == 5:
            assert same(positions, np.concatenate([vis[:, :2], np.ones((rows, 1), np.float32)], axis=-1))
        r = ref.colors_of(ref.project(other, model.mean.cpu().numpy(), model.components.cpu().numpy()), float(q1), float(q99))[1]
        assert measured("colour", np.abs(colors.cpu().numpy() - r).max()) <= COLOR_TOL


@pytest.mark.parametrize("N,D,dim", FIXTURE_CASES)
def test_fixture_cases_against_sklearns_recorded_output(N, D, dim):
    from gaussianprediction_amd import feature_vis as F
    g = np.load(GOLDEN)
    tag = f"{N}_{D}_{dim}"
    xyz, feats = torch.from_numpy(g[f"xyz_{N}"]).to(DEV), torch.from_numpy(g[f"features_{N}"]).to(DEV)
    positions, colors = F.PCA_vis(xyz, feats, dim=dim, return_only=True)
    e = measured("fixture", np.abs(colors.cpu().numpy() - g[f"colors_{tag}"]).max())
    if dim == 5:
        e = max(e, measured("fixture_position", np.abs(positions.cpu().numpy() - g[f"positions_{tag}"]).max()))
    else:
        assert same(positions, g[f"xyz_{N}"])
    assert FIXTURE_TOL <= COLOR_CAP and FIXTURE_TOL >= 4 * REF_TO_FIXTURE and e <= FIXTURE_TOL, e


def test_percentiles_of_awkward_arrays_are_exact():
    from gaussianprediction_amd import feature_vis as F
    rng = np.random.default_rng(11)
    inf = np.inf
    arrays = [np.array([3.25]), np.full(1000, -2.5), rng.permutation(np.r_[np.full(40, 1.5), np.full(61, -7.0)]),
              rng.permutation(np.r_[np.full(3, -inf), rng.normal(size=200), np.full(3, inf)]), rng.normal(size=101),
              rng.normal(size=300001) * 10.0 ** rng.integers(-20, 20, size=300001), rng.normal(size=(257, 3))]
    for a in arrays:
        a = np.ascontiguousarray(a, dtype=np.float32)
        for qs in ([1, 99], [0, 100], [50]):
            q, selected = F.percentiles(torch.from_numpy(a).to(DEV), qs, selected=True)
            want = ref.order_statistics(a, qs)
            assert same(selected, want), (a.shape, qs)
            with np.errstate(invalid="ignore"):
                want_q = np.array([ref.interpolate(lo, hi, p, a.size) for (lo, hi), p in zip(want, qs)], np.float32)
            assert np.array_equal(q.cpu().numpy(), want_q, equal_nan=True) and q.dtype == torch.float32
    zeros = torch.from_numpy(np.r_[np.full(50, 0.0), np.full(50, -0.0)].astype(np.float32)).to(DEV)          # -0 sorts below +0
    assert np.signbit(F.percentiles(zeros, [49.5], selected=True)[1].cpu().numpy()).tolist() == [[True, False]]


def test_colormap_is_the_table_lookup_exactly():
    from gaussianprediction_amd import feature_vis as F
    lut = F.jet_lut()
    assert lut.shape == (256, 3) and lut.is_cuda and F.jet_lut(DEV) is lut and same(lut, F.jet_table())
    rng = np.random.default_rng(3)
    x = np.r_[np.array(EDGE_VALUES + [np.inf, -np.inf, 255 / 256, 1 / 256, -0.0]), rng.uniform(-0.2, 1.2, size=1500), np.arange(257) / 256].astype(np.float32)
    idx = ref.lut_index(x)
    want = np.where(idx[:, None] < 0, np.float32(0), F.jet_table()[np.clip(idx, 0, 255)])
    got = F.colormap(torch.from_numpy(x).to(DEV))
    assert same(got, want) and idx[:7].tolist() == [0, 0, 128, 255, 255, 255, -1] and not got[6].any()
    assert same(F.colormap(torch.from_numpy(x[:1500].reshape(30, 50)).to(DEV)), want[:1500].reshape(30, 50, 3))
    grey = torch.linspace(0, 1, 256, device=DEV)[:, None].repeat(1, 3).contiguous()
    assert same(F.colormap(torch.from_numpy(x).to(DEV), lut=grey), np.where(idx[:, None] < 0, np.float32(0), grey.cpu().numpy()[np.clip(idx, 0, 255)]))
    assert F.colormap(torch.zeros(0, device=DEV)).shape == (0, 3)


def test_pca_vis_returns_and_writes_what_the_restatement_gives(tmp_path):
    from gaussianprediction_amd import feature_vis as F, io_formats as IO
    for dim in DIMS:
        xyz, feats, X, r, _ = case(4099, 32, dim)
        tx, tf = torch.tensor(xyz, device=DEV), torch.tensor(feats, device=DEV)
        positions, colors = F.PCA_vis(tx, tf, dim=dim, return_only=True)
        assert positions.is_cuda and colors.is_cuda and np.abs(colors.cpu().numpy() - r["colors"]).max() <= COLOR_TOL
        if dim == 5:
            assert np.abs(positions.cpu().numpy() - r["positions"]).max() <= COLOR_TOL and (positions[:, 2] == 1).all()
            assert float(positions[:, :2].min()) < 0 and float(positions[:, :2].max()) > 1          # unclipped
        else:
            assert same(positions, xyz)
        path = str(tmp_path / f"cloud_{dim}.ply")
        assert F.PCA_vis(tx, tf, path, dim=dim) is None
        back = F.PCA_vis(tx, tf, path, dim=dim, finish_return=True)
        assert same(back[0], positions) and same(back[1], colors)
        v = IO.read_ply_vertices(path)
        assert v.dtype.names == ("x", "y", "z", "red", "green", "blue") and len(v) == 4099
        assert same(np.stack([v["x"], v["y"], v["z"]], axis=-1), positions.cpu().numpy().astype(np.float64))
        assert same(np.stack([v["red"], v["green"], v["blue"]], axis=-1), IO.color_to_uint8(colors.cpu().numpy()).reshape(-1, 3))


def test_draw_weights_and_draw_motion_feature_write_the_references_text(tmp_path):
    from gaussianprediction_amd import feature_vis as F
    xyz, feats = case(257, 32, 3)[:2]
    tx, tf = torch.tensor(xyz, device=DEV), torch.tensor(feats, device=DEV)
    table = F.jet_table()
    colors = F.draw_motion_feature(tx, tf, str(tmp_path / "vis_feature.txt"))
    model, y = F.pca_fit(tf, 1, transformed=True)
    want = table[np.clip(ref.lut_index(y[:, 0].cpu().numpy()), 0, 255)]       # un-normalised, as the reference: most rows are an end of the table
    text = np.loadtxt(str(tmp_path / "vis_feature.txt"))
    assert same(colors, want) and text.shape == (257, 7) and np.array_equal(text, np.concatenate([xyz, want, np.ones((257, 1))], axis=-1).astype(np.float64))
    assert np.abs(y[:, 0].cpu().numpy() - ref.pca_vis(feats, 1)["Y"][:, 0]).max() <= 1e-4 * np.abs(y.cpu().numpy()).max()
    weights = torch.rand(257, 6, generator=torch.Generator().manual_seed(2)).to(DEV)
    kpts = torch.randn(6, 5, generator=torch.Generator().manual_seed(3)).to(DEV)
    colors = F.draw_weights(weights, tx, kpts, 4, directory=str(tmp_path / "visualize"))
    want = table[ref.lut_index(weights[:, 4].cpu().numpy())]
    assert same(colors, want) and sorted(os.listdir(tmp_path / "visualize")) == ["kpts4.txt", "weights_xyz_4.txt"]
    assert np.array_equal(np.loadtxt(str(tmp_path / "visualize" / "weights_xyz_4.txt")), np.concatenate([xyz, want], axis=-1).astype(np.float64))
    assert np.array_equal(np.loadtxt(str(tmp_path / "visualize" / "kpts4.txt")), kpts[4, :3].cpu().numpy().astype(np.float64)[None].repeat(3, axis=0))


def test_render_features_writes_its_directory_and_the_override_colour_renders(tmp_path):
    from PIL import Image
    import gaussianprediction_amd as gpa
    from gaussianprediction_amd import eval_render as ER, feature_vis as F
    from gaussianprediction_amd.cameras import orbit_cameras
    from test_gpu_render import build
    W, H, IT = 64, 48, 50000
    pc = build(N=3000, K=60, W=W, H=H)[0]
    views = orbit_cameras(2, 4.0, 0.6911, W, H, device=DEV)
    pipe, bg = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False), torch.zeros(3, device=DEV)
    root = str(tmp_path / "model")
    out_path, model = ER.render_features(root, "test", IT, views, pc, pipe, bg)
    assert out_path == os.path.join(root, "eval", "test", f"ours_{IT}", "features") and isinstance(model, F.PcaModel) and model.dim == 3
    tree = sorted(os.path.relpath(os.path.join(d, f), root) for d, _, files in os.walk(root) for f in files)
    assert tree == [os.path.join("eval", "test", f"ours_{IT}", "features", f"{i:05d}.png") for i in range(2)]
    feats = pc.motion_feature.detach().contiguous()
    want_model = F.pca_fit(feats, 3)
    assert same(model.components, want_model.components) and same(model.q, want_model.q)
    colors = want_model.colors(feats)
    for i, cam in enumerate(views):
        with torch.no_grad():
            want = gpa.render(cam, pc, pipe, bg, time=torch.from_numpy(cam.time).to(DEV), it=IT, override_color=colors)["render"]
            plain = gpa.render(cam, pc, pipe, bg, time=torch.from_numpy(cam.time).to(DEV), it=IT)["render"]
        assert float(want.max()) > 0.05 and not torch.equal(want, plain)
        got = np.array(Image.open(os.path.join(root, tree[i])))
        assert got.shape == (H, W, 3) and np.array_equal(got, P.quantise(want.cpu().numpy()).transpose(1, 2, 0)), i
    # a frozen basis and a caller's features: nothing is fitted, the same files are written again
    half = (feats * 0.5).contiguous()
    _, given = ER.render_features(root, "test", IT, views[:1], pc, pipe, bg, features=half, model=want_model)
    assert given is want_model
    with torch.no_grad():
        want = gpa.render(views[0], pc, pipe, bg, time=torch.from_numpy(views[0].time).to(DEV), it=IT, override_color=want_model.colors(half))["render"]
    assert np.array_equal(np.array(Image.open(os.path.join(root, tree[0]))), P.quantise(want.cpu().numpy()).transpose(1, 2, 0))


def test_what_the_module_refuses():
    from gaussianprediction_amd import _lib, feature_vis as F
    x = torch.tensor(case(33, 8, 3)[1], device=DEV)
    for bad, word in ((x.cpu(), "no CPU fallback"), (x.double(), "float32"), (x[:, ::2], "contiguous"), (x.t(), "contiguous"), (x[0], "dimension")):
        with pytest.raises(RuntimeError, match=word):
            F.pca_fit(bad)
    for bad, dim, word in ((x, 9, r"dim must be in 1 \.\. min\(8, D, N\)"), (x[:, :2].contiguous(), 3, "dim must be"), (x[:1], 1, "N must be >= 2"),
                           (x[:2], 3, "dim must be"), (x, 0, "dim must be")):
        with pytest.raises(_lib.GpHipError, match=word):
            F.pca_fit(bad, dim)
    model = F.pca_fit(x)
    with pytest.raises(RuntimeError, match="basis is for D = 8"):
        model.transform(x[:, :4].contiguous())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.colors(x.cpu())
    with pytest.raises(_lib.GpHipError, match="colours need dim 3 or 5"):
        F.pca_fit(x, 4).colors(x)
    with pytest.raises(_lib.GpHipError, match="number of percentiles"):
        F.percentiles(x, [1, 50, 99])
    with pytest.raises(_lib.GpHipError, match="0 .. 100"):
        F.percentiles(x, [-1])
    with pytest.raises(RuntimeError, match="float32"):
        F.colormap(x.double())
    with pytest.raises(RuntimeError, match=r"\[256, 3\]"):
        F.colormap(x, lut=torch.zeros(255, 3, device=DEV))
    with pytest.raises(RuntimeError, match="must be 3 or 5"):
        F.PCA_vis(x[:, :3].contiguous(), x, dim=4, return_only=True)
    with pytest.raises(RuntimeError, match=r"\[N, 3\]"):
        F.PCA_vis(x[:5, :3].contiguous(), x, return_only=True)
