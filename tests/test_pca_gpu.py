"""PCA on the GPU: the kernels of csrc/pca.hip through ops.py — exactly, on small-integer tables whose every sum is an integer
(which is also the lane-map check of the f64 MFMA: a wrong row formula cannot give x^T x), and within the derived bounds of
tests/pca_ref.py on planted real-valued ones — the bits against launch geometry, then the model's pca() against the ops sequence
on its own rows and against float64 numpy, pca_transform, whitening, no side effects on training, refusals, and the command line
(GCN_PCA)."""
import os
import subprocess
import threading

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import pca_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")
DIMS = [1, 5, 16, 17, 41, 128, 256]
NS = [2, 3, 4, 5, 63, 64, 65, 1000, R.PART - 1, R.PART, R.PART + 1, 2 * R.PART + 3]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def dev():
    from cuda_gcn_amd.ops import Device
    d = Device(0)
    yield d
    d.close()


def strides(dim, which):
    return dim + 3 if which else (dim + 3) // 4 * 4 + 4


def row_list(n, seed):
    """a list of n + 3 positions with repeats, a -1 and an n"""
    q = np.random.default_rng(seed).integers(0, n, n + 3).astype(np.int32)
    q[1], q[n], q[-1] = -1, n, q[0]
    return q


# ---- exactly, on integer tables ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", DIMS)
def test_sums_are_exact_on_integer_tables(dev, dim):
    """entries in {-3..3}, inverse norms that are powers of two: the mean is the integer column sum / count, the uncentred scatter
    the integer x^T x (asymmetric in its tile pairs: a swapped or misplaced result row shows), S is symmetric bit for bit, and a
    projection with an integer basis, an integer mean and power-of-two scales is exact in f32"""
    rng = np.random.default_rng(100 + dim)
    k = min(dim, 7)
    basis = rng.integers(-2, 3, (k, dim)).astype(np.float64)
    off = rng.integers(-4, 5, dim).astype(np.float64)
    scale = 2.0 ** rng.integers(-3, 4, k)
    for idx, n in enumerate(NS):
        t = rng.integers(-3, 4, (n, dim)).astype(np.float32)
        ld = strides(dim, idx % 2)
        inv = (2.0 ** rng.integers(-1, 2, n)).astype(np.float32) if idx % 3 == 0 else None
        for rows in (None, row_list(n, idx)):
            x, ok = R.rows_used(t, rows, inv)
            count = int(ok.sum())
            mean, got_count = dev.pca_mean(t, rows=rows, inv_norm=inv, ld=ld)
            assert got_count == count, (n, got_count, count)
            assert same_bits(mean, x.astype(np.float64).sum(0) / count), (n, rows is None)
            s = dev.pca_scatter(t, rows=rows, inv_norm=inv, ld=ld)
            x64 = x.astype(np.float64)
            assert np.array_equal(s, x64.T @ x64), (n, rows is None, np.abs(s - x64.T @ x64).max())
            assert same_bits(s, s.T)
            y = dev.pca_project(t, basis, mean=off, scale=scale, rows=rows, inv_norm=inv, ld=ld, ldy=k + 2)
            want = np.full((ok.size, k), np.nan, np.float32)
            want[ok] = (((x64 - off) @ basis.T) * scale).astype(np.float32)
            assert same_bits(y, want), (n, rows is None)
            plain = dev.pca_project(t, basis, rows=rows, inv_norm=inv, ld=ld)
            want[ok] = (x64 @ basis.T).astype(np.float32)
            assert same_bits(plain, want), (n, rows is None)


@pytest.mark.parametrize("dim", DIMS)
def test_centred_scatter_is_exact_on_mirrored_rows(dev, dim):
    """rows [t; -t] + an integer offset: the mean is the offset and the centred scatter 2 t^T t, exactly"""
    rng = np.random.default_rng(200 + dim)
    for idx, m in enumerate((1, 2, 32, 33, 500, R.PART // 2 + 1, R.PART + 2)):
        t = rng.integers(-3, 4, (m, dim)).astype(np.float64)
        off = rng.integers(-5, 6, dim).astype(np.float64)
        table = (np.concatenate([t, -t]) + off).astype(np.float32)
        ld = strides(dim, idx % 2)
        mean, count = dev.pca_mean(table, ld=ld)
        assert count == 2 * m and np.array_equal(mean, off), m
        s = dev.pca_scatter(table, mean, ld=ld)
        assert np.array_equal(s, 2 * t.T @ t), (m, np.abs(s - 2 * t.T @ t).max())
        assert same_bits(s, s.T)


# ---- within the bounds, on planted tables -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", DIMS)
def test_planted_tables_stay_inside_the_bounds(dev, dim):
    """|S - S_ref| <= (n + 2) 2^-53 |c|^T |c| entrywise with S_ref in longdouble from the same float64 mean, and
    |y - y_ref| <= (h + 2) 2^-53 |scale| sum |c| |v| + 2^-24 |y_ref|.  The mean, n float64 additions and a division:
    |mean - mean_ref| <= (n + 1) 2^-53 sum |x| / count."""
    from cuda_gcn_amd.model import pca_from_scatter
    for n, use_inv, rows in ((1000, False, None), (2 * R.PART + 3, True, None), (1000, False, row_list(1000, dim))):
        table = R.planted(n, dim, 300 + dim)
        inv = dev.embed_inv_norms(table) if use_inv else None
        x, ok = R.rows_used(table, rows, inv)
        cnt = x.shape[0]
        mean, count = dev.pca_mean(table, rows=rows, inv_norm=inv)
        assert count == cnt
        err = np.abs(mean - R.mean_ref(x))
        bound = (cnt + 1) * R.U * np.abs(x.astype(np.float64)).sum(0) / cnt
        print(f"dim={dim} n={n}: mean error / bound {np.max(err / bound):.3g}")
        assert np.all(err <= bound)
        for mu in (mean, None):
            s = dev.pca_scatter(table, mu, rows=rows, inv_norm=inv)
            s_ref, absprod = R.scatter_ref(x, mu)
            ratio = np.abs(s - s_ref) / R.scatter_bound(cnt, absprod)
            print(f"dim={dim} n={n} centred={mu is not None}: scatter error / bound {ratio.max():.3g}")
            assert np.all(np.abs(s - s_ref) <= R.scatter_bound(cnt, absprod))
            assert same_bits(s, s.T)
        s = dev.pca_scatter(table, mean, rows=rows, inv_norm=inv)
        k = min(dim, 9)
        fit = pca_from_scatter(s, mean, cnt, k=k, whiten=True)
        for scale in (None, fit["scale"]):
            y = dev.pca_project(table, fit["components"], mean=mean, scale=scale, rows=rows, inv_norm=inv)
            y_ref, ybound = R.project_ref(x, mean, fit["components"], scale)
            assert np.all(np.isnan(y[~ok])) and np.all(np.isfinite(y[ok]))
            ratio = np.abs(y[ok] - y_ref) / ybound
            print(f"dim={dim} n={n} whiten={scale is not None}: projection error / bound {ratio.max():.3g}")
            assert np.all(np.abs(y[ok] - y_ref) <= ybound)


# ---- the bits do not depend on how the work was launched --------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [5, 41, 128, 256])
def test_bits_do_not_depend_on_the_launch(dev, dim):
    n = 2 * R.PART + 3
    table = R.planted(n, dim, 400 + dim)
    inv = dev.embed_inv_norms(table)
    plan = dev.pca_plan(n, dim)
    assert plan["bytes_full"] == 3 * plan["bytes_min"]
    mean, count = dev.pca_mean(table, inv_norm=inv)
    s = dev.pca_scatter(table, mean, inv_norm=inv)
    # a second launch
    assert same_bits(dev.pca_mean(table, inv_norm=inv)[0], mean) and same_bits(dev.pca_scatter(table, mean, inv_norm=inv), s)
    # less scratch: one part per launch, and two
    for nbytes in (plan["bytes_min"], 2 * plan["bytes_min"] + 8):
        assert same_bits(dev.pca_mean(table, inv_norm=inv, scratch_bytes=nbytes)[0], mean), nbytes
        assert same_bits(dev.pca_scatter(table, mean, inv_norm=inv, scratch_bytes=nbytes), s), nbytes
    # the identity list, and another row stride
    every = np.arange(n, dtype=np.int32)
    assert same_bits(dev.pca_mean(table, rows=every, inv_norm=inv, ld=dim + 5)[0], mean)
    assert same_bits(dev.pca_scatter(table, mean, rows=every, inv_norm=inv, ld=dim + 5), s)
    # a projection in one batch as in two halves
    comp = R.orthogonal(dim, np.random.default_rng(dim))[:min(dim, 50)]
    y = dev.pca_project(table, comp, mean=mean, inv_norm=inv)
    cut = 1037
    halves = [dev.pca_project(table, comp, mean=mean, rows=every[a:b], inv_norm=inv) for a, b in ((0, cut), (cut, n))]
    assert same_bits(y, np.concatenate(halves))
    assert same_bits(y, dev.pca_project(table, comp, mean=mean, inv_norm=inv))


def test_a_skipped_position_gives_a_nan_row_and_lowers_the_count(dev):
    table = R.planted(70, 17, 5)
    rows = np.array([3, -1, 69, 70, 3, 2 ** 31 - 1, 0], np.int32)
    mean, count = dev.pca_mean(table, rows=rows)
    assert count == 4
    assert same_bits(mean, dev.pca_mean(table, rows=np.array([3, 69, 3, 0], np.int32))[0])
    assert same_bits(dev.pca_scatter(table, mean, rows=rows), dev.pca_scatter(table, mean, rows=np.array([3, 69, 3, 0], np.int32)))
    y = dev.pca_project(table, np.eye(17)[:3], mean=mean, rows=rows)
    assert np.array_equal(np.isnan(y).all(1), [False, True, False, True, False, True, False]) and not np.isnan(y[[0, 2, 4, 6]]).any()
    none, count = dev.pca_mean(table, rows=np.array([-1, 70], np.int32))
    assert count == 0 and np.all(np.isnan(none))


def test_kernel_refusals(dev):
    from cuda_gcn_amd.ops import GcnHipError
    t = np.zeros((8, 4), np.float32)
    with pytest.raises(GcnHipError, match="gcnhip_pca_mean: 1 <= dim <= 256"):
        dev.pca_mean(np.zeros((2, 257), np.float32), scratch_bytes=4096)
    with pytest.raises(GcnHipError, match="gcnhip_pca_scatter: the scratch is below the minimum"):
        dev.pca_scatter(t, scratch_bytes=2040)
    with pytest.raises(GcnHipError, match="gcnhip_pca_mean: the scratch is below the minimum"):
        dev.pca_mean(t, scratch_bytes=16)
    with pytest.raises(GcnHipError, match="gcnhip_pca_project: 1 <= k <= dim"):
        dev.pca_project(t, np.zeros((5, 4)))
    with pytest.raises(GcnHipError, match="gcnhip_pca_project: a row stride is below k"):
        dev.pca_project(t, np.zeros((3, 4)), ldy=2)


# ---- the model --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def trained_planted():
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.planted_communities(n_comm=8, size=128, p_in=0.5, feats=8)
    m = HipGCNModel(ds, seed=5, hidden_dim=16, dropout=0.0)
    m.run_epochs(10, want_trace=False)
    yield ds, m
    m.close()


def ops_pca(dev, table, inv, k, center=True, whiten=False, rows=None):
    from cuda_gcn_amd.model import pca_from_scatter
    n = table.shape[0] if rows is None else len(rows)
    mean = dev.pca_mean(table, rows=rows, inv_norm=inv)[0] if center else None
    s = dev.pca_scatter(table, mean, rows=rows, inv_norm=inv)
    fit = pca_from_scatter(s, mean, n, k=k, whiten=whiten)
    fit.update(mean=mean if center else np.zeros(table.shape[1]), scatter=s,
               coords=dev.pca_project(table, fit["components"], mean=mean, scale=fit["scale"], rows=rows, inv_norm=inv))
    return fit


KEYS = ("mean", "components", "eigenvalues", "explained_variance", "explained_variance_ratio", "singular_values", "coords", "scatter")


def test_pca_is_the_ops_sequence_on_the_models_rows(dev, trained_planted):
    ds, m = trained_planted
    n, h = ds["num_nodes"], 16
    table = m.embed()
    inv = dev.embed_inv_norms(table)
    assert same_bits(m.embed(normalize=True), dev.embed_rows(table, inv_norm=inv))
    for k, normalize, center, whiten in ((2, True, True, False), (16, True, True, True), (5, False, True, False), (3, True, False, True)):
        got = m.pca(k=k, normalize=normalize, center=center, whiten=whiten, return_scatter=True)
        want = ops_pca(dev, table, inv if normalize else None, k, center, whiten)
        for key in KEYS:
            assert same_bits(got[key], want[key]), (k, normalize, center, whiten, key)
        assert got["rank"] == want["rank"] and got["rows"] == n and got["coords"].shape == (n, k)
        assert (got["scale"] is None) == (not whiten) and (not whiten or same_bits(got["scale"], want["scale"]))
        assert (got["normalize"], got["center"], got["whiten"]) == (normalize, center, whiten)
    full = m.pca(k=4, return_scatter=True)
    again = m.pca(k=4, return_scatter=True, scratch_bytes=1)      # the small-scratch path gives the same bits
    assert all(same_bits(full[key], again[key]) for key in KEYS)
    assert m.pca(k=4, coords=False)["coords"] is None and "scatter" not in m.pca(k=4, coords=False)


def test_pca_agrees_with_float64_numpy(trained_planted):
    """numpy PCA in float64 of embed(normalize=True).  Both pairs are held against the GPU's scatter matrix S:
    E = |S V - V L|_F of the fit + |S U - U W|_F of numpy's eigh of its own float64 c^T c.  Eigenvalues agree within E (Weyl), the
    ratios within E / trace(S) + 2 (n + h) 2^-53 ratio (each total is a float64 sum of h sums of n terms), a component, up to
    sign, within the angle E / gap where the gap is above 8e-4 lambda_1, and on those components the coordinates agree with numpy's
    c u_j within the projection's own bound (tests/pca_ref.project_ref) + |c_i|_2 E / gap_j + |mean - mean_numpy|_2."""
    from cuda_gcn_amd.model import sym_eigen
    ds, m = trained_planted
    n, h = ds["num_nodes"], 16
    x = m.embed(normalize=True)
    got = m.pca(k=h, return_scatter=True)
    S = got["scatter"]
    x64 = x.astype(np.float64)
    mu = x64.mean(0)
    c = x64 - mu
    w, u = R.eigh_desc(c.T @ c)
    lam, v = sym_eigen(S)
    E = np.linalg.norm(S @ v - v * lam) + np.linalg.norm(S @ u - u * w)
    print(f"the two residual norms {E:.3g}; eigenvalue difference {np.abs(got['eigenvalues'] - np.maximum(w, 0)).max():.3g}")
    assert np.abs(got["mean"] - mu).max() <= (n + 1) * R.U * np.abs(x64).mean(0).max() * 2
    assert np.abs(got["eigenvalues"] - np.maximum(w, 0)).max() <= E
    ratio = np.maximum(w, 0) / np.maximum(w, 0).sum()
    assert np.all(np.abs(got["explained_variance_ratio"] - ratio) <= E / np.trace(S) + 2 * (n + h) * R.U * ratio)
    assert np.abs(got["explained_variance"] - np.maximum(w, 0) / (n - 1)).max() <= E / (n - 1)
    d = np.r_[np.inf, np.abs(np.diff(w)), np.inf]
    gaps = np.minimum(d[:-1], d[1:])
    y_ref, bound = R.project_ref(x, got["mean"], got["components"])
    assert np.all(np.abs(got["coords"] - y_ref) <= bound)
    dmu, cnorm = np.linalg.norm(got["mean"] - mu), np.linalg.norm(c, axis=1)
    checked = 0
    for j in range(h):
        if gaps[j] > 8e-4 * w[0]:
            theirs = u[:, j] * np.sign(u[np.argmax(np.abs(u[:, j])), j])
            angle = np.linalg.norm(got["components"][j] - theirs)
            print(f"component {j}: angle {angle:.3g}, allowed {E / gaps[j]:.3g}")
            assert angle <= E / gaps[j], j
            assert np.all(np.abs(got["coords"][:, j] - c @ theirs) <= bound[:, j] + cnorm * E / gaps[j] + dmu), j
            checked += 1
    assert checked >= 2


def test_transform_and_split_queries(trained_planted):
    ds, m = trained_planted
    n = ds["num_nodes"]
    split = np.asarray(ds["split"])
    fit = m.pca(k=3, whiten=True)
    nodes = np.array([5, 900, 5, 0, n - 1], np.int32)
    assert same_bits(m.pca_transform(fit, nodes), fit["coords"][nodes])
    assert same_bits(m.pca_transform(fit), fit["coords"])
    # a fit on the training split places every node; the split and the node query list the same rows
    train = np.flatnonzero(split == 1).astype(np.int32)
    a, b = m.pca(k=2, split=1), m.pca(k=2, nodes=train)
    assert a["rows"] == train.size and all(same_bits(a[key], b[key]) for key in KEYS if key != "scatter")
    y = m.pca_transform(a)
    assert y.shape == (n, 2) and np.all(np.isfinite(y)) and same_bits(y[train], a["coords"])
    rep = m.pca(k=2, nodes=[7, 7, 7, 2])                          # repeats count as often as listed
    assert rep["rows"] == 4 and rep["rank"] == 1 and same_bits(rep["coords"][0], rep["coords"][1])
    # without centring or normalising the transform follows the fit's flags
    for kw in (dict(center=False), dict(normalize=False), dict(center=False, normalize=False, whiten=True)):
        f = m.pca(k=4, **kw)
        assert same_bits(m.pca_transform(f, nodes), f["coords"][nodes]), kw


def test_whitened_coordinates_have_unit_variance(trained_planted):
    """sample variance 1 within 2^-22 + 8 h 2^-52 lambda_1 / lambda_j for every component inside the rank, 0 past it"""
    ds, m = trained_planted
    h = 16
    fit = m.pca(k=h, whiten=True)
    y = fit["coords"].astype(np.float64)
    lam = fit["eigenvalues"]
    for j in range(h):
        var = (y[:, j] ** 2).sum() / (fit["rows"] - 1)
        if j < fit["rank"]:
            print(f"component {j}: |variance - 1| = {abs(var - 1):.3g}, allowed {2.0 ** -22 + 8 * h * R.EPS * lam[0] / lam[j]:.3g}")
            assert abs(var - 1) <= 2.0 ** -22 + 8 * h * R.EPS * lam[0] / lam[j], j
        else:
            assert fit["scale"][j] == 0 and np.all(y[:, j] == 0), j
    assert np.all(np.isfinite(fit["coords"])) and np.all(np.isfinite(fit["scale"]))


def test_a_pca_call_between_epochs_changes_nothing():
    from cuda_gcn_amd import model as M
    ds = datagen.make_dataset("cora-syn")
    a = M.HipGCNModel(ds, seed=6, hidden_dim=16, dropout=0.5)
    b = M.HipGCNModel(ds, seed=6, hidden_dim=16, dropout=0.5)
    ta, tb = [a.run_epochs(3)], [b.run_epochs(3)]
    before = b.predict(logp=True)
    fit = b.pca(k=3, whiten=True)
    b.pca(k=2, split=2, normalize=False, center=False)
    b.pca_transform(fit, nodes=[1, 2, 3])
    assert all(same_bits(x, y) for x, y in zip(before, b.predict(logp=True)))
    ta.append(a.run_epochs(2))
    tb.append(b.run_epochs(2))
    ta, tb = np.concatenate(ta), np.concatenate(tb)
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32)), (ta, tb)
    for v in (2, 5):
        assert same_bits(a.var(v), b.var(v)), v
    assert a.eval(3) == b.eval(3) and same_bits(a.var(6), b.var(6)) and same_bits(a.var(3), b.var(3))
    a.close()
    b.close()


def test_refusals():
    from cuda_gcn_amd import model as M
    from cuda_gcn_amd.model import HipGCNModel, GcnHostError, _ck
    from tests.mr_threads import ThreadWorld
    ds = datagen.make_dataset("tiny-syn")
    n = ds["num_nodes"]
    m = HipGCNModel(ds, seed=1, hidden_dim=16)
    for k in (0, 17, "two", 2.5):
        with pytest.raises(GcnHostError, match=r"pca: k must be an integer in 1\.\.16"):
            m.pca(k=k)
    info = np.zeros(3, np.int64)

    def raw(model, k=2, split=0, nodes=None, count=0):
        return model.lib.gcnhost_model_pca_fit(model.h, k, split, nodes, count, 1, 1, 0, 0, 0, None, None, None, None, None, None, None, info.ctypes.data)
    for k in (0, 17):
        with pytest.raises(GcnHostError, match=r"pca: k must be in 1\.\.16, got"):
            _ck(m.lib, raw(m, k=k), "call")
    for split in (-1, 4):
        with pytest.raises(GcnHostError, match="pca: invalid argument \\(split is 0 with a node query"):
            _ck(m.lib, raw(m, split=split), "call")
    with pytest.raises(GcnHostError, match="pca: split is 1"):
        m.pca(split=4)
    with pytest.raises(GcnHostError, match="pca: give a split or a node query"):
        m.pca(split=1, nodes=[0, 1])
    for nodes in ([3], []):
        with pytest.raises(GcnHostError, match=f"pca: at least 2 rows, the query lists {len(nodes)}"):
            m.pca(nodes=nodes)
    with pytest.raises(GcnHostError, match="pca: .*not a node of the dataset"):
        m.pca(nodes=[0, n])
    with pytest.raises(GcnHostError, match="pca_transform: .*not a node of the dataset"):
        m.pca_transform(m.pca(), nodes=[-1])
    fit = m.pca(k=2, whiten=True)
    with pytest.raises(GcnHostError, match="pca_transform: the fit is of width 15, the hidden layer of width 16"):
        m.pca_transform(dict(fit, components=fit["components"][:, :15], mean=fit["mean"][:15]))
    for key in ("components", "mean", "scale"):
        broken = fit[key].copy()
        broken.flat[-1] = np.inf
        with pytest.raises(GcnHostError, match=f"pca_transform: the fit is not finite \\({key}\\)"):
            m.pca_transform(dict(fit, **{key: broken}))
    with pytest.raises(GcnHostError, match="pca_transform: the scale has 1 entries for 2 components"):
        m.pca_transform(dict(fit, scale=fit["scale"][:1]))
    assert m.pca_transform(fit, nodes=[]).shape == (0, 2)
    m.close()
    bf = HipGCNModel(ds, seed=1, flags=M.BF16_TABLES, hidden_dim=16)
    with pytest.raises(GcnHostError, match="pca: not with bf16 tables"):
        bf.pca()
    with pytest.raises(GcnHostError, match="pca_transform: not with bf16 tables"):
        bf.pca_transform(fit)
    bf.close()
    fat = HipGCNModel(ds, seed=1, hidden_dim=257)
    with pytest.raises(GcnHostError, match="pca: a hidden width of at most 256, this model has 257"):
        fat.pca()
    with pytest.raises(GcnHostError, match="pca: a hidden width of at most 256 \\(the scatter kernel"):
        _ck(fat.lib, raw(fat), "call")
    fat.close()
    tw = ThreadWorld(2)
    seen, errors = [None, None], []

    def body(rank):
        try:
            ag, ar = tw.callbacks(rank)
            r = HipGCNModel(ds, seed=4, device=0, rank=rank, world=2, host_allgather=ag, host_allreduce=ar, hidden_dim=16, dropout=0.5)
            try:
                r.pca()
                seen[rank] = "no error"
            except GcnHostError as e:
                seen[rank] = str(e)
            r.close()
        except BaseException as e:                                # a failed rank must not leave the other at a barrier forever
            errors.append((rank, e))
            tw.barrier.abort()
    threads = [threading.Thread(target=body, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert all("pca: one rank only" in s for s in seen), seen


# ---- the command line -------------------------------------------------------------------------------------------------------------

def test_cli_pca(tmp_path):
    """gcn-hip cora-syn with GCN_PCA: stdout keeps its lines and gains one; the file's N lines parse to the Python call on the same
    weights (handed over through a weights file, 0 epochs)"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.make_dataset("cora-syn")
    n = ds["num_nodes"]
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "cora-syn.gcnbin"))
    m = HipGCNModel(ds, seed=3, hidden_dim=16, dropout=0.5)
    m.run_epochs(6, want_trace=False)
    w = str(tmp_path / "w.gcnw")
    m.save_weights(w)
    want = m.pca(k=3)
    m.close()
    args = ["cora-syn", "-", "-", "16", "-", "0.5", "-", "-", "0"]
    out = str(tmp_path / "p.txt")
    env = dict(os.environ, GCN_SEED="3", GCN_LOAD_WEIGHTS=w, GCN_PCA=out, GCN_PCA_K="3")
    r = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-2].startswith("test_loss=") and lines[-1].startswith("pca_components=3 ")
    fields = dict(p.split("=") for p in lines[-1].split())
    assert list(fields) == ["pca_components", "pca_rows", "pca_rank", "pca_explained_variance_ratio"]
    assert int(fields["pca_rows"]) == n and int(fields["pca_rank"]) == want["rank"]
    ratios = np.array([float(v) for v in fields["pca_explained_variance_ratio"].split(",")])
    assert ratios.shape == (3,) and np.abs(ratios - want["explained_variance_ratio"][:3]).max() <= 5e-7
    rows = np.loadtxt(out, ndmin=2)
    assert rows.shape == (n, 4) and np.array_equal(rows[:, 0], np.arange(n))
    assert same_bits(rows[:, 1:].astype(np.float32), want["coords"])
    two = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env={k: v for k, v in env.items() if k != "GCN_PCA_K"},
                         capture_output=True, text=True)
    assert two.returncode == 0 and two.stdout.strip().splitlines()[-1].startswith("pca_components=2 "), two.stderr[-500:]
    for extra, msg in ((dict(GCN_GPUS="2"), "GCN_PCA runs on one GPU"), (dict(GCN_PCA_K="17"), "GCN_PCA needs GCN_PCA_K in 1..hidden_dim")):
        bad = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=dict(env, **extra), capture_output=True, text=True)
        assert bad.returncode != 0 and msg in bad.stderr, bad.stderr[-500:]
