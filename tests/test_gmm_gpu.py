"""The Gaussian mixture on the GPU (csrc/gmm.hip, ops.Device.gmm_*, HipGCNModel.gmm / gmm_score) against the float64 reference of
tests/gmm_ref.py: the E-step inside its derived f32 bound, the M-step inside the float64 one, the model against the chained ops calls
byte for byte and against planted blobs."""
import os
import subprocess

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import gmm_ref as R

pytestmark = pytest.mark.gpu
HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cuda_gcn_amd", "bin", "gcn-hip")
F32_ULP = 2.0 ** -23                                       # HIP documents expf to 1 ulp


@pytest.fixture(scope="module")
def dev():
    from cuda_gcn_amd.ops import Device
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def trained():
    from cuda_gcn_amd import model as M
    m = M.HipGCNModel(datagen.make_dataset("cora-syn"), seed=5, hidden_dim=16, dropout=0.5)
    m.run_epochs(5, want_trace=False)
    yield m
    m.close()


def case(n, k, dim, seed=0):
    """overlapping components, so that responsibilities are soft: a table with spare rows, a list with a repeat and (n > 1) one row
    outside the table, inverse norms for every other n, one component without weight when k >= 3"""
    rng = np.random.default_rng(1000 * n + 10 * k + dim + seed)
    mu = (0.5 * rng.standard_normal((k, dim))).astype(np.float32)
    var = rng.uniform(0.5, 1.5, (k, dim)).astype(np.float32)
    w = rng.uniform(0.5, 1.5, k)
    if k >= 3:
        w[k // 2] = 0.0
    n_table = n + 3
    table = (mu[rng.integers(0, k, n_table)] + rng.standard_normal((n_table, dim)) * np.sqrt(var.mean())).astype(np.float32)
    rows = rng.integers(0, n_table, n).astype(np.int32)
    if n > 1:
        rows[n // 2], rows[-1] = n_table, rows[0]
    inv = rng.uniform(0.5, 2.0, n_table).astype(np.float32) if n % 2 else None
    ok = rows < n_table
    xs = R.shifted(table[np.minimum(rows, n_table - 1)], None if inv is None else inv[np.minimum(rows, n_table - 1)], 0)
    shift = xs[ok].astype(np.float64).mean(0).astype(np.float32)
    xp = R.shifted(table[np.minimum(rows, n_table - 1)], None if inv is None else inv[np.minimum(rows, n_table - 1)], shift)
    prec, mprec, cst = R.operands(mu - shift, var, (w / w.sum()).astype(np.float32))
    return dict(table=table, rows=rows, inv=inv, shift=shift, xp=xp, ok=ok, prec=prec, mprec=mprec, cst=cst, k=k, dim=dim, n=n)


def estep(dev, c, **kw):
    """the table with a row stride of dim + 5; at dim 17 and 130 the operands with one of dim + 3 (20: vector loads, 133: scalar)"""
    ldc = c["dim"] + 3 if c["dim"] in (17, 130) else None
    return dev.gmm_estep(c["table"], c["shift"], c["prec"], c["mprec"], c["cst"], rows=c["rows"], inv_norm=c["inv"], ld=c["dim"] + 5, ldc=ldc, **kw)


@pytest.mark.parametrize("dim", [1, 15, 16, 17, 128, 130, 256])
@pytest.mark.parametrize("k", [1, 3, 64, 65, 130])
def test_estep_holds_the_f32_bound(dev, k, dim):
    for n in (1, 63, 65, 200):
        c = case(n, k, dim)
        got, ok = estep(dev, c), c["ok"]
        lj64, err, lse64 = R.estep64(c["xp"], c["prec"], c["mprec"], c["cst"])
        fin = np.isfinite(lj64)
        assert np.all(np.abs(got["lj"][ok] - lj64[ok])[fin[ok]] <= err[ok][fin[ok]]) and np.all(got["lj"][ok][~fin[ok]] == -np.inf), (n, k, dim)
        e_row = np.where(fin, err, 0.0).max(1)
        assert np.all(np.abs(got["lse"][ok] - lse64[ok]) <= (e_row + (k + 2) * R.U)[ok]), (n, k, dim)
        top = np.sort(lj64, 1)[:, ::-1]
        clear = ok & ((top[:, 0] - top[:, 1] > 2 * e_row) if k > 1 else True)
        assert np.array_equal(got["assign"][clear], lj64.argmax(1)[clear]) and clear.sum() >= ok.sum() // 2
        assert np.all(np.isnan(got["lj"][~ok])) and np.all(np.isnan(got["lse"][~ok])) and np.all(got["assign"][~ok] == -1)
        assert np.all(np.abs(got["max_resp"][ok] - np.exp(got["lj"][ok].max(1) - got["lse"][ok])) <= 4 * R.U)
        again = estep(dev, c)
        assert all(got[key].tobytes() == again[key].tobytes() for key in ("lj", "lse", "assign", "max_resp"))
        assert got["lse_sum"] == R.tree_sum(got["lse"]) == again["lse_sum"]
        assert estep(dev, c, want_lj=False)["lse"].tobytes() == got["lse"].tobytes()


MSTEP_CASES = [(1, 1, 1), (63, 3, 15), (65, 64, 16), (200, 65, 17), (200, 130, 128), (65, 3, 130), (63, 5, 256), (1023, 3, 17), (1025, 65, 16),
               (2100, 5, 130)]


@pytest.mark.parametrize("n,k,dim", MSTEP_CASES)
def test_mstep_holds_the_f64_bound(dev, n, k, dim):
    """on the GPU's own lj and lse: the sums against float64 sums with r = the exact exponential of the f32 argument lj - lse, one f32
    ulp of every r allowed for expf (DESIGN 4.30 has the reason); every scratch size gives the same bytes; the indicator form counts
    exactly"""
    c = case(n, k, dim, seed=1)
    e, ok = estep(dev, c), c["ok"]
    kw = dict(rows=c["rows"], inv_norm=c["inv"], ld=dim + 5)
    got = dev.gmm_mstep(c["table"], c["shift"], k, lj=e["lj"], lse=e["lse"], **kw)
    with np.errstate(invalid="ignore"):
        r = np.where(ok[:, None], np.exp((e["lj"] - e["lse"][:, None]).astype(np.float64)), 0)
    want, mass = R.sums64(np.where(ok[:, None], c["xp"], 0), r)
    assert np.all(np.abs(got - want) <= (n * 2.0 ** -53 + F32_ULP) * mass), (n, k, dim)
    plan = dev.gmm_plan(n, k, dim)
    for sbytes in (plan["mstep_bytes_min"], (plan["mstep_bytes_min"] + plan["mstep_bytes"]) // 2):
        assert dev.gmm_mstep(c["table"], c["shift"], k, lj=e["lj"], lse=e["lse"], scratch_bytes=sbytes, **kw).tobytes() == got.tobytes()
    hard = dev.gmm_mstep(c["table"], c["shift"], k, assign=e["assign"], **kw)
    one = (e["assign"][:, None] == np.arange(k)[None]) & ok[:, None]
    want, mass = R.sums64(np.where(ok[:, None], c["xp"], 0), one)
    assert np.array_equal(hard[:, 0], one.sum(0)) and np.all(np.abs(hard - want) <= n * 2.0 ** -53 * mass)


@pytest.mark.parametrize("spherical", [False, True])
def test_finalize(dev, spherical):
    """variances stay above reg_covar, an empty component keeps its operands and loses its weight, spherical rows are constant"""
    c = case(200, 5, 17, seed=2)
    a = estep(dev, c)["assign"]
    a[a == 3] = 0                                           # component 3 has no member
    sums = dev.gmm_mstep(c["table"], c["shift"], 5, assign=a, rows=c["rows"], inv_norm=c["inv"])
    sums[1, 18:] = sums[1, 1:18] ** 2 / sums[1, 0]          # component 1 has no variance of its own
    start = dev.gmm_finalize(None, 200, np.full((5, 17), 0.25, np.float32), np.ones((5, 17), np.float32), np.zeros(5, np.float32))
    got = dev.gmm_finalize(sums, 200, start["mu"], start["var"], start["weights"], start["prec"], start["mprec"], start["cst"], spherical, 1e-3)
    assert all(np.all(np.isfinite(got[key])) for key in ("mu", "var", "prec", "mprec", "weights")) and not np.any(np.isnan(got["cst"]))
    assert np.all(got["var"] >= np.float32(1e-3)) and np.all(got["var"][1] <= np.float32(1.1e-3))
    fit = np.array([True, True, False, False, True])        # component 2 has no weight in `case`, so no member either
    assert np.all(got["cst"][~fit] == -np.inf) and np.all(got["weights"][~fit] == 0) and np.isclose(got["weights"].sum(), 1, atol=1e-6)
    assert all(got[key][~fit].tobytes() == start[key][~fit].tobytes() for key in ("mu", "var", "prec", "mprec"))
    assert np.all(got["var"] == got["var"][:, :1]) == spherical
    p, q, cst = R.operands(got["mu"][fit], got["var"][fit], got["weights"][fit])
    assert np.allclose(got["prec"][fit], p, rtol=1e-6) and np.allclose(got["cst"][fit], cst, rtol=1e-5, atol=1e-5)


def chained(dev, x, means0, iters, reg_covar):
    """gmm()'s launches one by one"""
    n, k = x.shape[0], means0.shape[0]
    shift = dev.pca_mean(x)[0].astype(np.float32)
    cn = dev.kmeans_update(x, np.zeros(0, np.int32), means0, rows=np.zeros(0, np.int32))["cn"]
    hard = dev.kmeans_assign(x, means0, cn)[0]
    p = dev.gmm_finalize(None, n, means0 - shift, np.ones_like(means0), np.zeros(k, np.float32))
    for it in range(iters + 1):
        e = dev.gmm_estep(x, shift, p["prec"], p["mprec"], p["cst"]) if it else None
        sums = dev.gmm_mstep(x, shift, k, lj=e["lj"], lse=e["lse"]) if it else dev.gmm_mstep(x, shift, k, assign=hard)
        p = dev.gmm_finalize(sums, n, p["mu"], p["var"], p["weights"], p["prec"], p["mprec"], p["cst"], False, reg_covar)
    means = p["mu"] + shift
    q = dev.gmm_finalize(None, n, means - shift, p["var"], p["weights"])
    return dict(dev.gmm_estep(x, shift, q["prec"], q["mprec"], q["cst"]), means=means, variances=p["var"], weights=p["weights"],
                lower_bound=e["lse_sum"] / n)


@pytest.mark.parametrize("n,k,d", [(200, 3, 17), (520, 5, 130), (1100, 65, 16)])
def test_model_fits_planted_blobs(dev, trained, n, k, d):
    """gmm(data=) is the chained ops calls byte for byte, under every scratch cap; its labels are the float64 reference's (which are
    the planted ones), its lower bound lies within the E-step bound of the reference's"""
    from cuda_gcn_amd import model as M
    rng = np.random.default_rng(7)
    centres, label = rng.normal(size=(k, d)) * 4, np.arange(n) % k
    x = (centres[label] + rng.normal(size=(n, d)) * (0.3 + 0.2 * rng.random((k, d)))[label]).astype(np.float32)
    kw = dict(data=x, normalize=False, init=x[:k].copy(), iters=5, tol=0, report=False)
    fit, want = trained.gmm(k, **kw), chained(dev, x, x[:k].copy(), 5, 1e-6)
    small = trained.gmm(k, scratch_bytes=1, **kw)
    for key, ref in (("weights", "weights"), ("means", "means"), ("variances", "variances"), ("log_likelihood", "lse"), ("assign", "assign"),
                     ("max_resp", "max_resp")):
        assert fit[key].tobytes() == want[ref].tobytes() == small[key].tobytes(), key
    assert fit["lower_bound"] == want["lower_bound"] == small["lower_bound"] and fit["iters_run"] == 5 and not fit["converged"]
    labels, bounds, (mu, var, w) = R.fit64(x, x[:k], 5)
    assert np.array_equal(labels, label) and np.array_equal(fit["assign"], labels)
    sh = x.astype(np.float64).mean(0).astype(np.float32)
    err = R.estep64(R.shifted(x, None, sh), *R.operands(mu - sh, var, w))[1]
    bound = float((err.max(1) + (k + 2) * R.U).mean())
    assert abs(fit["lower_bound"] - bounds[-1]) <= bound and np.all(np.diff(fit["history"][:, 1]) >= -2 * bound)
    info = M.gmm_information(fit["lower_bound"], n, k, d, "diag")
    assert all(fit[key] == info[key] for key in ("n_parameters", "bic", "aic"))
    r = trained.gmm(k, resp=True, **kw)["resp"]
    assert np.allclose(r.sum(1), 1, atol=1e-5) and np.array_equal(r.argmax(1), labels)


def test_model_on_embeddings(trained):
    """the trained model's own rows: a fit of the test split, its score repeated bit for bit, the report, the refusals"""
    from cuda_gcn_amd import model as M
    before = [trained.var(v).tobytes() for v in (2, 5)]
    fit = trained.gmm(k=4, split=3, seed=3)
    n = fit["points"]
    assert n > 0 and fit["assign"].shape == (n,) and np.isfinite(fit["lower_bound"]) and fit["contingency"].sum() + fit["skipped"] == n
    assert trained.gmm_score(fit, split=3)["log_likelihood"].tobytes() == fit["log_likelihood"].tobytes()
    assert trained.gmm(k=4, split=3, seed=3)["log_likelihood"].tobytes() == fit["log_likelihood"].tobytes()
    sph = trained.gmm(k=2, nodes=np.arange(100), covariance_type="spherical", init=np.array([0, 50]))
    assert np.all(sph["variances"] == sph["variances"][:, :1]) and sph["n_parameters"] == 2 * 16 + 3
    assert np.all(np.isfinite(trained.gmm_score(sph, nodes=[5, 5, 7])["log_likelihood"]))
    assert [trained.var(v).tobytes() for v in (2, 5)] == before
    for kw, word in ((dict(k=0), "1..256"), (dict(k=4, nodes=[1, 2]), "above the 2 rows"), (dict(k=2, iters=0), "iters"), (dict(k=2, tol=-1), "tol"),
                     (dict(k=2, tol=np.nan), "tol"), (dict(k=2, reg_covar=0), "reg_covar"), (dict(k=2, split=4), "split"),
                     (dict(k=2, nodes=[10 ** 6, 1]), "node"), (dict(k=2, init="random"), "init"), (dict(k=2, init=np.array([0, 10 ** 6])), "position"),
                     (dict(k=2, covariance_type="full"), "covariance_type"), (dict(k=2, data=np.ones((4, 257), np.float32)), "256")):
        with pytest.raises(M.GcnHostError, match=word):
            trained.gmm(**kw)
    bf = M.HipGCNModel(datagen.make_dataset("cora-syn"), seed=1, flags=M.BF16_TABLES, hidden_dim=16)
    with pytest.raises(M.GcnHostError, match="bf16"):
        bf.gmm(k=2)
    bf.close()


def test_cli_gmm(tmp_path):
    """GCN_GMM prints the six keys of m.gmm on the test split and writes the file read_gmm parses to the same per-node numbers"""
    from cuda_gcn_amd.model import HipGCNModel, read_gmm
    ds = datagen.make_dataset("cora-syn")
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "cora-syn.gcnbin"))
    m = HipGCNModel(ds, seed=3, hidden_dim=16, dropout=0.5)
    m.run_epochs(6, want_trace=False)
    w, out = str(tmp_path / "w.gcnw"), str(tmp_path / "g.txt")
    m.save_weights(w)
    want = m.gmm(k=3, split=3, iters=7, covariance_type="spherical")
    m.close()
    args = ["timeout", "-k", "10", "50", HIP, "cora-syn", "-", "-", "16", "-", "0.5", "-", "-", "0"]
    env = dict(os.environ, GCN_SEED="3", GCN_LOAD_WEIGHTS=w, GCN_GMM=out, GCN_GMM_K="3", GCN_GMM_ITERS="7", GCN_GMM_COV="spherical")
    r = subprocess.run(args, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-1000:]
    fields = dict(p.split("=") for p in r.stdout.strip().splitlines()[-1].split())
    assert list(fields) == ["gmm_components", "gmm_iters", "gmm_converged", "gmm_lower_bound", "gmm_bic", "gmm_aic"]
    assert [float(v) for v in fields.values()] == [3, want["iters_run"], want["converged"], want["lower_bound"], want["bic"], want["aic"]]
    got = read_gmm(out)
    assert np.array_equal(got["node"], np.flatnonzero(np.asarray(ds["split"]) == 3)) and np.array_equal(got["component"], want["assign"])
    assert all(np.array_equal(got[key].astype(np.float32), want[key]) for key in ("max_resp", "log_likelihood"))   # %.9g: f32 exactly
    bad = subprocess.run(args, cwd=str(tmp_path), env=dict(env, GCN_GMM_COV="full"), capture_output=True, text=True)
    assert bad.returncode != 0 and "GCN_GMM needs GCN_GMM_COV" in bad.stderr
