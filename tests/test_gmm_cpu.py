"""What the Gaussian mixture needs without a GPU: the information criteria against scikit-learn, the file of the command line, the
argument checks, the C symbols."""
import ctypes

import numpy as np
import pytest

from cuda_gcn_amd import _lib
from cuda_gcn_amd import model as M


@pytest.mark.parametrize("cov", ["diag", "spherical"])
def test_gmm_information_is_scikit_learns(cov):
    from sklearn.mixture import GaussianMixture
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.normal(c, 0.5, (60, 7)) for c in (-2.0, 0.0, 3.0)])
    g = GaussianMixture(3, covariance_type=cov, random_state=0).fit(x)
    got = M.gmm_information(g.score(x), x.shape[0], 3, 7, cov)
    assert got["n_parameters"] == g._n_parameters()
    assert np.isclose(got["bic"], g.bic(x), rtol=1e-9, atol=0) and np.isclose(got["aic"], g.aic(x), rtol=1e-9, atol=0)


def test_gmm_information_refusals():
    for args in ((np.nan, 10, 2, 3), (-1.0, 0, 2, 3), (-1.0, 10, 0, 3), (-1.0, 10, 2, 0), (-1.0, 10, 2, 3, "full")):
        with pytest.raises(M.GcnHostError):
            M.gmm_information(*args)


@pytest.mark.parametrize("kw", [dict(k=0), dict(k=257), dict(k=2.5), dict(iters=0), dict(iters=None), dict(iters=np.nan), dict(tol="x"), dict(reg_covar=None), dict(tol=-1e-3), dict(tol=np.inf), dict(reg_covar=0.0),
                                dict(reg_covar=np.nan), dict(covariance_type="full"), dict(covariance_type="tied"), dict(init="kmeans++"),
                                dict(init=np.arange(4)), dict(init=np.ones((3, 15), np.float32)), dict(seed=-1)])
def test_gmm_argument_checks(kw):
    """the checks of HipGCNModel.gmm that need no model"""
    args = dict(dict(k=3, iters=10, tol=1e-3, covariance_type="diag", reg_covar=1e-6, init="kmeans", seed=None), **kw)
    with pytest.raises(M.GcnHostError):
        M.HipGCNModel._gmm_args(None, "gmm", dim=16, **args)
    assert M.HipGCNModel._gmm_args(None, "gmm", 3, 10, 0.0, "spherical", 1e-6, np.arange(3), 7, 16)[1] == 1


def test_read_gmm(tmp_path):
    p = tmp_path / "gmm.txt"
    p.write_text("3 0 0.75 -12.5\n\n9 2 1 -3.25\n")
    got = M.read_gmm(str(p))
    assert got["node"].tolist() == [3, 9] and got["component"].tolist() == [0, 2]
    assert got["max_resp"].tolist() == [0.75, 1.0] and got["log_likelihood"].tolist() == [-12.5, -3.25]
    p.write_text("3 -1 0.75 -12.5\n")
    with pytest.raises(M.GcnHostError, match="gmm.txt:1"):
        M.read_gmm(str(p))


def test_c_symbols_are_present():
    hip, host = _lib.gcnhip(), _lib.gcnhost()
    for name in ("gcnhip_gmm_plan", "gcnhip_gmm_estep", "gcnhip_gmm_mstep", "gcnhip_gmm_finalize"):
        assert hasattr(hip, name), name
    for name in ("gcnhost_model_gmm", "gcnhost_model_gmm_score", "gcnhost_gmm_information"):
        assert hasattr(host, name), name
    a, b, c = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.gcnhip_gmm_plan(2100, 41, 128, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0          # no GPU needed
    assert (a.value, b.value, c.value) == (256, 3 * 3 * 17 * 2048, 3 * 17 * 2048)
    assert hip.gcnhip_gmm_plan(10, 257, 16, None, None, None) == -1 and b"k" in hip.gcnhip_last_error()
