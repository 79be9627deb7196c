"""The float64 reference of temperature scaling and the reliability diagram (tests/calib_ref.py) against hand-worked cases, the
host-only calibration_report against numpy, and the argument checks of HipGCNModel.calibrate / calibration / set_temperature
that need no GPU."""
import os
import re
import types

import numpy as np
import pytest

from tests import calib_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def log_softmax(z):
    z = np.asarray(z, np.float64)
    z = z - z.max(axis=1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))


def test_uniform_rows_of_two_classes_sit_at_one_half():
    """conf = 1/2 whatever beta; with B bins it belongs to (b / B, (b + 1) / B] with b = ceil(B / 2) - 1: 10 bins put it into
    bin 4 = (0.4, 0.5] — its upper edge — and 15 bins into bin 7; the tie predicts class 0"""
    logp = np.log(np.full((6, 2), 0.5)).astype(np.float32)
    truth = np.array([0, 1, 0, 1, -1, 2])
    for beta in (0.25, 1.0, 4.0):
        b = R.bins(logp, truth, beta, 10)
        assert b["rows"].tolist() == [0, 1, 2, 3] and np.allclose(b["conf"], 0.5, rtol=0, atol=1e-15)
        assert b["pred"].tolist() == [0] * 4
        assert b["ambiguous"].all()                               # exactly on an edge: either side in f32
        assert b["count"].sum() == 4 and b["count"][4] + b["count"][5] == 4 and b["correct"].sum() == 2
        c = R.bins(logp, truth, beta, 15)
        assert c["count"][7] == 4 and not c["ambiguous"].any() and c["correct"][7] == 2 and abs(c["conf_sum"][7] - 2.0) < 1e-12
        s = R.nll_g_h(logp, truth, beta)
        assert np.allclose(s["nll"], np.log(2.0)) and np.allclose(s["g"], 0, atol=1e-15) and np.allclose(s["h"], 0, atol=1e-15)
        assert s["S"][3] == 4


def test_gradient_and_curvature_against_finite_differences():
    """g = d nll / d beta and h = d2 nll / d beta2 by central differences of the NLL; at beta = 1 on log-softmax rows,
    g = -(l_t - sum_j p_j l_j), minus the residual log-probability; h >= 0 everywhere"""
    rng = np.random.default_rng(0)
    logp = log_softmax(rng.standard_normal((40, 7)) * 3).astype(np.float32)
    truth = rng.integers(0, 7, 40)
    p = np.exp(logp.astype(np.float64))
    one = R.nll_g_h(logp, truth, 1.0)
    resid = logp[np.arange(40), truth] - (p / p.sum(axis=1, keepdims=True) * logp).sum(axis=1)
    assert np.allclose(one["g"], -resid, rtol=0, atol=1e-12)
    assert np.allclose(one["nll"], -logp[np.arange(40), truth] + np.log(p.sum(axis=1)), rtol=0, atol=1e-12)
    for beta in (0.25, 1.0, 4.0):
        d = 1e-5
        lo, mid, hi = (R.nll_g_h(logp, truth, b) for b in (beta - d, beta, beta + d))
        assert np.allclose((hi["nll"] - lo["nll"]) / (2 * d), mid["g"], rtol=0, atol=1e-7)
        assert np.allclose((hi["g"] - lo["g"]) / (2 * d), mid["h"], rtol=0, atol=1e-7)
        assert np.all(mid["h"] >= 0) and mid["h"].max() > 0
        assert np.all(mid["E_nll"] > 0) and np.all(mid["E_nll"] < 1e-4) and np.all(mid["E_g"] < 1e-3) and np.all(mid["E_h"] < 1e-2)
    # a column at -1e4 weighs nothing and gives no NaN; truth outside the classes and ids outside the table are skipped
    logp[3, 2] = -1e4
    s = R.nll_g_h(logp, np.where(np.arange(40) == 5, 7, truth), 0.25, rows=[3, 5, 3, -1, 40, 39])
    assert s["rows"].tolist() == [3, 3, 39] and np.isfinite(s["S"]).all() and np.isfinite(s["E_S"]).all()


def test_fit_recovers_a_planted_temperature():
    """labels drawn from softmax(z / T0): the fit on log_softmax(z) is the maximum-likelihood estimate of beta0 = 1 / T0.  Its
    sampling error is 1 / sqrt(Fisher information) = 1 / sqrt(sum h) at the estimate; five of those is the tolerance"""
    rng = np.random.default_rng(7)
    n, c, t0 = 4000, 10, 2.5
    z = rng.standard_normal((n, c)) * 4
    p = np.exp(log_softmax(z / t0))
    truth = (p.cumsum(axis=1) > rng.random((n, 1))).argmax(axis=1)
    logp = log_softmax(z).astype(np.float32)
    f = R.fit(logp, truth)
    at = R.nll_g_h(logp, truth, f["beta"])
    sigma = 1.0 / np.sqrt(at["S"][2])
    assert sigma < 0.02 and abs(f["beta"] - 1 / t0) <= 5 * sigma, (f["beta"], 1 / t0, sigma)
    assert abs(at["S"][1]) <= 1e-9 * at["S"][2] and not f["at_bound"] and f["nll_after"] < f["nll_before"]
    # the f32-beta iteration the host runs stops within its 1e-6 of the same minimiser
    g = R.newton(lambda b: R.nll_g_h(logp, truth, b)["S"])
    assert abs(g["beta"] - f["beta"]) <= 2e-6 * f["beta"] and g["steps"] <= 12 and g["beta"] == R.f32(g["beta"])
    # a split the model classifies perfectly has no minimum: the iteration ends on the bracket's upper end
    sure = log_softmax(np.eye(c)[truth] * 0.1).astype(np.float32)
    h = R.newton(lambda b: R.nll_g_h(sure, truth, b)["S"])
    assert h["at_bound"] and h["beta"] > 99.99 and h["steps"] <= 40
    flat = R.newton(lambda b: R.nll_g_h(log_softmax(np.eye(c)[truth] * 30).astype(np.float32), truth, b)["S"])
    assert flat["at_bound"] and flat["beta"] > 1                  # the gradient vanishes before the end is reached: reported all the same
    # and one it gets wrong with confidence is pushed to the lower end
    wrong = log_softmax(np.eye(c)[(truth + 1) % c] * 30).astype(np.float32)
    w = R.newton(lambda b: R.nll_g_h(wrong, truth, b)["S"])
    assert w["at_bound"] and w["beta"] < 0.010001


def test_scale_is_the_log_softmax_of_the_scaled_rows():
    rng = np.random.default_rng(2)
    logp = log_softmax(rng.standard_normal((9, 5)) * 2).astype(np.float32)
    out, e_out, prob, e_prob = R.scale(logp, 0.5, rows=[4, 1, 1, 20, -3])
    listed = np.zeros(9, bool)
    listed[[1, 4]] = True
    assert np.isnan(out[~listed]).all() and np.isnan(prob[~listed]).all()
    assert np.allclose(out[listed], log_softmax(0.5 * logp[listed].astype(np.float64)), rtol=0, atol=1e-14)
    assert np.allclose(prob[listed], np.exp(out[listed]).max(axis=1)) and np.all(e_out[listed] < 1e-5) and np.all(e_prob[listed] < 1e-5)
    same, _, _, _ = R.scale(logp, 1.0)
    assert np.allclose(same, logp, rtol=0, atol=1e-7)             # log-softmax rows are a fixed point at beta = 1


def test_calibration_report_against_numpy():
    from cuda_gcn_amd.model import GcnHostError, calibration_report
    rng = np.random.default_rng(1)
    for bins in (1, 15, 64):
        count = rng.integers(0, 50, bins)
        count[rng.random(bins) < 0.4] = 0                         # empty bins
        if bins == 1:
            count[:] = 17
        correct = (count * rng.random(bins)).astype(np.int64)
        conf = count * rng.random(bins)
        got, want = calibration_report(count, correct, conf), R.report(count, correct, conf)
        assert got["rows"] == want["rows"] == count.sum() and np.array_equal(got["count"], count)
        for k in ("accuracy", "confidence"):
            assert np.allclose(got[k], want[k], rtol=0, atol=1e-15) and np.all(got[k][count == 0] == 0)
        assert abs(got["ece"] - want["ece"]) < 1e-14 and abs(got["mce"] - want["mce"]) < 1e-14
    # all rows in one bin: ECE = MCE = that bin's gap
    one = calibration_report([0, 0, 10, 0], [0, 0, 7, 0], [0, 0, 9.0, 0])
    assert abs(one["ece"] - 0.2) < 1e-15 and abs(one["mce"] - 0.2) < 1e-15 and one["accuracy"].tolist() == [0, 0, 0.7, 0]
    none = calibration_report([0, 0], [0, 0], [0.0, 0.0])
    assert none["rows"] == 0 and none["ece"] == 0 and none["mce"] == 0
    for bad in (([1, 2], [0, 3], [0.5, 1.0]), ([-1, 2], [0, 0], [0.0, 0.0]), ([1, 2], [0, 1], [np.nan, 1.0]), ([1, 2], [0], [0.5, 1.0])):
        with pytest.raises(GcnHostError, match="calibration_report"):
            calibration_report(*bad)


def bare_model(num_nodes=10, classes=4, multilabel=False):
    from cuda_gcn_amd.model import HipGCNModel
    m = HipGCNModel.__new__(HipGCNModel)
    m.params = types.SimpleNamespace(num_nodes=num_nodes, output_dim=classes)
    m.multilabel = multilabel
    m.lib = None                                                  # any call into the library would fail loudly
    m.h = None
    return m


def test_model_argument_validation_needs_no_gpu():
    from cuda_gcn_amd.model import GcnHostError
    m = bare_model()
    for bins in (0, 65, -1, 2.5):
        with pytest.raises(GcnHostError, match=r"calibrate: bins must be an integer in 1\.\.64"):
            m.calibrate(bins=bins)
        with pytest.raises(GcnHostError, match=r"calibration: bins must be an integer in 1\.\.64"):
            m.calibration(split=3, bins=bins)
    for t in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(GcnHostError, match="calibration: the temperature must be finite and > 0"):
            m.calibration(split=3, temperature=t)
        with pytest.raises(GcnHostError, match="set_temperature: the temperature must be finite and > 0"):
            m.set_temperature(t)
    with pytest.raises(GcnHostError, match="calibrate: split is 1"):
        m.calibrate(split=0)
    with pytest.raises(GcnHostError, match="calibration: split is 1"):
        m.calibration(split=4)
    with pytest.raises(GcnHostError, match="calibration: give a split or a node query"):
        m.calibration(split=2, nodes=[1])
    for what, call in (("calibrate", lambda x: x.calibrate()), ("calibration", lambda x: x.calibration(split=3)),
                       ("set_temperature", lambda x: x.set_temperature(2.0))):
        with pytest.raises(GcnHostError, match=f"{what}: this is a multi-label model"):
            call(bare_model(multilabel=True))
        with pytest.raises(GcnHostError, match=f"{what}: at most 64 classes"):
            call(bare_model(classes=65))


def test_the_new_symbols_are_declared_and_exported():
    from cuda_gcn_amd import _lib
    drv = open(os.path.join(ROOT, "include", "gcnhip_driver.h")).read()
    surface = open(os.path.join(ROOT, "include", "gcnhip.h")).read()
    hip = _lib.gcnhip()
    for n in ("gcnhip_calib_nll_rows", "gcnhip_calib_bins_rows", "gcnhip_calib_scale_rows"):
        assert re.search(rf"\bint {n}\(", drv) and n not in surface
        assert hasattr(hip, n) and n in _lib.GCNHIP_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "gcnhost.h")).read()
    host = _lib.gcnhost()
    for n in ("gcnhost_model_calibrate", "gcnhost_model_calibration", "gcnhost_model_set_temperature", "gcnhost_model_temperature",
              "gcnhost_calibration_report"):
        assert re.search(rf"\bint {n}\(", hdr)
        assert hasattr(host, n) and n in _lib.GCNHOST_SYMBOLS
