"""Temperature scaling and calibration error on the GPU: the three kernels of csrc/calib.hip against the float64 reference of
tests/calib_ref.py within its carried bounds, the model's calibrate / calibration / set_temperature against the reference on
the model's own log-softmax rows, no side effects on training or on the T = 1 paths, refusals, and the command line
(GCN_CALIBRATE)."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import calib_ref as R
from tests import smooth_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")
SENTINEL = -7.5
BETAS = (0.25, 1.0, 4.0)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def log_softmax32(z):
    z = np.asarray(z, np.float64)
    z = z - z.max(axis=1, keepdims=True)
    return (z - np.log(np.exp(z).sum(axis=1, keepdims=True))).astype(np.float32)


def make_case(n, c, seed):
    """log-softmax rows with, from 5 rows on: a column at -1e4 (row 3), an exact tie for the maximum (row 4), truth -1 (row 1)
    and >= C (row 2)"""
    rng = np.random.default_rng(seed)
    logp = log_softmax32(rng.standard_normal((n, c)) * 2)
    truth = rng.integers(0, c, n).astype(np.int32)
    if n >= 5:
        truth[1], truth[2] = -1, c + 3
        logp[3, 1] = -1e4
        logp[4, 0] = logp[4, c - 1] = logp[4].max()
        truth[4] = 0
    return logp, truth


@pytest.fixture(scope="module")
def dev():
    from cuda_gcn_amd.ops import Device
    d = Device(0)
    yield d
    d.close()


def check_kernels(dev, logp, truth, rows, ld, beta, bins):
    n = logp.shape[0]
    listed = n if rows is None else len(rows)
    # nll, g, h
    want = R.nll_g_h(logp, truth, beta, rows)
    got = dev.calib_nll_rows(logp, truth, beta, rows, ld)
    assert got[3] == want["S"][3]
    assert np.all(np.abs(got[:3] - want["S"][:3]) <= want["E_S"]), (got, want["S"], want["E_S"])
    assert got[2] >= 0 and np.isfinite(got).all()
    assert same_bits(got, dev.calib_nll_rows(logp, truth, beta, rows, ld))
    # bins: the ambiguous rows are at most 1 % of the listed ones (a condition on the inputs, met by the reference alone)
    b = R.bins(logp, truth, beta, bins, rows)
    assert b["ambiguous"].sum() <= 0.01 * max(listed, 1), (int(b["ambiguous"].sum()), listed)
    count, correct, conf = dev.calib_bins_rows(logp, truth, beta, bins, rows, ld)
    assert count.sum() == want["S"][3]
    assert np.all(np.abs(count - b["count"]) <= b["amb_near"]) and np.all(np.abs(correct - b["correct"]) <= b["amb_near"])
    assert np.all(np.abs(conf - b["conf_sum"]) <= b["amb_near"] + b["E_conf"].sum() * (1 + 1e-9))
    again = dev.calib_bins_rows(logp, truth, beta, bins, rows, ld)
    assert all(same_bits(x, y) for x, y in zip((count, correct, conf), again))
    # scale: listed rows inside the table, whatever their truth; the rest and the padding untouched
    out, e_out, prob, e_prob = R.scale(logp, beta, rows)
    c = logp.shape[1]
    o, p = dev.calib_scale_rows(logp, beta, rows, ld, ld_out=c + 3, fill=SENTINEL)
    done = ~np.isnan(prob)
    assert np.all(o[~done] == SENTINEL) and np.all(o[:, c:] == SENTINEL) and np.all(p[~done] == SENTINEL)
    assert np.all(np.abs(o[done][:, :c].astype(np.float64) - out[done]) <= e_out[done])
    assert np.all(np.abs(p[done].astype(np.float64) - prob[done]) <= e_prob[done])
    o2, p2 = dev.calib_scale_rows(logp, beta, rows, ld, ld_out=c + 3, fill=SENTINEL)
    assert same_bits(o, o2) and same_bits(p, p2)
    if rows is None or len(set(rows)) == len(rows):              # in place: every row once
        q, pq = dev.calib_scale_rows(logp, beta, rows, ld, in_place=True, fill=SENTINEL)
        assert same_bits(q[done][:, :c], o[done][:, :c]) and same_bits(pq, p)
        if n:
            keep = dev.padded(logp, ld or c).download()
            assert same_bits(q[~done][:, :c], keep[~done][:, :c])


@pytest.mark.parametrize("c", [2, 41, 64])
def test_kernels_match_the_reference_on_small_shapes(dev, c):
    """n in {0, 1, 5, 17}, ld == C and > C, beta in {0.25, 1, 4}, bins 1 / 15 / 63 (64 runs past the block cap); a column at -1e4, a tie, truth -1 and >= C"""
    for n in (0, 1, 5, 17):
        logp, truth = make_case(n, c, 100 * c + n)
        for ld in (None, c + 5):
            for beta, bins in zip(BETAS, (15, 63, 1)):            # (the tie of two classes sits at 1/2: no even bin count)
                check_kernels(dev, logp, truth, None, ld, beta, bins)
    logp, truth = make_case(17, c, 7)
    rows = [16, 3, 3, -1, 17, 0, 4, 99, 2, 1, 3]                  # repeated, unsorted, outside the table
    for beta in BETAS:
        check_kernels(dev, logp, truth, rows, c + 1, beta, 9)
    check_kernels(dev, logp, truth, [9, 4, 16, 0, 3], None, 0.25, 15)           # distinct: also in place
    # the tie predicts the lowest column, and a row list may be empty
    assert R.bins(logp, truth, 1.0, 15, [4])["pred"].tolist() == [0]
    _, correct, _ = dev.calib_bins_rows(logp, truth, 1.0, 15, [4])
    assert correct.sum() == 1
    assert dev.calib_nll_rows(logp, truth, 1.0, np.zeros(0, np.int32)).tolist() == [0, 0, 0, 0]


def test_kernels_past_the_block_cap(dev):
    """20 011 rows of 41 floats: more than 256 blocks x 64 rows, so the cap and the grid-stride loop both run"""
    logp, truth = make_case(20011, 41, 3)
    check_kernels(dev, logp, truth, None, 48, 1.0, 15)
    rows = np.random.default_rng(0).integers(-5, 20020, 18000)
    check_kernels(dev, logp, truth, rows.tolist(), None, 0.25, 64)


def test_bins_match_exactly_far_from_every_edge(dev):
    """two classes with p = (q, 1 - q): conf = q exactly known, chosen in the middle of a bin of 10"""
    q = np.array([0.55, 0.65, 0.75, 0.85, 0.95, 0.55, 0.95, 0.75])
    logp = np.log(np.stack([q, 1 - q], axis=1)).astype(np.float32)
    truth = np.array([0, 1, 0, 0, 0, 1, 0, -1], np.int32)
    b = R.bins(logp, truth, 1.0, 10)
    assert not b["ambiguous"].any() and b["count"].tolist() == [0, 0, 0, 0, 0, 2, 1, 1, 1, 2] and b["correct"].tolist() == [0] * 5 + [1, 0, 1, 1, 2]
    count, correct, conf = dev.calib_bins_rows(logp, truth, 1.0, 10)
    assert np.array_equal(count, b["count"]) and np.array_equal(correct, b["correct"])
    assert np.all(np.abs(conf - b["conf_sum"]) <= 4 * b["E_conf"].max())


def test_kernel_refusals(dev):
    from cuda_gcn_amd.ops import GcnHipError
    logp, truth = make_case(5, 3, 0)
    for beta in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(GcnHipError, match="gcnhip_calib_nll_rows: beta must be finite and > 0"):
            dev.calib_nll_rows(logp, truth, beta)
        with pytest.raises(GcnHipError, match="gcnhip_calib_scale_rows: beta must be finite and > 0"):
            dev.calib_scale_rows(logp, beta)
    for bins in (0, 65):
        with pytest.raises(GcnHipError, match="gcnhip_calib_bins_rows: 1 <= bins <= 64"):
            dev.calib_bins_rows(logp, truth, 1.0, bins)
    with pytest.raises(GcnHipError, match="gcnhip_calib_scale_rows: a row stride is below num_classes"):
        dev.calib_scale_rows(logp, 1.0, ld_out=2)
    with pytest.raises(GcnHipError, match="gcnhip_calib_nll_rows: without a row list n is at most n_table"):
        dev.calib_nll_rows(logp, truth, 1.0, n=6)
    wide = np.zeros((2, 65), np.float32)
    with pytest.raises(GcnHipError, match="gcnhip_calib_scale_rows: 1 <= num_classes <= 64"):
        dev.calib_scale_rows(wide, 1.0)


# ---- the model ----------------------------------------------------------------------------------------------------------

def trained(name, epochs=10, **kw):
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.make_dataset(name) if isinstance(name, str) else name
    m = HipGCNModel(ds, seed=5, hidden_dim=16, **dict(dict(dropout=0.5), **kw))
    m.run_epochs(epochs, want_trace=False)
    return ds, m


def check_calibration(got, logp, label, rows, t, bins=15):
    beta = R.f32(np.float32(1.0) / np.float32(t))
    want = R.nll_g_h(logp, label, beta, rows)
    b = R.bins(logp, label, beta, bins, rows)
    assert got["rows"] == want["S"][3] and np.all(np.abs(got["sums"][:3] - want["S"][:3]) <= want["E_S"])
    assert abs(got["nll"] - want["S"][0] / want["S"][3]) <= want["E_S"][0] / want["S"][3]
    assert np.all(np.abs(got["count"] - b["count"]) <= b["amb_near"])
    ref = R.report(b["count"], b["correct"], b["conf_sum"])
    assert abs(got["ece"] - ref["ece"]) <= R.ece_bound(b, bins), (got["ece"], ref["ece"], R.ece_bound(b, bins))
    if not b["ambiguous"].any():
        assert np.allclose(got["accuracy"], ref["accuracy"], rtol=0, atol=1e-15)
        assert np.all(np.abs(got["confidence"] - ref["confidence"]) <= b["E_conf"].max() * (1 + 1e-9))
        assert abs(got["mce"] - ref["mce"]) <= b["E_conf"].max() * (1 + 1e-9)
    return ref


@pytest.mark.parametrize("name", ["cora-syn", "tiny-syn"])
def test_model_calibration_and_fit_match_the_reference(name):
    """calibration(split) at T = 1 and T = 2 and of a node query, calibrate(), and predict / correct_and_smooth under a set
    temperature, against the reference on the log-softmax rows predict(logp=True) returns at T = 1"""
    ds, m = trained(name)
    n, c = ds["num_nodes"], ds["output_dim"]
    pred1, prob1, logp = m.predict(logp=True)
    cs1, g1 = m.correct_and_smooth(iters_correct=5, iters_smooth=5)
    assert m.temperature == 1.0
    for split in (2, 3):
        rows = np.flatnonzero(ds["split"] == split)
        for t in (1.0, 2.0):
            check_calibration(m.calibration(split=split, temperature=t), logp, ds["label"], rows, t)
    q = [5, 3, 3, n - 1, 0]
    check_calibration(m.calibration(nodes=q, temperature=0.5, bins=7), logp, ds["label"], q, 0.5, bins=7)
    # the fit
    val = np.flatnonzero(ds["split"] == 2)
    fit = m.calibrate(apply=False)
    ref = R.fit(logp, ds["label"], val)
    at = R.nll_g_h(logp, ds["label"], ref["beta"], val)
    beta = 1.0 / fit["temperature"]
    assert abs(beta - ref["beta"]) <= at["E_S"][1] / at["S"][2] + 2e-6 * ref["beta"], (beta, ref["beta"], at["E_S"][1] / at["S"][2])
    e_nll = R.nll_g_h(logp, ds["label"], 1.0, val)["E_S"][0] / val.size
    assert fit["nll_after"] <= fit["nll_before"] + 2 * e_nll and abs(fit["nll_before"] - ref["nll_before"]) <= e_nll
    assert fit["steps"] <= 40 and not fit["at_bound"] and fit["rows"] == val.size and m.temperature == 1.0
    # predict and correct_and_smooth at T = 1 after those calls: the bits of before, and nothing of calib.hip runs
    pred, prob, lp = m.predict(logp=True)
    assert np.array_equal(pred, pred1) and same_bits(prob, prob1) and same_bits(lp, logp)
    cs, g = m.correct_and_smooth(iters_correct=5, iters_smooth=5)
    assert np.array_equal(cs, cs1) and same_bits(g, g1)
    # a set temperature
    logq1 = m.predict(nodes=q, logp=True)[2]
    t = 2.0
    m.set_temperature(t)
    assert m.temperature == t
    beta = R.f32(np.float32(1.0) / np.float32(t))
    out, e_out, prob_ref, e_prob = R.scale(logp, beta)
    pred, prob, lp = m.predict(logp=True)
    assert np.array_equal(pred, pred1)
    assert np.all(np.abs(lp.astype(np.float64) - out) <= e_out) and np.all(np.abs(prob.astype(np.float64) - prob_ref) <= e_prob)
    pq, probq, lq = m.predict(nodes=q, logp=True)                # a query that repeats a node: scaled once
    oq, e_oq, prob_q, e_prob_q = R.scale(logq1, beta)
    assert np.array_equal(pq, pred1[q])
    assert np.all(np.abs(lq.astype(np.float64) - oq) <= e_oq) and np.all(np.abs(probq.astype(np.float64) - prob_q) <= e_prob_q)
    assert same_bits(m.predict()[1], prob)                        # without logp the rows are kept all the same
    own = m.calibration(split=3)                                  # temperature=None: the model's own
    assert own["temperature"] == t and same_bits(own["sums"], m.calibration(split=3, temperature=t)["sums"])
    # Correct & Smooth starts from the calibrated softmax: smooth_ref's scheme from the rows predict() now returns; their
    # entrywise error e_out enters its first stage where EXP_ATOL alone does at T = 1
    csr = (ds["g_indptr"], ds["g_indices"], S.edge_coef(ds["g_indptr"], ds["g_indices"]))
    truth = np.where(ds["split"] == 1, ds["label"], -1)
    a = float(np.float32(0.8))
    cs, g = m.correct_and_smooth(iters_correct=5, iters_smooth=5)
    want = S.correct_and_smooth(csr, lp, truth, a, 5, a, 5)
    assert np.all(np.abs(g.astype(np.float64) - want["G"]) <= want["B_G"]), float((np.abs(g - want["G"]) - want["B_G"]).max())
    assert not same_bits(g, g1)
    m.set_temperature(1.0)
    assert same_bits(m.predict()[1], prob1)
    m.close()


def test_a_perfectly_classified_split_reports_at_bound():
    """the validation labels replaced by the model's own predictions: the NLL falls in beta without end"""
    from cuda_gcn_amd.model import HipGCNModel
    ds, m = trained("tiny-syn")
    pred, _ = m.predict()
    w1, w2 = m.var(2), m.var(5)
    m.close()
    sure = dict(ds, label=np.where(ds["split"] == 2, pred, ds["label"]).astype(np.int32))
    m2 = HipGCNModel(sure, seed=5, hidden_dim=16, dropout=0.5)
    m2.set_weights(w1, w2)
    fit = m2.calibrate()
    assert fit["at_bound"] and fit["temperature"] < 1 and fit["nll_after"] < fit["nll_before"] and fit["steps"] <= 40
    assert m2.temperature == pytest.approx(fit["temperature"])    # apply=True
    m2.close()


def test_a_reset_temperature_restores_every_bit():
    """predict at T = 1 after a temperature was set and reset has the bits of before; in between only pred is the same"""
    ds, m = trained("tiny-syn", epochs=3)
    before = m.predict(logp=True)
    m.set_temperature(3.0)
    mid = m.predict(logp=True)
    m.set_temperature(1.0)
    after = m.predict(logp=True)
    assert all(same_bits(x, y) for x, y in zip(before, after))
    assert np.array_equal(before[0], mid[0]) and not same_bits(before[2], mid[2])
    m.close()


@pytest.mark.parametrize("flags", ["0", "EVAL_LANE", "NO_GRAPH"])
def test_calibration_between_epochs_changes_nothing(flags):
    """two models with the same seed train in lockstep, one calling calibrate and calibration between epochs (and predicting under
    the fitted temperature): traces, weights, test metrics and the logits of the last forward are bit-identical"""
    from cuda_gcn_amd import model as M
    f = getattr(M, flags) if flags != "0" else 0
    ds = datagen.make_dataset("cora-syn")
    a = M.HipGCNModel(ds, seed=6, flags=f, hidden_dim=16, dropout=0.5)
    b = M.HipGCNModel(ds, seed=6, flags=f, hidden_dim=16, dropout=0.5)
    ta, tb = [], []
    for e in range(4):
        ta.append(a.run_epochs(1))
        tb.append(b.run_epochs(1))
        b.calibrate()
        b.calibration(split=3)
        b.calibration(nodes=[1, 2, 3], temperature=1.5)
        b.predict(nodes=[4, 4, 9])
    ta.append(np.array([a.train_epoch() + a.eval(2)], np.float32))
    tb.append(np.array([b.train_epoch() + b.eval(2)], np.float32))
    ta, tb = np.concatenate(ta), np.concatenate(tb)
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32)), (ta, tb)
    for k in (2, 5):
        assert same_bits(a.var(k), b.var(k)), k
    assert a.eval(3) == b.eval(3)
    assert same_bits(a.var(6), b.var(6))
    assert a.evaluate(split=3)["accuracy"] == b.evaluate(split=3)["accuracy"]          # evaluate ignores the temperature
    a.close()
    b.close()


def test_refusals():
    """a multi-label model, 65 classes, two ranks, bins 0 and 65, T <= 0: GcnHostError naming the method, from the Python front
    end and from the C entry points called directly"""
    from cuda_gcn_amd.model import HipGCNModel, GcnHostError, _ck
    from tests.mr_threads import ThreadWorld
    ds = datagen.make_dataset("tiny-syn")
    n = ds["num_nodes"]
    out6, sums = np.zeros(6), np.zeros(4)
    cnt, cor, conf = np.zeros(128, np.int64), np.zeros(128, np.int64), np.zeros(128)

    def direct(m, bins=15, t=1.0):
        return (lambda: m.lib.gcnhost_model_calibrate(m.h, 2, bins, out6.ctypes.data, cnt.ctypes.data, cor.ctypes.data, conf.ctypes.data),
                lambda: m.lib.gcnhost_model_calibration(m.h, 3, None, 0, t, bins, sums.ctypes.data, cnt.ctypes.data, cor.ctypes.data, conf.ctypes.data))
    y = np.random.default_rng(0).random((n, ds["output_dim"])) < 0.3
    ml = HipGCNModel(ds, seed=1, hidden_dim=16, multilabel=y)
    wide = HipGCNModel(dict(ds, output_dim=65, label=(np.arange(n) % 65).astype(np.int32)), seed=1, hidden_dim=16)
    for m, msg in ((ml, "this is a multi-label model"), (wide, "at most 64 classes")):
        for what, call in (("calibrate", m.calibrate), ("calibration", lambda: m.calibration(split=3)), ("set_temperature", lambda: m.set_temperature(2.0))):
            with pytest.raises(GcnHostError, match=f"{what}: {msg}"):
                call()
        for what, call in zip(("calibrate", "calibration"), direct(m)):
            with pytest.raises(GcnHostError, match=f"{what}: {msg}"):
                _ck(m.lib, call(), "call")
        with pytest.raises(GcnHostError, match=f"set_temperature: {msg}"):
            _ck(m.lib, m.lib.gcnhost_model_set_temperature(m.h, 2.0), "call")
        m.close()
    m = HipGCNModel(ds, seed=1, hidden_dim=16)
    for bins in (0, 65):
        with pytest.raises(GcnHostError, match="calibration: bins must be"):
            m.calibration(split=3, bins=bins)
        with pytest.raises(GcnHostError, match=r"calibration: bins must be in 1\.\.64"):
            _ck(m.lib, direct(m, bins=bins)[1](), "call")
    with pytest.raises(GcnHostError, match=r"calibrate: bins must be in 1\.\.64"):
        _ck(m.lib, direct(m, bins=65)[0](), "call")
    for t in (0.0, -2.0, float("nan")):
        with pytest.raises(GcnHostError, match="calibration: the temperature must be finite and > 0"):
            _ck(m.lib, direct(m, t=t)[1](), "call")
        with pytest.raises(GcnHostError, match="set_temperature: the temperature must be finite and > 0"):
            _ck(m.lib, m.lib.gcnhost_model_set_temperature(m.h, t), "call")
    m.close()
    # a split without labelled rows
    empty = HipGCNModel(dict(ds, split=np.where(ds["split"] == 2, 3, ds["split"]).astype(np.int32)), seed=1, hidden_dim=16)
    with pytest.raises(GcnHostError, match="calibrate: split 2 has no labelled rows"):
        empty.calibrate()
    empty.close()
    # two logical ranks: the fit and the measurement are refused on each, predict under a temperature works (row-local)
    tw = ThreadWorld(2)
    seen, errors = [None, None], []

    def body(rank):
        try:
            ag, ar = tw.callbacks(rank)
            r = HipGCNModel(ds, seed=4, device=0, rank=rank, world=2, host_allgather=ag, host_allreduce=ar, hidden_dim=16, dropout=0.5)
            msgs = []
            for call in (r.calibrate, lambda: r.calibration(split=3)):
                try:
                    call()
                    msgs.append("no error")
                except GcnHostError as e:
                    msgs.append(str(e))
            p1 = r.predict(logp=True)
            r.set_temperature(2.0)
            p2 = r.predict(logp=True)
            seen[rank] = (msgs, p1, p2)
            r.close()
        except BaseException as e:                                # a failed rank must not leave the other at a barrier forever
            errors.append((rank, e))
            tw.barrier.abort()
    threads = [threading.Thread(target=body, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    beta = R.f32(np.float32(1.0) / np.float32(2.0))
    for msgs, p1, p2 in seen:
        assert "calibrate: one rank only" in msgs[0] and "calibration: one rank only" in msgs[1]
        out, e_out, prob, e_prob = R.scale(p1[2], beta)
        assert np.array_equal(p1[0], p2[0]) and np.all(np.abs(p2[2] - out) <= e_out) and np.all(np.abs(p2[1] - prob) <= e_prob)


def test_calibration_lowers_the_test_ece_on_a_planted_graph():
    """8 planted communities of 128 nodes (half of every node's edges inside its community, 8 features), no dropout, 50 epochs:
    the model separates the test split (accuracy 0.81 with the CPU oracle's training path, same data and seed 5) but its
    probabilities lag behind — in the float64 reference on those weights the test-split ECE is 0.4277 before and 0.0725 after the
    fit on the validation split (T = 0.22; 194 test rows, no ambiguous row, ECE bound 5e-6: a gain of 0.355).  Here: the same
    reference on the model's own log-softmax rows shows a gain of at least 0.1, and the model's two ECE values match it within
    the bound"""
    ds = datagen.planted_communities(n_comm=8, size=128, p_in=0.5, feats=8)
    ds, m = trained(ds, epochs=50, dropout=0.0)
    _, _, logp = m.predict(logp=True)
    test, val = np.flatnonzero(ds["split"] == 3), np.flatnonzero(ds["split"] == 2)
    before = m.calibration(split=3)
    fit = m.calibrate()
    after = m.calibration(split=3)
    ref_before = check_calibration(before, logp, ds["label"], test, 1.0)
    ref_after = check_calibration(after, logp, ds["label"], test, fit["temperature"])
    ref_fit = R.fit(logp, ds["label"], val)
    print(f"planted: T {fit['temperature']:.4f} (reference {ref_fit['temperature']:.4f}), test ECE reference {ref_before['ece']:.4f} -> "
          f"{ref_after['ece']:.4f}, GPU {before['ece']:.4f} -> {after['ece']:.4f}, {test.size} test rows")
    assert ref_before["ece"] - ref_after["ece"] > 0.1, (ref_before["ece"], ref_after["ece"])
    assert abs(fit["ece_before"] - m.calibration(split=2, temperature=1.0)["ece"]) <= 1e-12
    m.close()


# ---- the command line ---------------------------------------------------------------------------------------------------

def test_cli_calibrate(tmp_path):
    """gcn-hip cora-syn with GCN_CALIBRATE: one more line after the test line, which parses; the file holds two tables whose
    counts sum to the test split; GCN_PREDICT's probabilities are the Python path's calibrated ones (weights handed over through
    a weights file, 0 epochs); refused with GCN_MULTILABEL before the GPU is touched"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.make_dataset("cora-syn")
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "cora-syn.gcnbin"))
    m = HipGCNModel(ds, seed=3, hidden_dim=16, dropout=0.5)
    m.run_epochs(6, want_trace=False)
    w = str(tmp_path / "w.gcnw")
    m.save_weights(w)
    fit = m.calibrate()
    pred, prob = m.predict()
    ece = m.calibration(split=3)["ece"]
    m.close()
    args = ["cora-syn", "-", "-", "16", "-", "0.5", "-", "-", "0"]
    table, p = str(tmp_path / "cal.txt"), str(tmp_path / "p.txt")
    env = dict(os.environ, GCN_SEED="3", GCN_LOAD_WEIGHTS=w, GCN_CALIBRATE=table, GCN_PREDICT=p)
    r = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-2].startswith("test_loss=")
    got = re.fullmatch(r"temperature=(\S+) val_nll_before=(\S+) val_nll_after=(\S+) test_ece_before=(\S+) test_ece_after=(\S+)", lines[-1])
    assert got, lines[-3:]
    t, nb, na, eb, ea = (float(x) for x in got.groups())
    assert abs(t - fit["temperature"]) <= 1e-5 + 1e-5 * t and abs(nb - fit["nll_before"]) <= 2e-5 and abs(na - fit["nll_after"]) <= 2e-5
    assert na <= nb + 1e-5 and abs(ea - ece) <= 1e-5 + 2.0 / int((ds["split"] == 3).sum())
    text = open(table).read().strip().splitlines()
    heads = [i for i, l in enumerate(text) if l.startswith("temperature ")]
    assert len(heads) == 2 and len(text) == 2 * 16
    labelled = int(((ds["split"] == 3) & (ds["label"] >= 0) & (ds["label"] < ds["output_dim"])).sum())
    for h in heads:
        assert int(text[h].split()[3]) == labelled
        assert sum(int(l.split()[7]) for l in text[h + 1:h + 16]) == labelled
    assert float(text[heads[0]].split()[1]) == 1.0 and abs(float(text[heads[1]].split()[1]) - t) <= 1e-5 * t + 1e-5
    rows = np.loadtxt(p, ndmin=2)
    assert np.array_equal(rows[:, 1].astype(np.int64), pred) and np.all(np.abs(rows[:, 2] - prob) <= 2e-5)      # %.6g, and T to 1e-5
    labels = tmp_path / "labels.txt"
    labels.write_text("".join(f"{int(c) % 3}\n" for c in ds["label"]))
    bad = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=dict(env, GCN_MULTILABEL=str(labels)),
                         capture_output=True, text=True)
    assert bad.returncode != 0 and "GCN_CALIBRATE fits the temperature of a single-label model" in bad.stderr, bad.stderr[-500:]
