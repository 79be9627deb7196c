"""HipGCNModel.tune_thresholds and the thresholds= paths of predict_multilabel / evaluate on the planted 40-class multi-label
model of tests/test_ranking_model_gpu.py, against tests/thresholds_ref.py on ranking(return_scores=True)'s own score rows (the
logits of the same forward): every output exactly.  Splits, a query with repeats, every row, one class per batch; the cuts
applied; thresholds=None and ranking() unchanged; no side effects on training; the refusals."""
import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import thresholds_ref as TR
from tests.test_ranking_model_gpu import listed, multi, same_bits, same_result

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    ds, m = multi()
    yield ds, m
    m.close()


def check_fit(m, ds, split=None, nodes=None, beta=1.0, **kw):
    """tune_thresholds() against the reference on ranking()'s scores of the same rows; returns (fit, scores, truth)"""
    from cuda_gcn_amd.model import class_report
    fit = m.tune_thresholds(split=split, nodes=nodes, beta=beta, **kw)
    scores = m.ranking(split=split, nodes=nodes, return_scores=True)["scores"]
    who = listed(m, ds, split, nodes)
    truth = ds["multilabel"][who]
    want = TR.table_fit(scores, truth, beta)
    assert fit["rows"] == who.size and fit["beta"] == beta
    assert fit["threshold"].dtype == np.float32 and fit["f"].dtype == np.float64 and fit["defined"].dtype == bool
    assert same_bits(fit["threshold"], want["threshold"]), (fit["threshold"], want["threshold"])
    assert same_bits(fit["f"], want["f"])
    assert np.array_equal(fit["defined"], want["defined"].astype(bool))
    for k in ("tp", "fp", "fn", "pos", "neg", "invalid"):
        assert fit[k].dtype == np.int64 and np.array_equal(fit[k], want[k]), k
    rep = class_report(tp=fit["tp"], fp=fit["fp"], fn=fit["fn"])
    for k in ("support", "precision", "recall", "f1", "macro_f1", "micro_f1"):
        assert same_bits(np.asarray(fit[k]), np.asarray(rep[k])), k
    # the invariant of the fit: on its own rows no class does worse than with the training rule
    base = TR.default_counts(scores, truth)
    for c in np.flatnonzero(fit["defined"]):
        assert fit["f"][c] >= TR.f_beta(base[0][c], base[1][c], base[2][c], beta), c
    return fit, scores, truth


def test_fit_equals_the_reference(model):
    """the validation split (some classes have no positive there), the other splits, a query with repeats, every row and no
    row; beta 0.5, 1 and 2; one class per batch and a few per batch give the same bits"""
    ds, m = model
    n = ds["num_nodes"]
    fit, _, truth = check_fit(m, ds, split=2)
    assert not fit["defined"].all() and fit["defined"].any() and not fit["invalid"].any()
    assert np.array_equal(fit["defined"], truth.any(axis=0))
    und = ~fit["defined"]
    assert not fit["threshold"][und].any() and not fit["f"][und].any() and not fit["tp"][und].any() and not fit["fn"][und].any()
    assert same_result(fit, m.tune_thresholds())               # the default is the validation split at beta 1
    q = np.concatenate([np.arange(0, n, 2), [7, 7, 7, n - 1]]).astype(np.int32)
    for kw in (dict(split=1, beta=2.0), dict(split=3, beta=0.5), dict(nodes=q), dict()):
        f, _, _ = check_fit(m, ds, **kw)
        who = listed(m, ds, kw.get("split"), kw.get("nodes"))
        for cap in (1, 5 * 16 * who.size):
            assert same_result(f, m.tune_thresholds(**dict(dict(split=None), **kw), scratch_bytes=cap))
    empty = m.tune_thresholds(split=None, nodes=[])
    assert empty["rows"] == 0 and not empty["defined"].any() and not empty["threshold"].any() and not empty["fp"].any() and empty["macro_f1"] == 0.0


def test_cuts_applied(model):
    """evaluate(thresholds=) on the fit rows returns the fit's counts and a macro-F1 that is at least the default's;
    predict_multilabel(thresholds=) is scores >= thr in numpy and prob stays the sigmoid; thresholds=None gives the old bits"""
    ds, m = model
    n = ds["num_nodes"]
    fit, scores, _ = check_fit(m, ds, split=2)
    thr = fit["threshold"]
    base = m.evaluate(split=2)
    ev = m.evaluate(split=2, thresholds=thr)
    for k in ("tp", "fp", "fn"):
        assert np.array_equal(ev[k], fit[k]), k
    assert ev["rows"] == fit["rows"] and same_result(ev, m.evaluate(split=2, thresholds=fit))
    assert ev["macro_f1"] >= base["macro_f1"] and ev["macro_f1"] == fit["macro_f1"]
    print("validation macro-F1: default", base["macro_f1"], "tuned", ev["macro_f1"])
    assert same_result(base, m.evaluate(split=2)) and same_result(base, m.evaluate(split=2, thresholds=None))
    # other rows than the fit's: against the rule on their scores
    q = np.concatenate([np.arange(1, n, 3), [5, 5, n - 1]]).astype(np.int32)
    for kw in (dict(split=3), dict(nodes=q), dict()):
        sc = m.ranking(**dict(dict(split=None), **kw), return_scores=True)["scores"]
        who = listed(m, ds, kw.get("split"), kw.get("nodes"))
        ev = m.evaluate(**kw, thresholds=thr)
        assert np.array_equal(np.stack([ev["tp"], ev["fp"], ev["fn"]]), TR.counts(sc, ds["multilabel"][who], thr)) and ev["rows"] == who.size
    # predictions
    sc = m.ranking(split=None, nodes=q, return_scores=True)["scores"]
    old_sets, old_prob = m.predict_multilabel(nodes=q, prob=True)
    sets, prob = m.predict_multilabel(nodes=q, prob=True, thresholds=thr)
    assert np.array_equal(sets, sc >= thr[None, :]) and np.array_equal(sets, TR.predict(sc, thr)) and same_bits(prob, old_prob)
    assert np.array_equal(old_sets, sc > 0) and not np.array_equal(sets, old_sets)
    assert np.array_equal(m.predict_multilabel(nodes=q, thresholds=thr), sets)
    tiny = np.full(40, np.nextafter(np.float32(0), np.float32(1)), np.float32)
    assert np.array_equal(m.predict_multilabel(nodes=q, thresholds=tiny), old_sets)
    every = m.predict_multilabel(thresholds=thr)
    ids, _ = m.row_ids()
    assert every.shape == (n, 40) and np.array_equal(every[np.argsort(ids)][q], sets)
    again_sets, again_prob = m.predict_multilabel(nodes=q, prob=True, thresholds=None)
    assert same_bits(again_sets, old_sets) and same_bits(again_prob, old_prob)


def test_ranking_is_unchanged_around_the_calls(model):
    ds, m = model
    before = m.ranking(split=3, return_scores=True)
    fit = m.tune_thresholds(split=2, scratch_bytes=1)
    m.evaluate(split=3, thresholds=fit)
    m.predict_multilabel(thresholds=fit)
    assert same_result(before, m.ranking(split=3, return_scores=True))


def test_thresholds_between_epochs_change_nothing():
    """two models with the same seed train in lockstep, one fitting and applying thresholds between epochs: their traces,
    weights and the logits of the last forward are bit-identical"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.planted_multilabel(classes=41, size=128)
    kw = dict(seed=6, hidden_dim=16, dropout=0.5, multilabel=ds["multilabel"])
    a, b = HipGCNModel(ds, **kw), HipGCNModel(ds, **kw)
    ta, tb = [], []
    q = np.arange(0, ds["num_nodes"], 7, dtype=np.int32)
    for e in range(3):
        ta.append(a.run_epochs(1))
        tb.append(b.run_epochs(1))
        fit = b.tune_thresholds(scratch_bytes=1 if e == 0 else 0)
        b.tune_thresholds(split=None, nodes=q, beta=2.0)
        b.evaluate(split=3, thresholds=fit)
        b.predict_multilabel(nodes=q, thresholds=fit)
    ta.append(np.array([a.train_epoch() + a.eval(2)], np.float32))
    tb.append(np.array([b.train_epoch() + b.eval(2)], np.float32))
    ta, tb = np.concatenate(ta), np.concatenate(tb)
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32)), (ta, tb)
    for k in (2, 5):
        assert same_bits(a.var(k), b.var(k)), k
    ea = a.eval(3)
    before = b.eval(3), b.var(6)
    fit = b.tune_thresholds()
    b.evaluate(split=1, thresholds=fit)
    assert same_bits(before[1], b.var(6)) and before[0] == ea and same_bits(a.var(6), b.var(6))
    assert a.eval(3) == b.eval(3) == ea
    a.close()
    b.close()


def test_refusals(model):
    """a single-label model, a split outside 1..3, a split and a query together, a bad beta, a negative scratch cap, more than
    2^24 listed rows, thresholds of the wrong length or with a NaN: an error naming the call, from the Python front end and
    from the C entry points called directly.  (More than one rank is refused by the check ranking() shares, which
    tests/test_ranking_model_gpu.py reaches with two ranks.)"""
    from cuda_gcn_amd.model import HipGCNModel, GcnHostError, _ck
    ds, m = model
    c = 40

    def direct(mm, split=2, nodes=None, n_nodes=0, beta=1.0):
        k = max(mm.params.output_dim, 1)
        out = [np.zeros(k, np.int64) for _ in range(6)]
        thr, f, d = np.zeros(k, np.float32), np.zeros(k, np.float64), np.zeros(k, np.int32)
        return mm.lib.gcnhost_model_tune_thresholds(mm.h, split, nodes, n_nodes, beta, 0, thr.ctypes.data, out[0].ctypes.data, out[1].ctypes.data,
                                                    out[2].ctypes.data, f.ctypes.data, out[3].ctypes.data, out[4].ctypes.data, out[5].ctypes.data,
                                                    d.ctypes.data, None)

    assert direct(m) == 0
    for bad in (0, 4, -1, "val"):
        with pytest.raises(ValueError, match="tune_thresholds: split is 1"):
            m.tune_thresholds(split=bad)
    with pytest.raises(ValueError, match="tune_thresholds: give a split or a node query, not both"):
        m.tune_thresholds(split=2, nodes=[1])
    with pytest.raises(ValueError, match="tune_thresholds: scratch_bytes must be >= 0"):
        m.tune_thresholds(scratch_bytes=-1)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tune_thresholds: beta must be finite and > 0"):
            m.tune_thresholds(beta=bad)
        with pytest.raises(GcnHostError, match="tune_thresholds: beta must be finite and > 0"):
            _ck(m.lib, direct(m, beta=bad), "call")
    for split in (4, -1):
        with pytest.raises(GcnHostError, match="tune_thresholds: invalid argument"):
            _ck(m.lib, direct(m, split=split), "call")
    with pytest.raises(GcnHostError, match="tune_thresholds: node .* is not a node of the dataset"):
        m.tune_thresholds(split=None, nodes=[ds["num_nodes"]])
    one = np.zeros(1, np.int32)
    with pytest.raises(GcnHostError, match=r"tune_thresholds: at most 2\^24 listed rows"):
        _ck(m.lib, direct(m, split=0, nodes=one.ctypes.data, n_nodes=2 ** 24 + 1), "call")
    nan = np.zeros(c, np.float32)
    nan[7] = np.nan
    for call in (lambda t: m.evaluate(split=2, thresholds=t), lambda t: m.predict_multilabel(thresholds=t)):
        with pytest.raises(ValueError, match="39 thresholds for 40 classes"):
            call(np.zeros(c - 1, np.float32))
        with pytest.raises(ValueError, match="the threshold of class 7 is NaN"):
            call(nan)
    counts, words, rows = np.zeros((3, c), np.int64), np.zeros((ds["num_nodes"], 2), np.uint32), np.zeros(1, np.int64)
    ok = np.zeros(c, np.float32)
    for t, k, msg in ((ok, c - 1, "39 thresholds for 40 classes"), (nan, c, "the threshold of class 7 is NaN")):
        with pytest.raises(GcnHostError, match=f"evaluate: {msg}"):
            _ck(m.lib, m.lib.gcnhost_model_evaluate_thr(m.h, 2, None, 0, t.ctypes.data, k, counts.ctypes.data, rows.ctypes.data), "call")
        with pytest.raises(GcnHostError, match=f"predict_multilabel: {msg}"):
            _ck(m.lib, m.lib.gcnhost_model_predict_multilabel_thr(m.h, None, 0, t.ctypes.data, k, words.ctypes.data, None), "call")
    # a single-label model
    sds = datagen.make_dataset("tiny-syn")
    s = HipGCNModel(sds, seed=1, hidden_dim=16)
    with pytest.raises(GcnHostError, match="tune_thresholds: this is a single-label model"):
        s.tune_thresholds()
    with pytest.raises(GcnHostError, match="tune_thresholds: this is a single-label model"):
        _ck(s.lib, direct(s), "call")
    with pytest.raises(GcnHostError, match="evaluate: this is a single-label model"):
        s.evaluate(split=2, thresholds=np.zeros(sds["output_dim"], np.float32))
    with pytest.raises(GcnHostError, match="predict_multilabel: this is a single-label model"):
        s.predict_multilabel(thresholds=np.zeros(sds["output_dim"], np.float32))
    s.close()
