"""Per-class metrics from integer counts (host/report.h through model.class_report) against plain numpy formulas, its argument
checks, and the presence of the evaluation entry points in the libraries and their headers.  No GPU needed."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ratio(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.where(b > 0, a / np.where(b > 0, b, 1.0), 0.0)


def numpy_report(tp, fp, fn):
    tp, fp, fn = (np.asarray(v, np.int64) for v in (tp, fp, fn))
    f1 = ratio(2 * tp, 2 * tp + fp + fn)
    return dict(support=(tp + fn).astype(np.float64), precision=ratio(tp, tp + fp), recall=ratio(tp, tp + fn), f1=f1,
                macro_f1=float(f1.mean()), micro_f1=float(ratio(2 * tp.sum(), 2 * tp.sum() + fp.sum() + fn.sum())))


def check(got, want, C):
    """1e-15 relative: both sides are one float64 division of exactly represented integers; the mean of C values gets C ulps"""
    for k in ("support", "precision", "recall", "f1"):
        assert got[k].dtype == np.float64 and got[k].shape == (C,)
        assert np.all(np.isfinite(got[k])), k
        assert np.allclose(got[k], want[k], rtol=1e-15, atol=0), k
    assert got["micro_f1"] == pytest.approx(want["micro_f1"], rel=1e-15, abs=0)
    assert got["macro_f1"] == pytest.approx(want["macro_f1"], rel=C * 2.3e-16, abs=0)


def from_matrix(m):
    m = np.asarray(m, np.int64)
    tp = np.diag(m)
    return tp, m.sum(axis=0) - tp, m.sum(axis=1) - tp


@pytest.mark.parametrize("C", [1, 2, 7, 41, 64])
def test_class_report_from_a_confusion_matrix(C):
    from cuda_gcn_amd.model import class_report
    rng = np.random.default_rng(C)
    for trial in range(4):
        m = rng.integers(0, 10 ** rng.integers(1, 8), (C, C)).astype(np.int64)
        if C > 2 and trial % 2:
            m[1, :] = 0                                        # a class with no support
            m[:, 2] = 0                                        # a class never predicted
        got = class_report(confusion=m)
        tp, fp, fn = from_matrix(m)
        check(got, numpy_report(tp, fp, fn), C)
        assert np.array_equal(got["tp"], tp) and np.array_equal(got["fp"], fp) and np.array_equal(got["fn"], fn)
        assert got["tp"].dtype == np.int64
        assert got["rows"] == int(m.sum())
        want_acc = float(np.trace(m)) / float(m.sum()) if m.sum() else 0.0
        assert got["accuracy"] == pytest.approx(want_acc, rel=1e-15, abs=0)
        assert got["accuracy"] == pytest.approx(got["micro_f1"], rel=1e-15, abs=0)      # single-label: the same number
        if C > 2 and trial % 2:
            assert got["support"][1] == 0 and got["recall"][1] == 0 and got["f1"][1] == 0
            assert got["precision"][2] == 0 and got["f1"][2] == 0


@pytest.mark.parametrize("C", [1, 3, 121, 256])
def test_class_report_from_tp_fp_fn(C):
    from cuda_gcn_amd.model import class_report
    rng = np.random.default_rng(100 + C)
    tp, fp, fn = (rng.integers(0, 2 ** 31, C).astype(np.int64) for _ in range(3))
    tp[0] = fp[0] = 0                                          # never predicted
    if C > 1:
        tp[1] = fn[1] = 0                                      # no support
    got = class_report(tp=tp, fp=fp, fn=fn)
    check(got, numpy_report(tp, fp, fn), C)
    assert got["accuracy"] == 0.0 and got["rows"] == 0
    assert got["precision"][0] == 0 and (C == 1 or got["recall"][1] == 0)


@pytest.mark.parametrize("C", [1, 5])
def test_all_zero_counts_give_zeros_not_nan(C):
    from cuda_gcn_amd.model import class_report
    for got in (class_report(confusion=np.zeros((C, C), np.int64)),
                class_report(tp=np.zeros(C, np.int64), fp=np.zeros(C, np.int64), fn=np.zeros(C, np.int64))):
        for k in ("support", "precision", "recall", "f1"):
            assert np.array_equal(got[k], np.zeros(C))
        assert got["macro_f1"] == 0.0 and got["micro_f1"] == 0.0 and got["accuracy"] == 0.0 and got["rows"] == 0


def test_one_class():
    from cuda_gcn_amd.model import class_report
    got = class_report(confusion=[[9]])
    assert got["precision"][0] == 1.0 and got["recall"][0] == 1.0 and got["f1"][0] == 1.0
    assert got["macro_f1"] == 1.0 and got["micro_f1"] == 1.0 and got["accuracy"] == 1.0 and got["support"][0] == 9.0


def test_argument_checks():
    from cuda_gcn_amd.model import class_report, GcnHostError
    with pytest.raises((GcnHostError, ValueError)):
        class_report(confusion=[[1, -1], [0, 2]])
    with pytest.raises((GcnHostError, ValueError)):
        class_report(tp=[1, 2], fp=[0, -3], fn=[0, 0])
    with pytest.raises(ValueError):
        class_report(confusion=np.zeros((2, 3), np.int64))
    with pytest.raises(ValueError):
        class_report(confusion=np.zeros(4, np.int64))
    with pytest.raises(ValueError):
        class_report(tp=[1, 2], fp=[1], fn=[0, 0])
    with pytest.raises(ValueError):
        class_report(tp=[1, 2], fp=[1, 1])
    with pytest.raises(ValueError):
        class_report()
    with pytest.raises(ValueError):
        class_report(confusion=[[1]], tp=[1], fp=[0], fn=[0])


def test_entry_points_are_exported_and_declared():
    from cuda_gcn_amd import _lib
    hip, host = _lib.gcnhip(), _lib.gcnhost()
    drv = open(os.path.join(ROOT, "include", "gcnhip_driver.h")).read()
    for n in ("gcnhip_confusion_rows", "gcnhip_bce_class_counts_rows"):
        assert hasattr(hip, n) and n in _lib.GCNHIP_SYMBOLS
        assert re.search(r"\bint\s+" + n + r"\s*\(", drv), n
    hdr = open(os.path.join(ROOT, "include", "gcnhost.h")).read()
    for n in ("gcnhost_model_evaluate", "gcnhost_class_report"):
        assert hasattr(host, n) and n in _lib.GCNHOST_SYMBOLS
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr), n
    from cuda_gcn_amd.model import HipGCNModel
    from cuda_gcn_amd.ops import Device
    assert callable(HipGCNModel.evaluate) and callable(Device.confusion_rows) and callable(Device.bce_class_counts_rows)
