"""Multi-label decision thresholds without a GPU: the numpy reference of the fit (tests/thresholds_ref.py) against the
definition — a brute force over every distinct score — on random, tie-heavy and edge-value scores; the invariant that the
fitted cut never scores below the training rule z > 0 on the fit rows; a hand-worked case; classes without positives or
negatives; the thresholds file; the refusals of the Python front end; the names in the binding tables and headers."""
import os
import re

import numpy as np
import pytest

from tests import ranking_ref as R
from tests import thresholds_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETAS = (0.5, 1.0, 2.0)


def bits(x):
    return np.float32(x).tobytes()


def columns(rng, kind, n):
    if kind == "random":
        z = rng.standard_normal(n).astype(np.float32)
    elif kind == "ties":
        z = (rng.integers(-4, 5, n) / 4).astype(np.float32)
    else:
        z = rng.choice(np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 3e-42, -3e-42, 1.17549435e-38, 1.0, -1.0, np.nan], np.float32), n)
    return z, rng.random(n) < rng.choice([0.05, 0.3, 0.7])


@pytest.mark.parametrize("kind", ["random", "ties", "edges"])
def test_reference_equals_brute_force_and_beats_the_training_rule(kind):
    """candidates = the positives' keys with ties to the largest key gives what trying every distinct score gives — threshold
    bits, counts and F — and on the fit rows F_tuned >= F(z > 0) for every class with a positive"""
    rng = np.random.default_rng({"random": 1, "ties": 2, "edges": 3}[kind])
    for it in range(200):
        z, y = columns(rng, kind, int(rng.integers(1, 60)))
        for beta in BETAS:
            got = TR.table_fit(z[:, None], y[:, None], beta)
            want = TR.brute_fit(z, y, beta)
            assert bits(got["threshold"][0]) == bits(want[0]), (it, beta, z, y)
            assert (got["defined"][0], got["tp"][0], got["fp"][0], got["fn"][0]) == want[1:5] and got["f"][0] == want[5], (it, beta, z, y)
            assert not np.isnan(got["f"][0]) and not np.isnan(got["threshold"][0])
            ok = ~np.isnan(z)
            assert got["pos"][0] == (y & ok).sum() and got["neg"][0] == (~y & ok).sum() and got["invalid"][0] == (~ok).sum()
            cnt = TR.counts(z[ok, None], y[ok, None], got["threshold"])[:, 0]
            assert cnt.tolist() == [got["tp"][0], got["fp"][0], got["fn"][0]]
            if got["defined"][0]:
                d = TR.default_counts(z[ok, None], y[ok, None])[:, 0]
                assert got["f"][0] >= TR.f_beta(d[0], d[1], d[2], beta)


def test_hand_worked_case():
    """positives at 2, 1, 1, -1 and negatives at 3, 1, 0, 0, -2.  Cuts at the positives' scores:
         t = 2: TP 1 FP 1 FN 3    t = 1: TP 3 FP 2 FN 1    t = -1: TP 4 FP 4 FN 0
       beta = 1: F = 2 TP / (2 TP + FN + FP) = 2/6, 6/9, 8/12: the cuts 1 and -1 tie at 2/3 and the higher one, 1, wins.
       beta = 2: F = 5 TP / (5 TP + 4 FN + FP) = 5/18, 15/21, 20/24: -1 wins.   beta = 0.5: 1.25 TP / (1.25 TP + 0.25 FN + FP)
       = 1.25/3, 3.75/6, 5/9: 1 wins."""
    z = np.array([2, 1, 1, -1, 3, 1, 0, 0, -2], np.float32)
    y = np.array([1, 1, 1, 1, 0, 0, 0, 0, 0], bool)
    assert 6.0 / 9.0 == 8.0 / 12.0
    for beta, thr, tp, fp, fn, f in ((1.0, 1.0, 3, 2, 1, 6.0 / 9.0), (2.0, -1.0, 4, 4, 0, 20.0 / 24.0), (0.5, 1.0, 3, 2, 1, 3.75 / 6.0)):
        got = TR.table_fit(z[:, None], y[:, None], beta)
        assert (got["threshold"][0], got["defined"][0], got["tp"][0], got["fp"][0], got["fn"][0], got["f"][0]) == (thr, 1, tp, fp, fn, f)
    assert TR.f_beta(3, 2, 1, 1.0) == 6.0 / 9.0 and TR.f_beta(0, 5, 3, 1.0) == 0.0


def test_classes_without_positives_or_negatives():
    z = np.array([0.5, -0.0, -1.0, 2.0, np.nan], np.float32)
    none = TR.table_fit(z[:, None], np.zeros((5, 1), bool))
    assert bits(none["threshold"][0]) == bits(0.0) and none["defined"][0] == 0 and none["f"][0] == 0.0
    assert (none["tp"][0], none["fp"][0], none["fn"][0], none["pos"][0], none["neg"][0], none["invalid"][0]) == (0, 3, 0, 0, 4, 1)   # -0.0 >= 0.0
    every = TR.table_fit(z[:, None], np.ones((5, 1), bool), 2.0)
    assert every["threshold"][0] == -1.0 and every["defined"][0] == 1 and every["f"][0] == 1.0
    assert (every["tp"][0], every["fp"][0], every["fn"][0], every["pos"][0], every["neg"][0]) == (4, 0, 0, 4, 0)
    nan = TR.table_fit(np.full((3, 1), np.nan, np.float32), np.array([[1], [0], [1]], bool))
    assert nan["defined"][0] == 0 and nan["pos"][0] == nan["neg"][0] == 0 and nan["invalid"][0] == 3 and nan["fp"][0] == 0
    # the rule: -0.0 and +0.0 are one cut, a denormal cut is not zero, a NaN logit is never predicted, a NaN cut predicts nothing
    zz = np.array([[0.0, -0.0, 1e-45, -1e-45, np.nan]], np.float32).T
    assert TR.predict(zz, [0.0])[:, 0].tolist() == TR.predict(zz, [-0.0])[:, 0].tolist() == [True, True, True, False, False]
    assert TR.predict(zz, [1e-45])[:, 0].tolist() == [False, False, True, False, False]
    assert not TR.predict(zz, [np.nan]).any()
    k = R.key(np.array([-np.inf, -1.0, -1e-45, 0.0, 1e-45, 1.0, np.inf], np.float32))
    assert same_floats(TR.key_to_float(k), [-np.inf, -1.0, -1e-45, 0.0, 1e-45, 1.0, np.inf])


def same_floats(a, b):
    return np.ascontiguousarray(a, np.float32).tobytes() == np.ascontiguousarray(b, np.float32).tobytes()


def test_thresholds_file_round_trip(tmp_path):
    """every float32 survives %.9g exactly (random bit patterns, denormals, +-inf, -0.0); the fit's comments are written and
    ignored on reading, as are comment lines; a wrong count, a bad token and a NaN are refused with the line named"""
    from cuda_gcn_amd.model import GcnHostError, read_thresholds, write_thresholds
    rng = np.random.default_rng(4)
    thr = rng.integers(0, 2 ** 32, 4000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    thr = thr[~np.isnan(thr)]
    thr = np.concatenate([thr, np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -3e-42, 1.17549435e-38, 3.4028235e38, 0.1], np.float32)])
    path = str(tmp_path / "thr.txt")
    write_thresholds(path, thr)
    assert same_floats(read_thresholds(path), thr) and same_floats(read_thresholds(path, num_classes=thr.size), thr)
    c = 5
    fit = dict(threshold=np.array([0.25, -1.5, 0.0, 1e-45, np.inf], np.float32), pos=np.arange(c), neg=np.arange(c) + 10, tp=np.arange(c),
               fp=np.arange(c) * 2, fn=np.zeros(c, np.int64), f=np.linspace(0, 1, c))
    write_thresholds(path, fit)
    lines = open(path).read().splitlines()
    assert len(lines) == c and lines[0].split()[0] == "0.25"
    assert lines[1] == "-1.5 # class 1 pos 1 neg 11 tp 1 fp 2 fn 0 f 0.250000000"
    assert same_floats(read_thresholds(path, num_classes=c), fit["threshold"])
    with open(path, "w") as f:
        f.write("# fitted on the validation split\n0.5\n\n  -2e-3   # class 1\n1e-45#x\ninf\n")
    assert same_floats(read_thresholds(path), np.array([0.5, -2e-3, 1e-45, np.inf], np.float32))
    with pytest.raises(GcnHostError, match="4 thresholds for 5 classes"):
        read_thresholds(path, num_classes=5)
    for text, msg in (("0.5\nnan\n", "line 2: the threshold is NaN"), ("0.5\n0.25 0.75\n", "line 2: '0.25 0.75' is not one number"),
                      ("abc\n", "line 1: 'abc' is not one number"), ("# nothing\n\n", "no thresholds in the file")):
        with open(path, "w") as f:
            f.write(text)
        with pytest.raises(GcnHostError, match=msg):
            read_thresholds(path)
    with pytest.raises(GcnHostError, match="cannot open the thresholds file"):
        read_thresholds(str(tmp_path / "missing.txt"))
    with pytest.raises(ValueError, match="write_thresholds: the threshold of class 1 is NaN"):
        write_thresholds(path, np.array([0.0, np.nan], np.float32))
    with pytest.raises(ValueError, match="one entry per threshold"):
        write_thresholds(path, dict(fit, pos=np.arange(3)))
    lib = __import__("cuda_gcn_amd._lib", fromlist=["x"]).gcnhost()
    bad = np.array([0.0, np.nan], np.float32)
    assert lib.gcnhost_thresholds_write(os.fsencode(path), 2, bad.ctypes.data, None, None, None, None, None, None) == -1
    assert b"the threshold of class 1 is NaN" in lib.gcnhost_last_error()
    pos = np.zeros(2, np.int64)
    assert lib.gcnhost_thresholds_write(os.fsencode(path), 2, bad.ctypes.data, pos.ctypes.data, None, None, None, None, None) == -1
    assert b"go together" in lib.gcnhost_last_error()


def test_python_side_refusals():
    from cuda_gcn_amd.model import check_beta, thresholds_array
    assert same_floats(thresholds_array("evaluate", [0.5, -1], 2), [0.5, -1.0])
    assert same_floats(thresholds_array("evaluate", dict(threshold=np.zeros(3)), 3), np.zeros(3))
    with pytest.raises(ValueError, match="evaluate: 3 thresholds for 4 classes"):
        thresholds_array("evaluate", np.zeros(3), 4)
    with pytest.raises(ValueError, match="predict_multilabel: the threshold of class 2 is NaN"):
        thresholds_array("predict_multilabel", [0, 1, np.nan], 3)
    assert check_beta("tune_thresholds", 2) == 2.0
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tune_thresholds: beta must be finite and > 0"):
            check_beta("tune_thresholds", bad)


def test_names_in_the_binding_tables_and_headers():
    from cuda_gcn_amd import _lib
    drv = open(os.path.join(ROOT, "include", "gcnhip_driver.h")).read()
    host_h = open(os.path.join(ROOT, "include", "gcnhost.h")).read()
    hip, host = _lib.gcnhip(), _lib.gcnhost()
    for n in ("gcnhip_threshold_scan", "gcnhip_bce_predict_rows_thr", "gcnhip_bce_class_counts_rows_thr"):
        assert n in _lib.GCNHIP_SYMBOLS and hasattr(hip, n) and re.search(rf"\bint {n}\(", drv)
    for n in ("gcnhost_model_tune_thresholds", "gcnhost_model_predict_multilabel_thr", "gcnhost_model_evaluate_thr", "gcnhost_thresholds_read",
              "gcnhost_thresholds_write"):
        assert n in _lib.GCNHOST_SYMBOLS and hasattr(host, n) and re.search(rf"\bint {n}\(", host_h)
    from cuda_gcn_amd import ops
    assert re.search(rf"#define GCNHIP_THRESHOLD_SCAN_BLOCKS {ops.THRESHOLD_SCAN_BLOCKS}\b", drv)
    for name in ("threshold_scan", "bce_predict_rows_thr", "bce_class_counts_rows_thr"):
        assert hasattr(ops.Device, name)
