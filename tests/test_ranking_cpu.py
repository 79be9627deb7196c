"""Ranking metrics without a GPU: the numpy reference of tests/ranking_ref.py against scikit-learn, the key map, the host-only
derivation (host/ranking.h through gcnhost_ranking_report) on hand-worked cases and its refusals, and the binding tables."""
import numpy as np
import pytest

from tests import ranking_ref as R

FLT_MAX = np.finfo(np.float32).max


def cases():
    rng = np.random.default_rng(7)
    grid = np.arange(-1.0, 1.01, 0.25).astype(np.float32)
    for n in (2, 37, 1000):
        yield "random", rng.standard_normal(n).astype(np.float32), rng.random(n) < 0.3
        yield "ties", rng.choice(grid, n), rng.random(n) < 0.5
        z = np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        other = rng.random(n) < 0.2
        z[other] = rng.choice(grid, int(other.sum()))
        yield "zeros", z, rng.random(n) < 0.4


def test_reference_against_scikit_learn():
    """u2 / (2 P N) is roc_auc_score and ap_sum / P is average_precision_score, to 1e-12: random f32 scores, scores from
    {-1, -0.75, ..., 1} (massive ties), a mix of -0.0 and +0.0"""
    metrics = pytest.importorskip("sklearn.metrics")
    seen = 0
    for name, s, y in cases():
        if y.all() or not y.any():
            y = y.copy()
            y[0], y[-1] = True, False
        st = R.table_stats(s[:, None], y[:, None])
        rep = R.report(st["u2"], st["ap_sum"], st["pos"], st["neg"])
        assert rep["auc_defined"][0] and rep["ap_defined"][0]
        assert abs(rep["auc"][0] - metrics.roc_auc_score(y, s.astype(np.float64))) <= 1e-12, name
        assert abs(rep["ap"][0] - metrics.average_precision_score(y, s.astype(np.float64))) <= 1e-12, name
        seen += 1
    assert seen == 9


def sweep():
    tiny = np.float32(1e-45)
    pos = np.array([0.0, tiny, 2 * tiny, np.finfo(np.float32).tiny, 1e-3, 0.5, 1.0, 1.0 + 2.0 ** -23, 1e10, FLT_MAX, np.inf], np.float32)
    return np.concatenate([-pos[::-1], pos])                   # -inf .. -0.0, +0.0 .. +inf


def test_key_map():
    """monotone on a sorted sweep with +-inf, +-0, denormals and +-FLT_MAX; key(-0.0) == key(+0.0); no non-NaN key is the
    sentinel; equal floats have equal keys and only they; ops.rank_key_host is the reference's map"""
    from cuda_gcn_amd import ops
    x = sweep()
    k = ops.rank_key_host(x)
    assert k.dtype == np.uint32 and np.array_equal(k, R.key(x))
    assert np.all(np.diff(x.astype(np.float64)) >= 0)
    for i in range(x.size - 1):
        assert (k[i] < k[i + 1]) == (x[i] < x[i + 1]) and (k[i] == k[i + 1]) == (x[i] == x[i + 1]), (i, x[i], x[i + 1])
    assert ops.rank_key_host(np.float32(-0.0).reshape(1))[0] == ops.rank_key_host(np.float32(0.0).reshape(1))[0] == 0x80000000
    assert k.max() == 0xFF800000 < ops.RANK_SENTINEL == R.SENTINEL and k.min() == 0x007FFFFF
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)
    f = bits.view(np.float32)
    f = f[~np.isnan(f)]
    kf = ops.rank_key_host(f)
    assert not np.any(kf == ops.RANK_SENTINEL)
    order = np.argsort(kf, kind="stable")
    assert np.all(np.diff(f[order].astype(np.float64)) >= 0)
    assert np.all(ops.rank_key_host(np.array([np.nan, -np.nan], np.float32)) == ops.RANK_SENTINEL)


def test_ranking_report_hand_worked():
    """scores 0.1 0.4 0.35 0.8 with truth 0 0 1 1: three of the four pairs are ordered right (u2 = 6, auc = 0.75), the
    precisions at the positives are 1 and 2 / 3 (ap = 5 / 6); a tie of a positive with a negative is half a pair"""
    from cuda_gcn_amd.model import ranking_report
    st = R.table_stats(np.array([[0.1], [0.4], [0.35], [0.8]], np.float32), np.array([[0], [0], [1], [1]], bool))
    assert st["u2"][0] == 6 and st["pos"][0] == 2 and st["neg"][0] == 2 and st["ap_sum"][0] == 1.0 + 2.0 / 3.0
    tie = R.table_stats(np.array([[0.5], [0.5]], np.float32), np.array([[1], [0]], bool))
    assert tie["u2"][0] == 1 and tie["ap_sum"][0] == 0.5
    r = ranking_report(u2=[6, 1], ap_sum=[1.0 + 2.0 / 3.0, 0.5], pos=[2, 1], neg=[2, 1])
    assert r["auc"].tolist() == [0.75, 0.5] and r["ap"].tolist() == [(1.0 + 2.0 / 3.0) / 2, 0.5]
    assert r["auc_defined"].all() and r["ap_defined"].all() and r["classes_defined"] == 2
    assert r["macro_auc"] == 0.625 and r["macro_ap"] == ((1.0 + 2.0 / 3.0) / 2 + 0.5) / 2
    assert r["weighted_auc"] == (2 * 0.75 + 0.5) / 3 and r["weighted_ap"] == (2 * ((1.0 + 2.0 / 3.0) / 2) + 0.5) / 3
    want = R.report([6, 1], [1.0 + 2.0 / 3.0, 0.5], [2, 1], [2, 1])
    for k, v in want.items():
        assert np.array_equal(np.asarray(r[k]), np.asarray(v)), k


def test_ranking_report_undefined_classes():
    """P = 0, N = 0 and both give 0 with the mask clear — never NaN; the macro and weighted means run over the defined classes"""
    from cuda_gcn_amd.model import ranking_report
    #            defined   P = 0   N = 0   both    defined
    r = ranking_report(u2=[12, 0, 0, 0, 3], ap_sum=[2.5, 0.0, 4.0, 0.0, 0.5], pos=[3, 0, 4, 0, 1], neg=[4, 5, 0, 0, 3])
    assert r["auc_defined"].tolist() == [True, False, False, False, True] and r["ap_defined"].tolist() == [True, False, True, False, True]
    assert r["auc"].tolist() == [0.5, 0.0, 0.0, 0.0, 0.5] and r["ap"].tolist() == [2.5 / 3, 0.0, 1.0, 0.0, 0.5]
    assert r["classes_defined"] == 2 and r["macro_auc"] == 0.5 and r["macro_ap"] == (2.5 / 3 + 1.0 + 0.5) / 3
    assert r["weighted_auc"] == 0.5 and r["weighted_ap"] == (3 * (2.5 / 3) + 4 * 1.0 + 0.5) / 8
    none = ranking_report(u2=[0, 0], ap_sum=[0.0, 0.0], pos=[0, 0], neg=[0, 7])
    assert not none["auc_defined"].any() and not none["ap_defined"].any() and none["classes_defined"] == 0
    assert none["macro_auc"] == none["macro_ap"] == none["weighted_auc"] == none["weighted_ap"] == 0.0
    assert not np.isnan(np.concatenate([r["auc"], r["ap"], none["auc"], none["ap"]])).any()
    want = R.report([12, 0, 0, 0, 3], [2.5, 0.0, 4.0, 0.0, 0.5], [3, 0, 4, 0, 1], [4, 5, 0, 0, 3])
    for k, v in want.items():
        assert np.array_equal(np.asarray(r[k]), np.asarray(v)), k


def test_ranking_report_refusals():
    from cuda_gcn_amd.model import GcnHostError, ranking_report
    ok = dict(u2=[4], ap_sum=[1.0], pos=[2], neg=[2])
    ranking_report(**ok)
    for bad, msg in ((dict(ok, pos=[-1]), "negative count for class 0"), (dict(ok, neg=[-2]), "negative count for class 0"),
                     (dict(ok, u2=[9]), r"u2 outside \[0, 2 P N\] for class 0"), (dict(ok, u2=[-1]), r"u2 outside \[0, 2 P N\]"),
                     (dict(ok, ap_sum=[2.5]), r"ap_sum outside \[0, P\]"), (dict(ok, ap_sum=[-0.5]), r"ap_sum outside \[0, P\]"),
                     (dict(ok, ap_sum=[float("nan")]), r"ap_sum outside \[0, P\]"),
                     (dict(u2=[], ap_sum=[], pos=[], neg=[]), "the number of classes must be at least 1"),
                     (dict(ok, pos=[1, 2]), "u2, ap_sum, pos and neg must have one entry per class")):
        with pytest.raises(GcnHostError, match=f"ranking_report: {msg}"):
            ranking_report(**bad)
    # u2 = 2 P N exactly is a perfect ranking, not an error
    assert ranking_report(u2=[8], ap_sum=[2.0], pos=[2], neg=[2])["auc"][0] == 1.0


def test_binding_tables_name_the_new_entry_points():
    from cuda_gcn_amd import _lib, ops
    hip, host = _lib.gcnhip(), _lib.gcnhost()
    for n in ("gcnhip_rank_keys", "gcnhip_sort_segments_u32", "gcnhip_rank_stats", "gcnhip_sort_tile"):
        assert n in _lib.GCNHIP_SYMBOLS and hasattr(hip, n)
    for n in ("gcnhost_model_ranking", "gcnhost_ranking_report"):
        assert n in _lib.GCNHOST_SYMBOLS and hasattr(host, n)
    t = ops.SORT_TILE                                          # asked of the library: no GPU needed
    assert t == hip.gcnhip_sort_tile() and t >= 256 and t & (t - 1) == 0
