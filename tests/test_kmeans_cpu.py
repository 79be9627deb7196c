"""What of the clustering query needs no GPU: the scores of host/kmeans.h against the formulas of tests/kmeans_ref.py and, where it
imports, against scikit-learn; the reference's Philox draw; the scratch plan's byte counts; the ABI tables."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import dropout_ref
from tests import kmeans_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("purity", "homogeneity", "completeness", "v_measure", "nmi", "ari", "entropy_classes", "entropy_clusters")


def tables():
    rng = np.random.default_rng(11)
    out = []
    for k, c in ((1, 1), (1, 5), (6, 1), (3, 3), (8, 5), (41, 41), (256, 64), (7, 64)):
        t = rng.integers(0, 40, (k, c))
        out.append(("random", t))
        if k > 2 and c > 2:
            u = t.copy()
            u[1] = 0
            u[:, 2] = 0
            u[rng.random((k, c)) < 0.5] = 0
            out.append(("empty rows and columns", u))
    out.append(("one cluster", np.array([[5, 7, 1, 0]])))
    out.append(("one class", np.array([[5], [7], [0], [2]])))
    out.append(("one cluster, one class", np.array([[9]])))
    out.append(("one non-empty cell", np.array([[0, 0], [0, 4], [0, 0]])))
    perm = np.zeros((5, 5), np.int64)
    perm[np.arange(5), rng.permutation(5)] = [3, 1, 10, 7, 2]
    out.append(("a perfect match up to relabelling", perm))
    out.append(("independent", np.outer([2, 4, 6], [1, 3, 5])))
    out.append(("no rows", np.zeros((3, 4), np.int64)))
    out.append(("large counts", rng.integers(0, 200000, (20, 10))))
    return out


def labels_of(t):
    i, y = np.nonzero(t)
    reps = t[i, y]
    return np.repeat(y, reps), np.repeat(i, reps)                 # (truth, cluster) per row


def test_cluster_report_matches_the_formulas_and_sklearn():
    from cuda_gcn_amd.model import cluster_report
    try:
        from sklearn import metrics as SK
    except ImportError:
        SK = None
    for what, t in tables():
        got = cluster_report(t)
        want = R.cluster_scores(t)
        assert got["rows"] == want["rows"] == int(np.sum(t)), what
        for name in NAMES:
            assert np.isfinite(got[name]), (what, name)
            assert abs(got[name] - want[name]) <= 1e-12, (what, name, got[name], want[name])
        if SK is not None and got["rows"] > 0 and got["rows"] < 100000:
            truth, pred = labels_of(np.asarray(t))
            h, c, v = SK.homogeneity_completeness_v_measure(truth, pred)
            sk = dict(homogeneity=h, completeness=c, v_measure=v, nmi=SK.normalized_mutual_info_score(truth, pred),
                      ari=SK.adjusted_rand_score(truth, pred))
            for name, x in sk.items():
                assert abs(got[name] - x) <= 1e-12, (what, name, got[name], x)
    p = cluster_report(tables()[-4][1])
    assert p["purity"] == 1.0 and abs(p["nmi"] - 1) <= 1e-12 and p["ari"] == 1.0
    one = cluster_report(np.array([[9]]))
    assert (one["nmi"], one["ari"], one["v_measure"], one["purity"]) == (1.0, 1.0, 1.0, 1.0)
    single_cluster = cluster_report(np.array([[5, 7, 1, 0]]))
    assert single_cluster["nmi"] == 0.0 and single_cluster["ari"] == 0.0 and single_cluster["completeness"] == 1.0 and single_cluster["homogeneity"] == 0.0


def test_cluster_report_refusals():
    from cuda_gcn_amd.model import cluster_report, GcnHostError
    with pytest.raises(GcnHostError, match="cluster_report: a negative count"):
        cluster_report(np.array([[1, -1], [2, 3]]))
    for bad in (np.zeros(4, np.int64), np.zeros((0, 3), np.int64), np.zeros((2, 0), np.int64)):
        with pytest.raises(GcnHostError, match="cluster_report"):
            cluster_report(bad)


def test_reference_draw_is_philox():
    """the function the seeding reference draws from reproduces Random123's known answers, and seed_word is its word 0 at the
    counter {i, 0, t, 0x6B6D2B2B} under the key {lo32, hi32}"""
    for ctr, key, out in dropout_ref.KNOWN_ANSWERS:
        assert tuple(int(v) for v in dropout_ref.philox4x32_10(ctr, key)) == out
    s = 0x0123456789ABCDEF
    i = np.array([0, 1, 77, 2 ** 31 - 1], np.uint64)
    w = R.seed_word(i, 5, s)
    for j, v in zip(i, w):
        assert int(v) == int(dropout_ref.philox4x32_10((int(j), 0, 5, 0x6B6D2B2B), (0x89ABCDEF, 0x01234567))[0])
    assert len(set(int(v) for v in R.seed_word(np.arange(1000), 1, s))) > 990
    from cuda_gcn_amd.model import KEY_KMEANS
    hdr = open(os.path.join(ROOT, "cuda_gcn_amd", "host", "module.h")).read()
    assert int(re.search(r"KEY_KMEANS = (0x[0-9A-Fa-f]+)ull", hdr).group(1), 16) == KEY_KMEANS == R.KEY_KMEANS


def up256(b):
    return (b + 255) // 256 * 256


@pytest.mark.parametrize("n,k,dim", [(0, 1, 1), (1000, 7, 5), (1000, 256, 256), (232965, 41, 128), (1025, 64, 17)])
def test_plan_byte_counts(n, k, dim):
    """update: {histograms [chunks of 1024 x k] | two start tables [k + 1] | the member list [n] | chunk sums | float64 rows
    [k x dim]} each rounded up to 256 bytes, then segment partials of dim doubles: n // 128 + k of them (at least 64), at least
    64; seeding: d2min [n] and 1024 (key, position) slots"""
    from cuda_gcn_amd import _lib
    lib = _lib.gcnhip()
    a, b, s = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert lib.gcnhip_kmeans_plan(n, k, dim, C.byref(a), C.byref(b), C.byref(s)) == 0
    chunks = max(-(-n // 1024), 1)
    fixed = up256(chunks * k * 4) + up256(2 * (k + 1) * 4) + up256(max(n, 1) * 4) + up256(chunks * 8) + up256(k * dim * 8)
    assert a.value == fixed + dim * 8 * max(n // 128 + k, 64)
    assert b.value == fixed + dim * 8 * 64
    assert s.value == up256(max(n, 1) * 4) + up256(1024 * 8) + up256(1024 * 4)
    assert a.value >= b.value
    for bad in ((-1, 4, 4), (10, 0, 4), (10, 257, 4), (10, 4, 0), (10, 4, 257)):
        assert lib.gcnhip_kmeans_plan(*bad, None, None, None) == -1
        assert b"gcnhip_kmeans_plan" in lib.gcnhip_last_error()


def test_abi_tables_hold_the_new_entry_points():
    from cuda_gcn_amd import _lib
    hip, host = _lib.gcnhip(), _lib.gcnhost()
    drv = open(os.path.join(ROOT, "include", "gcnhip_driver.h")).read()
    hst = open(os.path.join(ROOT, "include", "gcnhost.h")).read()
    for n in ("gcnhip_kmeans_plan", "gcnhip_kmeans_assign", "gcnhip_kmeans_update", "gcnhip_kmeans_seed", "gcnhip_contingency_rows"):
        assert n in _lib.GCNHIP_SYMBOLS and hasattr(hip, n) and re.search(rf"\bint {n}\(", drv), n
    for n in ("gcnhost_model_kmeans", "gcnhost_cluster_report"):
        assert n in _lib.GCNHOST_SYMBOLS and hasattr(host, n) and re.search(rf"\bint {n}\(", hst), n
