"""Split conformal prediction without a GPU: the quantile rule of host/conformal.h through its C entry point and the Python
binding, against the reference's; the reference of tests/conformal_ref.py against definitions spelled out; the finite-sample
identity; refusals of the host functions; the binding tables."""
import math

import numpy as np
import pytest

from tests import conformal_ref as R


def cq(*a, **kw):
    from cuda_gcn_amd.model import conformal_quantile
    return conformal_quantile(*a, **kw)


def test_quantile_rule():
    """k > n gives +inf, negatives are dropped, ties, n = 0"""
    assert cq([], 0.1) == dict(threshold=math.inf, n_cal=0, k=1)
    assert cq([-1.0, -1.0], 0.5) == dict(threshold=math.inf, n_cal=0, k=1)
    s = np.array([0.9, 0.1, -1.0, 0.5, 0.3, -1.0, 0.7], np.float32)          # five kept
    assert cq(s, 0.5) == dict(threshold=float(np.float32(0.5)), n_cal=5, k=3)  # ceil(6 . 0.5) = 3
    assert cq(s, 0.2) == dict(threshold=float(np.float32(0.9)), n_cal=5, k=5)  # ceil(6 . 0.8) = 5
    got = cq(s, 0.1)                                                           # ceil(6 . 0.9) = 6 > 5
    assert got["threshold"] == math.inf and got["k"] == 6 and got["n_cal"] == 5
    ties = np.array([0.25, 0.5, 0.5, 0.5, 0.75], np.float32)
    for alpha, want in ((0.7, 0.5), (0.5, 0.5), (0.4, 0.5), (0.3, 0.75)):     # k = 2, 3, 4, 5
        assert cq(ties, alpha)["threshold"] == want
    assert cq([0.0, 0.0], 0.5)["threshold"] == 0.0                             # a score of zero is a score


def test_python_and_c_agree_on_k_and_on_the_quantile():
    rng = np.random.default_rng(0)
    for alpha in (0.1, 0.3, 0.5):
        for n in range(0, 201):
            s = rng.random(n).astype(np.float32)
            got = cq(s, alpha)
            q, k, kept = R.quantile(s, alpha)
            assert got["k"] == k == R.quantile_k(n, alpha) and got["n_cal"] == kept == n, (alpha, n)
            assert got["threshold"] == q, (alpha, n)
            # the finite-sample identity: at least k calibration scores are <= q (and k - 1 < (n + 1)(1 - alpha) <= k)
            assert k - 1 < (n + 1) * (1 - alpha) <= k
            if k <= n:
                assert (s <= got["threshold"]).sum() >= k and (s < got["threshold"]).sum() < k


def test_per_class_grouping():
    rng = np.random.default_rng(1)
    c = 5
    s = rng.random(300).astype(np.float32)
    lab = rng.integers(-1, c + 1, 300).astype(np.int32)                       # -1 and c: outside, dropped
    s[rng.random(300) < 0.1] = -1.0
    lab[lab == 3] = 2                                                         # class 3 has no rows
    got = cq(s, 0.2, labels=lab, num_classes=c)
    th, k, n_cal = R.quantile_per_class(s, lab, c, 0.2)
    assert np.array_equal(got["threshold"].astype(np.float64), th) and np.array_equal(got["k"], k) and np.array_equal(got["n_cal"], n_cal)
    assert got["threshold"][3] == math.inf and got["n_cal"][3] == 0
    for j in range(c):
        mine = s[(lab == j) & (s >= 0)]
        assert n_cal[j] == mine.size and (k[j] > mine.size or (mine <= th[j]).sum() >= k[j])


def test_host_refusals():
    from cuda_gcn_amd.model import GcnHostError
    for alpha in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(GcnHostError, match=r"conformal_quantile: alpha must be in \(0, 1\)"):
            cq([0.5], alpha)
    with pytest.raises(GcnHostError, match="conformal_quantile: a score is NaN"):
        cq([0.5, float("nan")], 0.1)
    with pytest.raises(GcnHostError, match="conformal_quantile: 1 <= num_classes <= 64"):
        cq([0.5], 0.1, labels=[0], num_classes=65)
    with pytest.raises(GcnHostError, match="conformal_quantile: 2 labels for 1 scores"):
        cq([0.5], 0.1, labels=[0, 1], num_classes=2)


@pytest.mark.parametrize("c", [2, 7, 41])
def test_reference_scores_and_sets_against_the_definitions(c):
    """scores() (vectorised) against the class-by-class definitions; ranks are a permutation with ties to the lower class; the
    last rank scores exactly 1 (+ its penalty); sets and counts against loops"""
    logp, truth = R.make_case(17, c, 9)
    rank = R.ranks(logp)
    assert np.array_equal(np.sort(rank, axis=1), np.broadcast_to(np.arange(c), (17, c)))
    tied = np.flatnonzero(logp[4] == logp[4].max())                            # row 4: classes 0, C - 1 and the row's own maximum
    assert tied[0] == 0 and tied[-1] == c - 1 and rank[4, tied].tolist() == list(range(tied.size))     # the lower class first
    for beta in (0.25, 1.0, 4.0):
        for method, lam, k_reg in ((R.LAC, 0.0, 0), (R.APS, 0.0, 0), (R.APS, 0.01, 2)):
            s, e, _ = R.scores(logp, beta, method, lam, k_reg)
            want = R.brute_force_scores(logp, beta, method, lam, k_reg)
            assert np.all(np.abs(s - want) <= 1e-14), (beta, method)
            assert np.all(e > 0) and e.max() < 1e-4
            if method == R.APS:
                pen = R.calib_ref.f32(lam) * max(0, c - k_reg)
                assert np.all(s[rank == c - 1] == 1.0 + pen)
                assert np.all(np.diff(np.take_along_axis(s, np.argsort(rank, axis=1), axis=1), axis=1) >= 0)      # grows with the rank
            rows = [16, 3, 3, -1, 17, 0, 4, 99, 2, 1, 3]
            for th in (0.5, 0.9, math.inf):
                st = R.sets(s, e, th, truth, rows)
                counts = np.zeros(4 + 3 * c + 1, np.int64)
                for i, r in enumerate(rows):
                    if not 0 <= r < 17:
                        assert st["size"][i] == -1 and not st["member"][i].any()
                        continue
                    members = [j for j in range(c) if s[r, j] <= th]
                    assert np.flatnonzero(st["member"][i]).tolist() == members and st["size"][i] == len(members)
                    counts[0] += 1
                    counts[3] += not members
                    counts[4 + len(members)] += 1
                    if 0 <= truth[r] < c:
                        counts[1] += 1
                        counts[2] += truth[r] in members
                        counts[4 + c + 1 + truth[r]] += 1
                        counts[4 + 2 * c + 1 + truth[r]] += truth[r] in members
                assert np.array_equal(st["counts"], counts)
                if th == math.inf:
                    assert np.all(st["size"][st["size"] >= 0] == c) and not st["ambiguous"].any()
            ts, tb = R.true_scores(s, e, truth, rows)
            for i, r in enumerate(rows):
                ok = 0 <= r < 17 and 0 <= truth[r] < c
                assert ts[i] == (s[r, truth[r]] if ok else -1.0) and tb[i] == (e[r, truth[r]] if ok else 0.0)


def test_reference_coverage_guarantee_on_its_own_calibration_rows():
    """with the threshold of the rule, at least k of the calibration rows are covered — on the reference's own scores"""
    logp, truth = R.make_case(4001, 7, 2)
    for method in (R.LAC, R.APS):
        s, e, _ = R.scores(logp, 1.0, method)
        ts, _ = R.true_scores(s, e, truth)
        for alpha in (0.1, 0.3):
            q, k, n = R.quantile(ts, alpha)
            st = R.sets(s, e, q, truth)
            assert n == st["counts"][1] and st["counts"][2] == (ts[ts >= 0] <= q).sum() >= k
            assert st["counts"][2] / n >= 1 - alpha


def test_binding_tables_name_the_new_entry_points():
    from cuda_gcn_amd import _lib
    hip, host = _lib.gcnhip(), _lib.gcnhost()
    for n in ("gcnhip_conformal_scores", "gcnhip_conformal_true_scores", "gcnhip_conformal_sets_rows"):
        assert n in _lib.GCNHIP_SYMBOLS and hasattr(hip, n)
    for n in ("gcnhost_model_conformal_fit", "gcnhost_model_conformal_sets", "gcnhost_conformal_quantile"):
        assert n in _lib.GCNHOST_SYMBOLS and hasattr(host, n)


def test_struct_layout_matches_the_header():
    """gcnhost_conformal as ctypes lays it out: the offsets a C compiler gives the header's struct"""
    import ctypes as C
    from cuda_gcn_amd.model import _ConformalFit as F
    assert (F.method.offset, F.lam.offset, F.k_reg.offset, F.diffusion.offset, F.temperature.offset) == (0, 4, 8, 12, 16)
    assert (F.alpha.offset, F.per_class.offset, F.thresh.offset, F.n_cal.offset) == (24, 32, 36, 296)
    assert C.sizeof(F) == 296 + 64 * 8
