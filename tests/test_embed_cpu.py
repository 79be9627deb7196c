"""The acceptance rule of tests/embed_ref.py, tested on the CPU: it passes the float32 numpy answer of the same definition and
rejects each kind of wrong answer a top-k kernel can give.  (A checker that accepted everything would hide a wrong kernel.)
The host entry points refuse nothing without a device — every refusal of embed / similar / score_pairs needs a built model —
so those are in tests/test_embed_gpu.py."""
import numpy as np
import pytest

from tests import embed_ref as R

K = 10


def make_table(n=200, dim=16, seed=0):
    """standard-normal rows after a ReLU; row 1 all zero; rows 3 and 7 equal, long and almost parallel to row 0, so that query 0
    has an exact tie at the top of its list under both metrics"""
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((n, dim)), 0).astype(np.float32)
    x[1] = 0
    x[3] = 3 * x[0] + np.float32(0.01) * np.abs(rng.standard_normal(dim)).astype(np.float32)
    x[7] = x[3]
    return x


@pytest.fixture(scope="module", params=["dot", "cosine"])
def case(request):
    x = make_table()
    metric = request.param
    q_rows = [0, 1, 5, 5, 199]
    ids, scores = R.topk_f32(x, q_rows, K, metric)
    return x, metric, q_rows, ids, scores


def judge(case, i, ids, scores, **kw):
    x, metric, q_rows, _, _ = case
    s64, E = R.scores64(x, q_rows[i], metric)
    R.check_query(ids, scores, q_rows[i], s64, E, **kw)
    return s64, E


def test_the_checker_passes_the_float32_answer(case):
    x, metric, q_rows, ids, scores = case
    R.check_topk(x, q_rows, ids, scores, metric)
    perm = np.random.default_rng(1).permutation(x.shape[0]).astype(np.int32)
    pi, ps = R.topk_f32(x, q_rows, K, metric, row_id=perm)
    R.check_topk(x, q_rows, pi, ps, metric, row_id=perm)
    assert not np.array_equal(pi, perm[ids])                      # the tie of rows 3 and 7 is broken by id, not by row
    ai, as_ = R.topk_f32(x, q_rows, K, metric, exclude_self=False)
    R.check_topk(x, q_rows, ai, as_, metric, exclude_self=False)
    few_i, few_s = R.topk_f32(x[:6], [2], K, metric)              # 5 candidates for 10 slots
    assert np.all(few_i[0, 5:] == -1) and np.all(np.isneginf(few_s[0, 5:]))
    R.check_topk(x[:6], [2], few_i, few_s, metric)


def test_two_untied_neighbours_swapped_are_rejected(case):
    _, _, _, ids, scores = case
    i, s = ids[2].copy(), scores[2].astype(np.float64)
    assert s[4] > s[5]
    i[[4, 5]], s[[4, 5]] = i[[5, 4]], s[[5, 4]]
    with pytest.raises(AssertionError, match="rule 3"):
        judge(case, 2, i, s)
    i, s = ids[2].copy(), scores[2].astype(np.float64)            # the ids alone: each score then belongs to the other row
    i[[4, 5]] = i[[5, 4]]
    with pytest.raises(AssertionError, match="rule 2"):
        judge(case, 2, i, s)


def test_a_better_candidate_left_out_is_rejected(case):
    x, metric, q_rows, _, _ = case
    ids, scores = R.topk_f32(x, q_rows, K + 1, metric)
    i, s = np.delete(ids[2], 3), np.delete(scores[2], 3)          # the 4th best dropped, the 11th best let in
    with pytest.raises(AssertionError, match="rule 4"):
        judge(case, 2, i, s)


def test_the_query_returned_under_exclude_self_is_rejected(case):
    x, metric, q_rows, ids, scores = case
    full_i, full_s = R.topk_f32(x, q_rows, K, metric, exclude_self=False)
    assert q_rows[2] in full_i[2]
    with pytest.raises(AssertionError, match="rule 1"):
        judge(case, 2, full_i[2], full_s[2])
    judge(case, 2, full_i[2], full_s[2], exclude_self=False)
    i = ids[2].copy()
    i[6] = i[5]
    with pytest.raises(AssertionError, match="rule 1"):           # and an id twice
        judge(case, 2, i, scores[2])


def test_a_tie_in_descending_id_order_is_rejected(case):
    _, _, _, ids, scores = case
    i, s = ids[0].copy(), scores[0]
    a, b = int(np.flatnonzero(i == 3)[0]), int(np.flatnonzero(i == 7)[0])
    assert b == a + 1 and s[a] == s[b]
    i[[a, b]] = i[[b, a]]
    with pytest.raises(AssertionError, match="rule 3"):
        judge(case, 0, i, s)


def test_a_score_off_by_three_bounds_is_rejected(case):
    x, metric, q_rows, ids, scores = case
    s64, E = R.scores64(x, q_rows[2], metric)
    s = scores[2].astype(np.float64)
    s[K - 1] -= 3 * E[ids[2, K - 1]]
    with pytest.raises(AssertionError, match="rule 2"):
        judge(case, 2, ids[2], s)
    s = scores[2].astype(np.float64)
    s[0] += 3 * E[ids[2, 0]]
    with pytest.raises(AssertionError, match="rule 2"):
        judge(case, 2, ids[2], s)


def test_bounds_and_norms_of_the_reference():
    x = make_table()
    r = R.inv_norms64(x)
    assert r[1] == 0 and np.allclose(r[[0, 2]] * np.sqrt((x[[0, 2]].astype(np.float64) ** 2).sum(axis=1)), 1, rtol=1e-15)
    s, E = R.pair_scores64(x, [0, 1, 3], [0, 5, 7], "cosine")
    assert abs(s[0] - 1) <= 1e-15 and s[1] == 0 and E[1] == 0 and abs(s[2] - 1) <= 1e-15
    assert E[0] == pytest.approx((2 * 16 + 16) * R.U)
    assert R.near_ties(x, [0], 1, "dot") == 1 and R.near_ties(x, [5], 1, "dot") == 0      # rows 3 and 7 tie for query 0's first place
    group = np.arange(200) % 4
    assert R.own_group_share(np.array([[4, 8, 1, -1]]), group, [0]).tolist() == [2 / 3]
    assert R.topk64(x, [0], 2, "cosine").tolist() == [[3, 7]]
