"""Float64 reference for the embedding kernels (csrc/embed.hip) and the acceptance rule their answers are held to.

Score of rows (q, c) of a table x [n, dim]: metric "dot": sum_j x_qj x_cj; metric "cosine": that times r_q r_c with
r = 1 / sqrt(sum_j x_rj^2), or 0 for an all-zero row.  s64 is the score in float64.

The bound.  With u = 2^-24 (half an ulp of f32, relative):

    E(q, c) = (2 dim + 16) . u . sum_j |x_qj x_cj| . r_q r_c          (r = 1 for dot)

Where it comes from:
  * dim . u for the f32 dot product summed in ANY order (each of the dim products rounds once, each of the at most dim adds
    rounds once: the classical bound (dim . u) . sum |a_j b_j| to first order);
  * dim . u / 2 + 2 u per inverse norm: the sum of squares carries dim . u relative (same argument, all terms positive), the
    square root halves a relative error, and the correctly rounded square root and division add u each — twice, for r_q and r_c:
    dim . u + 4 u together;
  * 2 u for the two multiplies (dot . r_q) . r_c;
  * the remaining 10 u are slack for the second-order terms (the products of the errors above, at most (2 dim + 6)^2 u^2 <
    u for dim <= 256).
For "dot" only the first line applies and the bound is that much more generous.

The acceptance rule for one query q with answer (id_0 .. id_{k-1}, score_0 .. score_{k-1}) needs no cap on ambiguous cases:
  1. the returned ids are distinct, name rows of the table, and are not the query when it is excluded; with m < k candidates
     exactly the first m slots are filled and the rest hold -1 / -inf;
  2. |score_i - s64(q, id_i)| <= E(q, id_i);
  3. the scores are non-increasing, and equal scores have ascending ids;
  4. every candidate c that was not returned has s64(q, c) <= score_{k-1} + E(q, c).
"""
import numpy as np

U = 2.0 ** -24


def inv_norms64(x):
    """float64 1 / sqrt(sum of squares) of every row, 0 for an all-zero row"""
    s = (np.asarray(x, np.float64) ** 2).sum(axis=1)
    return np.where(s > 0, 1.0 / np.sqrt(np.where(s > 0, s, 1.0)), 0.0)


def inv_norm_bound(dim):
    """relative error allowed to an f32 inverse norm: (dim / 2 + 2) . u"""
    return (dim / 2 + 2) * U


def scores64(x, q, metric, r=None):
    """(s64 [n], E [n]) of query row q against every row of x (float64 [n, dim]); r = inv_norms64(x) for cosine"""
    x = np.asarray(x, np.float64)
    dim = x.shape[1]
    s = x @ x[q]
    a = np.abs(x) @ np.abs(x[q])
    if metric == "cosine":
        r = inv_norms64(x) if r is None else r
        s, a = s * r * r[q], a * r * r[q]
    elif metric != "dot":
        raise ValueError(metric)
    return s, (2 * dim + 16) * U * a


def pair_scores64(x, src, dst, metric):
    """(s64 [m], E [m]) of the listed row pairs"""
    x = np.asarray(x, np.float64)
    dim = x.shape[1]
    s = (x[src] * x[dst]).sum(axis=1)
    a = np.abs(x[src] * x[dst]).sum(axis=1)
    if metric == "cosine":
        r = inv_norms64(x)
        s, a = s * r[src] * r[dst], a * r[src] * r[dst]
    elif metric != "dot":
        raise ValueError(metric)
    return s, (2 * dim + 16) * U * a


def topk_f32(x, q_rows, k, metric, row_id=None, exclude_self=True):
    """The same definition carried out in float32 numpy: (ids int32 [nq, k], scores f32 [nq, k]), -1 / -inf past the candidates."""
    x = np.asarray(x, np.float32)
    n = x.shape[0]
    ids_of = np.arange(n, dtype=np.int32) if row_id is None else np.asarray(row_id, np.int32)
    if metric == "cosine":
        s2 = (x * x).sum(axis=1, dtype=np.float32)
        inv = np.where(s2 > 0, np.float32(1) / np.sqrt(np.where(s2 > 0, s2, np.float32(1)), dtype=np.float32), np.float32(0)).astype(np.float32)
    out_i = np.full((len(q_rows), k), -1, np.int32)
    out_s = np.full((len(q_rows), k), -np.inf, np.float32)
    for i, q in enumerate(q_rows):
        s = (x @ x[q]).astype(np.float32)
        if metric == "cosine":
            s = (s * inv[q]).astype(np.float32) * inv
        cand = np.flatnonzero(np.arange(n) != q) if exclude_self else np.arange(n)
        order = cand[np.lexsort((ids_of[cand], -s[cand]))][:k]
        out_i[i, :order.size] = ids_of[order]
        out_s[i, :order.size] = s[order]
    return out_i, out_s


def check_query(ids, scores, q, s64, E, row_id=None, exclude_self=True):
    """The acceptance rule for one query row q; s64, E = scores64(x, q, ...).  Raises AssertionError naming the clause."""
    n = s64.shape[0]
    k = len(ids)
    ids = np.asarray(ids, np.int64)
    scores = np.asarray(scores, np.float64)
    ids_of = np.arange(n, dtype=np.int64) if row_id is None else np.asarray(row_id, np.int64)
    row_of = np.full(int(ids_of.max()) + 1 if n else 0, -1, np.int64)
    row_of[ids_of] = np.arange(n)
    cand = np.ones(n, bool)
    if exclude_self:
        cand[q] = False
    m = min(k, int(cand.sum()))
    # 1
    assert np.all(ids[m:] == -1) and np.all(np.isneginf(scores[m:])), f"rule 1: slots past the {m} candidates are not -1 / -inf"
    got = ids[:m]
    assert np.all((got >= 0) & (got < row_of.size)), "rule 1: an id outside the table"
    rows = row_of[got]
    assert np.all(rows >= 0), "rule 1: an id that names no row"
    assert np.unique(got).size == m, "rule 1: an id returned twice"
    assert not (exclude_self and np.any(rows == q)), "rule 1: the query itself was returned"
    # 2
    err = np.abs(scores[:m] - s64[rows])
    assert np.all(err <= E[rows]), f"rule 2: a score is off by {float((err - E[rows]).max()):.3e} beyond its bound"
    # 3
    d = np.diff(scores[:m])
    assert np.all(d <= 0), "rule 3: the scores increase somewhere"
    assert np.all(np.diff(got)[d == 0] > 0), "rule 3: equal scores whose ids do not ascend"
    # 4
    if m:
        left = cand.copy()
        left[rows] = False
        over = s64[left] - (scores[m - 1] + E[left])
        assert not np.any(over > 0), f"rule 4: a candidate left out beats the last returned score by {float(over.max()):.3e} beyond its bound"


def check_topk(x, q_rows, ids, scores, metric, row_id=None, exclude_self=True):
    """the rule for every query of an answer [nq, k]"""
    x64 = np.asarray(x, np.float64)
    r = inv_norms64(x64) if metric == "cosine" else None
    for i, q in enumerate(q_rows):
        s64, E = scores64(x64, q, metric, r)
        check_query(ids[i], scores[i], q, s64, E, row_id, exclude_self)


def near_ties(x, q_rows, k, metric, exclude_self=True):
    """number of queries whose k-th and (k+1)-th reference scores lie within 2 E of each other: the queries whose answer SET the
    bound leaves open"""
    x64 = np.asarray(x, np.float64)
    r = inv_norms64(x64) if metric == "cosine" else None
    count = 0
    for q in q_rows:
        s64, E = scores64(x64, q, metric, r)
        if exclude_self:
            s64, E = np.delete(s64, q), np.delete(E, q)
        if s64.size <= k:
            continue
        order = np.argsort(-s64, kind="stable")
        a, b = order[k - 1], order[k]
        count += bool(s64[a] - s64[b] <= E[a] + E[b])
    return count


def own_group_share(ids, group, q_rows):
    """per query: the share of its returned neighbours (ids >= 0) that carry the query's group"""
    ids = np.asarray(ids)
    same = (group[np.where(ids >= 0, ids, 0)] == group[np.asarray(q_rows)][:, None]) & (ids >= 0)
    return same.sum(axis=1) / np.maximum((ids >= 0).sum(axis=1), 1)


def topk64(x, q_rows, k, metric, exclude_self=True):
    """ids [nq, k] of the float64 reference (ties by ascending row)"""
    x64 = np.asarray(x, np.float64)
    r = inv_norms64(x64) if metric == "cosine" else None
    out = np.full((len(q_rows), k), -1, np.int64)
    for i, q in enumerate(q_rows):
        s64, _ = scores64(x64, q, metric, r)
        order = np.lexsort((np.arange(s64.size), -s64))
        order = (order[order != q] if exclude_self else order)[:k]
        out[i, :order.size] = order
    return out
