"""float64 numpy reference of split conformal prediction as the GPU path computes it (no GPU here): the conformity scores of
csrc/conformal.hip (LAC and APS / RAPS), their diffusion over the graph, the true-class scores, the quantile rule of
host/conformal.h, the sets and their counts — each score with an ERROR BOUND for the f32 kernels, so that no tolerance has
to be guessed.

Inputs are log-softmax rows l (f32 values, read exactly) and an f32 beta = 1 / T; p = softmax(beta . l) and its bound dp are
calib_ref._softmax's.  rank_j = #{k : l_k > l_j, or l_k == l_j and k < j} is taken on the f32 inputs by both sides: exact.

Error bounds (u = 2^-24; DESIGN §2: one f32 sum of terms t_i in any order is within 8 u sum |t_i| of the real sum):
  LAC   s_j = 1 - p_j, one rounded difference of values <= 1:                       E = dp_j + 2 u
  APS   s_j = cum_j + pen_j with cum_j = sum_{rank_k <= rank_j} p_k clamped to 1 (the clamp moves towards the real sum, which
        never exceeds 1), pen_j = lam . max(0, rank_j + 1 - k_reg) one rounded product of an exact integer, and one rounded sum:
                                                                                    E = sum_{rank_k <= rank_j} dp_k + 8 u cum_j + 2 u (|pen_j| + |s_j|)
        The last-ranked class has cum = 1 exactly on both sides.
  diffusion   S' = d . A^ . S + (1 - d) . S is linear: E' = d |A^| E + (1 - d) E plus the blend's own rounding
              8 u (d |A^| |S| + (1 - d) |S|), which is smooth_ref.propagate's recurrence for one step started from b0 = E.
  quantile    an order statistic is 1-Lipschitz in the sup norm: |q_gpu - q_ref| <= the largest E of the scores it was taken from.
  sets        class j is in the set iff s_j <= thresh_j; an entry is AMBIGUOUS iff |s_ref - thresh| <= E: only there may an f32
              kernel decide otherwise."""
import math

import numpy as np

from tests import calib_ref
from tests import smooth_ref

U = calib_ref.U
LAC, APS = 0, 1


def ranks(logp):
    """int64 [n, C]: rank_j = #{k : l_k > l_j, or l_k == l_j and k < j} — a stable sort of -l"""
    l = np.asarray(logp, np.float64)
    order = np.argsort(-l, axis=1, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(l.shape[1]), l.shape), axis=1)
    return rank


def scores(logp, beta, method, lam=0.0, k_reg=0):
    """(S, E, rank) [n, C]: the scores of every class of every row, their f32 bound, the ranks"""
    l = np.asarray(logp, np.float64)
    n, c = l.shape
    _, _, p, _, _, dp, _ = calib_ref._softmax(l, calib_ref.f32(beta))
    rank = ranks(l)
    if method == LAC:
        return 1.0 - p, dp + 2 * U, rank
    order = np.argsort(rank, axis=1)                                  # order[:, i] = the class of rank i
    cum = np.take_along_axis(np.cumsum(np.take_along_axis(p, order, axis=1), axis=1), rank, axis=1)
    cdp = np.take_along_axis(np.cumsum(np.take_along_axis(dp, order, axis=1), axis=1), rank, axis=1)
    cum = np.minimum(cum, 1.0)
    cum[rank == c - 1] = 1.0
    pen = calib_ref.f32(lam) * np.maximum(0, rank + 1 - int(k_reg))
    s = cum + pen
    return s, cdp + 8 * U * cum + 2 * U * (np.abs(pen) + np.abs(s)), rank


def diffuse(csr, s, e, d):
    """(S', E'): d . A^ . S + (1 - d) . S with the bound pushed through (d is the f32 value the launch takes)"""
    d = calib_ref.f32(d)
    out, bound = smooth_ref.propagate(csr, s, d, 1, b0=e)
    return out, bound


def listed(n_table, rows):
    """(ids int64 in list order, inside: which of them are rows of the table)"""
    idx = np.arange(n_table) if rows is None else np.asarray(rows, np.int64).ravel()
    return idx, (idx >= 0) & (idx < n_table)


def true_scores(s, e, truth, rows=None):
    """(score, bound) per list position: s[r, truth[r]], or -1 (bound 0) when r is outside the table or truth[r] outside [0, C)"""
    s = np.asarray(s, np.float64)
    n, c = s.shape
    idx, inside = listed(n, rows)
    truth = np.asarray(truth, np.int64)
    out, bound = np.full(idx.size, -1.0), np.zeros(idx.size)
    r = idx[inside]
    t = truth[r]
    ok = (t >= 0) & (t < c)
    pos = np.flatnonzero(inside)[ok]
    out[pos], bound[pos] = s[r[ok], t[ok]], np.asarray(e, np.float64)[r[ok], t[ok]]
    return out, bound


def quantile_k(n, alpha):
    """k = ceil((n + 1)(1 - alpha)) in float64: host/conformal.h's expression"""
    return int(math.ceil(float(n + 1) * (1.0 - float(alpha))))


def quantile(sc, alpha):
    """(q, k, n'): negative scores dropped, the k-th smallest of the n' left, +inf when k > n'"""
    sc = np.asarray(sc, np.float64).ravel()
    kept = np.sort(sc[sc >= 0])
    k = quantile_k(kept.size, alpha)
    return (float(kept[k - 1]) if k <= kept.size else math.inf), k, int(kept.size)


def quantile_per_class(sc, labels, num_classes, alpha):
    """(thresh [C], k [C], n_cal [C]): the rule on the scores of every label"""
    sc, labels = np.asarray(sc, np.float64).ravel(), np.asarray(labels, np.int64).ravel()
    out = [quantile(sc[labels == c], alpha) for c in range(num_classes)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out], np.int64), np.array([o[2] for o in out], np.int64)


def sets(s, e, thresh, truth=None, rows=None):
    """dict: member bool [n listed, C] (all False for an id outside the table), size int32 (-1 there), ambiguous bool [n listed, C],
    counts int64 [4 + 3 C + 1] = {rows in the table, labelled, covered, empty | size_hist [C + 1] | class_support [C] |
    class_covered [C]} and amb_rows: the listed rows with an ambiguous entry (each may move any count it takes part in by one)"""
    s, e = np.asarray(s, np.float64), np.asarray(e, np.float64)
    n, c = s.shape
    th = np.broadcast_to(np.asarray(thresh, np.float64), (c,))
    idx, inside = listed(n, rows)
    member = np.zeros((idx.size, c), bool)
    amb = np.zeros((idx.size, c), bool)
    r = idx[inside]
    member[inside] = s[r] <= th
    amb[inside] = np.abs(s[r] - th) <= e[r]                          # (a threshold of +inf is infinitely far: never ambiguous)
    size = np.where(inside, member.sum(axis=1), -1).astype(np.int32)
    counts = np.zeros(4 + 3 * c + 1, np.int64)
    counts[0] = inside.sum()
    counts[3] = (size == 0).sum()
    counts[4:4 + c + 1] = np.bincount(size[inside], minlength=c + 1)
    if truth is not None:
        t = np.full(idx.size, -1, np.int64)
        t[inside] = np.asarray(truth, np.int64)[r]
        lab = inside & (t >= 0) & (t < c)
        hit = np.zeros(idx.size, bool)
        hit[lab] = member[lab, t[lab]]
        counts[1], counts[2] = lab.sum(), hit.sum()
        counts[4 + c + 1:4 + 2 * c + 1] = np.bincount(t[lab], minlength=c)
        counts[4 + 2 * c + 1:] = np.bincount(t[hit], minlength=c)
    return dict(member=member, size=size, ambiguous=amb, counts=counts, amb_rows=int(amb.any(axis=1).sum()))


def brute_force_scores(logp, beta, method, lam=0.0, k_reg=0):
    """the definitions spelled out class by class (slow; what scores() is checked against)"""
    l = np.asarray(logp, np.float64)
    n, c = l.shape
    b = calib_ref.f32(beta)
    out = np.zeros((n, c))
    for r in range(n):
        z = b * l[r]
        p = np.exp(z - z.max())
        p = p / p.sum()
        for j in range(c):
            before = [k for k in range(c) if l[r, k] > l[r, j] or (l[r, k] == l[r, j] and k < j)]
            if method == LAC:
                out[r, j] = 1.0 - p[j]
                continue
            rank = len(before)
            # the classes ranked before j, best first, then j itself
            chain = sorted(before, key=lambda k: (-l[r, k], k)) + [j]
            cum = 1.0 if rank == c - 1 else min(float(np.sum(p[chain])), 1.0)
            out[r, j] = cum + calib_ref.f32(lam) * max(0, rank + 1 - int(k_reg))
    return out


def make_case(n, c, seed):
    """test_calibration_gpu.make_case's rows (from 5 rows on: a column at -1e4 in row 3, an exact tie for the maximum in row 4,
    truth -1 in row 1 and >= C in row 2) with the truth otherwise DRAWN FROM EACH ROW'S SOFTMAX, as a model's labels are:
    independent random labels would push every threshold to the full-set score"""
    from tests.test_calibration_gpu import make_case as calib_case
    logp, truth = calib_case(n, c, seed)
    p = np.exp(logp.astype(np.float64))
    cdf = np.cumsum(p / p.sum(axis=1, keepdims=True), axis=1) if n else np.zeros((0, c))
    draw = np.random.default_rng(seed + 1000).random(n)
    drawn = np.minimum((cdf < draw[:, None]).sum(axis=1), c - 1).astype(np.int32)
    special = np.zeros(n, bool)
    if n >= 5:
        special[[1, 2, 4]] = True
    return logp, np.where(special, truth, drawn).astype(np.int32)
