"""numpy reference of the multi-label decision thresholds (csrc/thresholds.hip): the rule and the fit, on the keys of
tests/ranking_ref.py.

  rule   class c is predicted for a row when its logit z is not NaN and key(z) >= key(t[c])
  fit    candidates = the keys k of the class's positives; TP = #{pos >= k}, FP = #{neg >= k}, FN = P - TP;
         w = beta * beta; num = (1.0 + w) * TP; den = num + w * FN + FP; F = num / den   (float64, in this order, no fused step)
         winner: the largest F, among equal F the largest key.  P == 0: defined = 0, threshold 0.0, TP = FN = 0,
         FP = #{neg >= key(0)}, F = 0.

Python floats are IEEE float64 and every operation is rounded once, so f_beta() below is the expression the kernel evaluates
bit for bit.  brute_fit() is the definition the fit is checked against: every distinct score as a cut, in float comparison."""
import numpy as np

from tests import ranking_ref as R

KEY_ZERO = 0x80000000


def key_to_float(k):
    """the float32 a key came from (+0.0 for the key of either zero)"""
    k = np.asarray(k, np.uint32)
    return np.where(k >> 31 == 1, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def f_beta(tp, fp, fn, beta):
    if tp == 0:
        return 0.0
    w = float(beta) * float(beta)
    num = (1.0 + w) * float(int(tp))
    den = num + w * float(int(fn)) + float(int(fp))
    return num / den


def sorted_fit(pk, nk, beta=1.0):
    """(threshold float32, defined, tp, fp, fn, f) from the sorted keys of a class's positives and negatives"""
    P, N = int(pk.size), int(nk.size)
    if P == 0:
        return np.float32(0.0), 0, 0, N - int(np.searchsorted(nk, np.uint32(KEY_ZERO), "left")), 0, 0.0
    best = None
    for k in np.unique(pk):
        tp = P - int(np.searchsorted(pk, k, "left"))
        fp = N - int(np.searchsorted(nk, k, "left"))
        cand = (f_beta(tp, fp, P - tp, beta), int(k), tp, fp)
        if best is None or cand[:2] > best[:2]:
            best = cand
    f, k, tp, fp = best
    return key_to_float(np.uint32(k))[()], 1, tp, fp, P - tp, f


def fit_columns(pos_keys, neg_keys, beta=1.0):
    """sorted_fit over lists of sorted key arrays -> dict of arrays: threshold f32, defined int32, tp / fp / fn int64, f float64"""
    rows = [sorted_fit(p, q, beta) for p, q in zip(pos_keys, neg_keys)]
    return dict(threshold=np.array([r[0] for r in rows], np.float32), defined=np.array([r[1] for r in rows], np.int32),
                tp=np.array([r[2] for r in rows], np.int64), fp=np.array([r[3] for r in rows], np.int64),
                fn=np.array([r[4] for r in rows], np.int64), f=np.array([r[5] for r in rows], np.float64))


def table_fit(scores, truth, beta=1.0):
    """the fit of every class of a score table f32 [n, C] against bool truth [n, C], plus pos / neg / invalid"""
    st = R.table_stats(scores, np.asarray(truth, bool))
    out = fit_columns(st["pos_keys"], st["neg_keys"], beta)
    out.update(pos=st["pos"], neg=st["neg"], invalid=st["invalid"])
    return out


def predict(scores, thr):
    """bool [n, C]: the rule, on the integer keys"""
    scores = np.ascontiguousarray(scores, np.float32)
    thr = np.ascontiguousarray(thr, np.float32)
    return ~np.isnan(scores) & (R.key(scores) >= R.key(thr)[None, :])          # a NaN threshold's key is the sentinel: above every logit's


def counts(scores, truth, thr):
    """int64 [3, C] = TP, FP, FN of the rule"""
    p, y = predict(scores, thr), np.asarray(truth, bool)
    return np.stack([(p & y).sum(0), (p & ~y).sum(0), (~p & y).sum(0)]).astype(np.int64)


def default_counts(scores, truth):
    """int64 [3, C] = TP, FP, FN of the training rule z > 0"""
    p, y = np.asarray(scores, np.float32) > 0, np.asarray(truth, bool)
    return np.stack([(p & y).sum(0), (p & ~y).sum(0), (~p & y).sum(0)]).astype(np.int64)


def brute_fit(z, y, beta=1.0):
    """The definition, for one class: every distinct non-NaN score is tried as a cut t (predict z >= t, float comparison);
    the largest F wins, among equal F the largest t.  Same tuple as sorted_fit."""
    z, y = np.asarray(z, np.float32), np.asarray(y, bool)
    ok = ~np.isnan(z)
    z, y = z[ok].astype(np.float64), y[ok]                     # float64 compares every float32, denormals included, exactly
    P = int(y.sum())
    if P == 0:
        return np.float32(0.0), 0, 0, int((z >= 0.0).sum()), 0, 0.0
    best = None
    for t in np.unique(z):                                     # -0.0 and +0.0 are one value here
        p = z >= t
        tp, fp = int((p & y).sum()), int((p & ~y).sum())
        cand = (f_beta(tp, fp, P - tp, beta), float(t), tp, fp)
        if best is None or cand[:2] > best[:2]:
            best = cand
    f, t, tp, fp = best
    return np.float32(t) + np.float32(0.0), 1, tp, fp, P - tp, f        # + 0.0: a winning -0.0 is reported as +0.0
