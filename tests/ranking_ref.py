"""numpy reference of the ranking metrics (csrc/ranking.hip, host/ranking.h): the key map, exact integers for u2, float64 for
ap_sum, and the derived report.  Everything goes through the keys and numpy.searchsorted, the form the kernels use:

  u2     = sum over positives i of #{negatives with key < key_i} + #{negatives with key <= key_i}
  ap_sum = sum over positives i of TP_ge(i) / (TP_ge(i) + FP_ge(i)),  TP_ge / FP_ge = positives / negatives with key >= key_i

The terms of ap_sum are single float64 divisions of exact integers; they are added exactly (math.fsum), so a float64 sum of
the same P terms in ANY order lies within P . 2^-53 relative of this value, and the tests allow P . 2^-52."""
import math

import numpy as np

SENTINEL = 0xFFFFFFFF


def key(x):
    """the order-preserving uint32 image of float32 scores; a NaN maps to SENTINEL (it has no key)"""
    x = np.ascontiguousarray(x, np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    b = np.where(b == 0x80000000, 0, b)
    k = np.where(b >> 31 == 1, b ^ 0xFFFFFFFF, b | 0x80000000)
    return np.where(np.isnan(x), SENTINEL, k).astype(np.uint32)


def sorted_stats(pk, nk):
    """(u2 as a Python int, ap_sum float64) from the sorted keys of a class's positives and negatives"""
    P, N = pk.size, nk.size
    if P == 0:
        return 0, 0.0
    lt, le = np.searchsorted(nk, pk, "left").astype(np.int64), np.searchsorted(nk, pk, "right").astype(np.int64)
    tp = P - np.searchsorted(pk, pk, "left").astype(np.int64)
    fp = N - lt
    return int(lt.sum() + le.sum()), math.fsum((tp.astype(np.float64) / (tp + fp).astype(np.float64)).tolist())


def table_stats(scores, truth, classes=None, num_classes=None):
    """What gcnhip_rank_keys + sort + gcnhip_rank_stats give for the listed rows.  scores f32 [n, C]; truth int [n] (a label
    outside [0, num_classes) is in no class) or bool [n, C].  Returns a dict: pos, neg, invalid (int64 [C]), unlabelled,
    u2 (int64 [C]), ap_sum (float64 [C]), pos_keys / neg_keys (lists of sorted uint32 arrays)."""
    scores = np.ascontiguousarray(scores, np.float32)
    n, C = scores.shape
    truth = np.asarray(truth)
    num_classes = C if num_classes is None else num_classes
    classes = np.arange(C) if classes is None else np.asarray(classes)
    if truth.ndim == 1:
        labelled = (truth >= 0) & (truth < num_classes)
        is_pos = truth[:, None] == classes[None, :]
    else:
        labelled = np.ones(n, bool)
        is_pos = truth.astype(bool)
    nan = np.isnan(scores)
    k = key(scores)
    out = dict(pos=np.zeros(C, np.int64), neg=np.zeros(C, np.int64), invalid=np.zeros(C, np.int64), unlabelled=int((~labelled).sum()),
               u2=np.zeros(C, np.int64), ap_sum=np.zeros(C, np.float64), pos_keys=[], neg_keys=[])
    for c in range(C):
        ok = labelled & ~nan[:, c]
        pk, nk = np.sort(k[ok & is_pos[:, c], c]), np.sort(k[ok & ~is_pos[:, c], c])
        out["pos"][c], out["neg"][c], out["invalid"][c] = pk.size, nk.size, int((labelled & nan[:, c]).sum())
        out["u2"][c], out["ap_sum"][c] = sorted_stats(pk, nk)
        out["pos_keys"].append(pk)
        out["neg_keys"].append(nk)
    return out


def key_tables(scores, truth, classes=None, num_classes=None):
    """the two unsorted tables gcnhip_rank_keys writes: uint32 [C, n], SENTINEL where the row is no positive (negative)"""
    scores = np.ascontiguousarray(scores, np.float32)
    n, C = scores.shape
    truth = np.asarray(truth)
    num_classes = C if num_classes is None else num_classes
    classes = np.arange(C) if classes is None else np.asarray(classes)
    if truth.ndim == 1:
        labelled = ((truth >= 0) & (truth < num_classes))[:, None]
        is_pos = truth[:, None] == classes[None, :]
    else:
        labelled, is_pos = np.ones((n, 1), bool), truth.astype(bool)
    ok = labelled & ~np.isnan(scores)
    k = key(scores)
    return (np.where(ok & is_pos, k, SENTINEL).astype(np.uint32).T.copy(), np.where(ok & ~is_pos, k, SENTINEL).astype(np.uint32).T.copy())


def report(u2, ap_sum, pos, neg):
    """host/ranking.h in numpy: undefined values are 0 with the mask clear, the means run over the defined classes"""
    u2, pos, neg = (np.asarray(a, np.int64) for a in (u2, pos, neg))
    ap_sum = np.asarray(ap_sum, np.float64)
    ad, pd = (pos > 0) & (neg > 0), pos > 0
    auc = np.array([int(u) / (2 * int(p) * int(q)) if d else 0.0 for u, p, q, d in zip(u2, pos, neg, ad)], np.float64)
    ap = np.array([s / int(p) if d else 0.0 for s, p, d in zip(ap_sum, pos, pd)], np.float64)

    def mean(v, d, w=None):
        if not d.any():
            return 0.0
        t = tot = 0.0
        for x, on, wt in zip(v, d, np.ones(len(v)) if w is None else w):     # the host's order of additions
            if on:
                t += float(wt) * x
                tot += float(wt)
        return t / tot
    return dict(auc=auc, ap=ap, auc_defined=ad, ap_defined=pd, macro_auc=mean(auc, ad), macro_ap=mean(ap, pd), weighted_auc=mean(auc, ad, pos),
                weighted_ap=mean(ap, pd, pos), classes_defined=int(ad.sum()))
