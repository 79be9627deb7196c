"""Float64 reference of map quality as include/gcnhip_driver.h defines it (csrc/mapq.hip): brute-force d2 of the f32 rows the kernel
sees, the (d2, position) order, kNN lists, ranks, the penalty sums and the scores; and how many candidates lie within the f32 error
bound of a target's distance (`slack`), which is all a float table's ranks may differ by.  numpy only."""
import numpy as np

from tests.dbscan_ref import dist2
from tests.tsne_ref import scaled_rows                          # noqa: F401 (re-exported: the rows a pack holds)


def candidates(xs, ok):
    """d2 float64 [n, n] with +inf at the self pair and where either position is no point"""
    d = dist2(xs, ok)
    np.fill_diagonal(d, np.inf)
    return d


def knn(d, k):
    """int32 [n, k]: per row the k candidates of smallest (d2, position), nearest first; -1 past the candidates"""
    order = np.argsort(d, axis=1, kind="stable")[:, :k]         # stable: equal distances in ascending position
    return np.where(np.isfinite(np.take_along_axis(d, order, 1)), order, -1).astype(np.int32)


def ranks(d, targets):
    """int32 [n, k]: 1 + the candidates of row i other than the target with a smaller (d2, position); 0 where i or the target is no point"""
    n, pos = d.shape[0], np.arange(d.shape[0])
    out = np.zeros(targets.shape, np.int32)
    for i in range(n):
        for t, j in enumerate(targets[i]):
            if 0 <= j < n and np.isfinite(d[i, j]):
                out[i, t] = 1 + int(((d[i] < d[i, j]) | ((d[i] == d[i, j]) & (pos < j))).sum())
    return out


def scores(knn_x, knn_y, rank_x, rank_y, ok, k):
    """(per int64 [n, 3], totals int64 [4], (trustworthiness, continuity, overlap)) from the lists and the rank tables"""
    shared = np.array([np.intersect1d(a[a >= 0], b[b >= 0]).size for a, b in zip(knn_x, knn_y)])
    per = np.stack([np.maximum(rank_x - k, 0).sum(1), np.maximum(rank_y - k, 0).sum(1), shared], 1) * ok[:, None]
    m = int(ok.sum())
    tot = np.append(per.sum(0), m).astype(np.int64)
    worst = m * k * (2 * m - 3 * k - 1) / 2
    return per, tot, (1 - tot[0] / worst, 1 - tot[1] / worst, tot[2] / (m * k))


def bound(xs, i, a, b):
    """the f32 error bound on d2(i, a) - d2(i, b): (dim + 4) 2^-24 (2 xn_i + xn_a + xn_b)"""
    xn = (xs.astype(np.float64) ** 2).sum(1)
    return (xs.shape[1] + 4) * 2.0 ** -24 * (2 * xn[i] + xn[a] + xn[b])


def slack(xs, d, targets):
    """int [n, k]: the candidates l other than the target whose d2(i, l) is within the bound of d2(i, target)"""
    out = np.zeros(targets.shape, np.int64)
    l = np.arange(d.shape[0])
    for i in range(d.shape[0]):
        for t, j in enumerate(targets[i]):
            if j >= 0 and np.isfinite(d[i, j]):
                out[i, t] = int((np.isfinite(d[i]) & (l != j) & (np.abs(d[i] - d[i, j]) <= bound(xs, i, l, j))).sum())
    return out


def boundary_rows(xs, d, k):
    """bool [n]: the gap between the k-th and the (k + 1)-th neighbour is within the bound (the kNN SET is then not decided in f32)"""
    o = np.argsort(d, axis=1, kind="stable")
    i = np.arange(d.shape[0])
    return d[i, o[:, k]] - d[i, o[:, k - 1]] <= bound(xs, i, o[:, k - 1], o[:, k])
