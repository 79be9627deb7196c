"""Float64 reference for the k-means kernels (csrc/kmeans.hip), the scores of host/kmeans.h, and the rules their answers are
held to.  numpy only; the Philox is tests/dropout_ref.py's.

Rows.  x [n_table, dim] f32; a list position i names row r = rows[i] (rows None: r = i); a row outside [0, n_table) is invalid.
The row used is x^ = x . inv[r] (inv None: x).  u = 2^-24 (half an ulp of f32, relative).

Assign.  d(i, c) = cn[c] - 2 (x_r . m_c) inv[r], cn an INPUT (f32, taken as exact).  The f32 value differs from the float64
one by at most

    E(i, c) = (dim + 3) u (cn[c] + 2 sum_j |x^_ij| |m_cj|)

  * dim u sum|x^||m| for the f32 dot product in any order (dim products and at most dim adds, each rounding once, first order),
    doubled by the exact factor 2;
  * u . 2 sum|x^||m| for the multiplication by inv[r];
  * u |d| <= u (cn + 2 sum|x^||m|) for the subtraction;
  * together (dim + 2) u 2 sum|x^||m| + u cn; the rest of (dim + 3) u (cn + 2 sum|x^||m|) is slack for second-order terms.
So the centre a correct kernel chooses has d64(i, chosen) - min_c d64(i, c) <= E(i, chosen) + E(i, best), and a row whose
float64 runner-up lies inside E(i, second) + E(i, best) of the best may take either ("ambiguous").
dist2 = max(0, |x^|^2 + d) adds the f32 squared norm of the row ((dim + 2) u relative: dim for the sum, two multiplications by
inv) and one more addition: E2(i, c) = E(i, c) + (dim + 3) u |x^_i|^2.

Update.  mean64[c] = (sum over the members of float64(f32(x . inv))) / count.  The kernel adds the same float64 terms in a fixed
order: any order of count terms is within count . 2^-53 . sum|term| of the exact sum, first order; the division and the cast to
f32 round once each (2^-53 and 2^-24 relative).  Bound used: |M - mean64| <= 2^-23 |mean64| + 2^-52 sum|term| + 2^-149 — "one
f32 ulp" plus the float64 summation term, which only matters where a mean cancels to almost nothing.
cn[c] = f32(sum_j float64(M_cj)^2 added in column order): every square is exact in float64, so this is bit-defined.
inertia: a float64 sum of n non-negative f32 terms in some fixed order: within n . 2^-52 . sum of the float64 sum.

Seeding.  w(i, t) = word 0 of Philox4x32-10(counter {i, 0, t, 0x6B6D2B2B}, key {lo32 s, hi32 s}); first position
(w(0, 0) . n) >> 32; step t: d2min[i] = min(d2min[i], |x^_i - m_(t-1)|^2) with x^ the f32-ROUNDED product (the kernel subtracts
rounded products, and the centre is the rounded row itself, so a copy of a chosen row has d2min = 0 exactly), key_i =
-log((w + 0.5) 2^-32) / d2min[i], +inf at d2min = 0 or an invalid row; the smallest (key, position) wins; every key +inf: the
lowest valid position.  The f32 d2 carries at most (dim + 3) u relative (each difference u, its square 2 u + u, dim adds), the
float64 log and division 2^-52: a step whose winner leads the runner-up by more than 4 (dim + 2) u relative (1e-9 where every
d2 is an exact integer) is decided.
"""
import numpy as np

from tests import dropout_ref

U = 2.0 ** -24
KEY_KMEANS = 0xE7037ED1A0B428DB
TAG = 0x6B6D2B2B
M32 = 0xFFFFFFFF


def list_rows(n_table, rows):
    """(row per list position with -1 for an invalid one, valid mask)"""
    r = np.arange(n_table, dtype=np.int64) if rows is None else np.asarray(rows, np.int64).ravel()
    ok = (r >= 0) & (r < n_table)
    return np.where(ok, r, -1), ok


def scaled_f32(x, inv, r):
    """the f32-rounded products x[r] . inv[r] of valid rows r"""
    x = np.asarray(x, np.float32)
    if inv is None:
        return x[r]
    return (x[r] * np.asarray(inv, np.float32)[r][:, None]).astype(np.float32)


def cn_f32(M):
    """the kernel's squared norms: float64 sum of squares in column order, cast to f32"""
    M = np.asarray(M, np.float32)
    s = np.zeros(M.shape[0], np.float64)
    for j in range(M.shape[1]):
        s += M[:, j].astype(np.float64) ** 2
    return s.astype(np.float32)


def assign64(x, M, cn, inv=None, rows=None):
    """(d64 [n, k], E [n, k], xn64 [n], valid [n]) — invalid positions hold NaN"""
    x = np.asarray(x, np.float64)
    M = np.asarray(M, np.float64)
    cn = np.asarray(cn, np.float64)
    r, ok = list_rows(x.shape[0], rows)
    f = np.ones(x.shape[0]) if inv is None else np.asarray(inv, np.float64)
    xs = x[np.maximum(r, 0)] * f[np.maximum(r, 0)][:, None]
    d = cn[None, :] - 2.0 * (xs @ M.T)
    a = np.abs(xs) @ np.abs(M).T
    E = (x.shape[1] + 3) * U * (cn[None, :] + 2.0 * a)
    xn = (xs ** 2).sum(axis=1)
    d[~ok], E[~ok], xn[~ok] = np.nan, np.nan, np.nan
    return d, E, xn, ok


def check_assign(x, M, cn, assign, dist2, inv=None, rows=None):
    """The acceptance rule of a real-valued assignment.  Returns the share of ambiguous rows among the valid ones."""
    d, E, xn, ok = assign64(x, M, cn, inv, rows)
    assign = np.asarray(assign)
    assert np.all(assign[~ok] == -1) and np.all(np.isnan(np.asarray(dist2)[~ok])), "an invalid row must give -1 / NaN"
    d, E, xn, a, got = d[ok], E[ok], xn[ok], assign[ok].astype(np.int64), np.asarray(dist2, np.float64)[ok]
    k = d.shape[1]
    assert np.all((a >= 0) & (a < k)), "an assignment outside [0, k)"
    idx = np.arange(d.shape[0])
    best = np.argmin(d, axis=1)
    over = d[idx, a] - d[idx, best] - (E[idx, a] + E[idx, best])
    assert np.all(over <= 0), f"a chosen centre is {float(over.max()):.3e} beyond the bound behind the float64 minimum"
    if k > 1:
        masked = d.copy()
        masked[idx, best] = np.inf
        second = np.argmin(masked, axis=1)
        ambiguous = d[idx, second] - d[idx, best] <= E[idx, second] + E[idx, best]
    else:
        ambiguous = np.zeros(d.shape[0], bool)
    assert np.all(a[~ambiguous] == best[~ambiguous]), "a row outside the margin did not take the float64 argmin"
    want = np.maximum(0.0, xn + d[idx, a])
    E2 = E[idx, a] + (x.shape[1] + 3) * U * xn
    err = np.abs(got - want) - E2
    assert np.all(err <= 0), f"dist2 is off by {float(err.max()):.3e} beyond its bound"
    return float(ambiguous.mean()) if ambiguous.size else 0.0


def assign_exact(x, M, cn, inv=None, rows=None):
    """(assign int32, dist2 f32) where every d is an exact f32 integer: the float64 values ARE the f32 ones; lowest c on ties"""
    d, _, xn, ok = assign64(x, M, cn, inv, rows)
    a = np.where(ok, np.argmin(np.where(ok[:, None], d, 0.0), axis=1), -1).astype(np.int32)
    dist = np.where(ok, np.maximum(0.0, xn + d[np.arange(d.shape[0]), np.maximum(a, 0)]), np.nan).astype(np.float32)
    return a, dist


def update64(x, assign, M_prev, inv=None, rows=None):
    """(mean64 [k, dim] with NaN for an empty centre, sizes [k], abs64 [k, dim] = sum of |term|)"""
    x = np.asarray(x, np.float32)
    k, dim = np.asarray(M_prev).shape
    r, ok = list_rows(x.shape[0], rows)
    a = np.asarray(assign, np.int64).ravel()
    member = ok & (a >= 0) & (a < k)
    terms = scaled_f32(x, inv, r[member]).astype(np.float64)
    s, ab = np.zeros((k, dim)), np.zeros((k, dim))
    np.add.at(s, a[member], terms)
    np.add.at(ab, a[member], np.abs(terms))
    sizes = np.bincount(a[member], minlength=k).astype(np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(sizes[:, None] > 0, s / sizes[:, None], np.nan)
    return mean, sizes, ab


def update_bound(mean, ab):
    return 2.0 ** -23 * np.abs(mean) + 2.0 ** -52 * ab + 2.0 ** -149


def check_update(x, assign, M_prev, got, inv=None, rows=None, exact=False):
    """got: ops.kmeans_update's dict.  exact: bit-equal centres (integer tables without inv)."""
    mean, sizes, ab = update64(x, assign, M_prev, inv, rows)
    M_prev = np.asarray(M_prev, np.float32)
    assert np.array_equal(got["sizes"], sizes), "sizes"
    empty = sizes == 0
    assert got["centers"][empty].tobytes() == M_prev[empty].tobytes(), "an empty centre did not keep its row"
    if exact:
        assert got["centers"][~empty].tobytes() == mean[~empty].astype(np.float32).tobytes(), "centres are not the rounded float64 means"
    else:
        err = np.abs(got["centers"][~empty].astype(np.float64) - mean[~empty]) - update_bound(mean[~empty], ab[~empty])
        assert np.all(err <= 0), f"a centre is {float(err.max()):.3e} beyond its bound"
    assert got["cn"].tobytes() == cn_f32(got["centers"]).tobytes(), "cn is not the f32 of the ordered float64 sum of squares"


def seed_word(i, t, s):
    """w(i, t) of the stream s (already seed ^ KEY_KMEANS) -> uint64 array of 32-bit words"""
    return dropout_ref.philox4x32_10((i, 0, t, TAG), (s & M32, (s >> 32) & M32))[..., 0]


def seed64(x, k, s, inv=None, rows=None):
    """(positions [k], leads [k]): the float64 race; lead[t] = (runner-up key - winning key) / winning key (inf when one of them is
    infinite)"""
    x = np.asarray(x, np.float32)
    r, ok = list_rows(x.shape[0], rows)
    n = r.size
    xs = np.zeros((n, x.shape[1]))
    xs[ok] = scaled_f32(x, inv, r[ok]).astype(np.float64)
    pos = [int((int(seed_word(0, 0, s)) * n) >> 32)]
    leads = [np.inf]
    d2min = np.full(n, np.inf)
    idx = np.arange(n)
    for t in range(1, k):
        p = pos[-1]
        centre = xs[p] if p >= 0 and ok[p] else np.zeros(x.shape[1])
        d2min = np.minimum(d2min, ((xs - centre) ** 2).sum(axis=1))
        w = seed_word(idx, t, s).astype(np.float64)
        with np.errstate(divide="ignore"):
            key = np.where(ok & (d2min > 0), -np.log((w + 0.5) * 2.0 ** -32) / np.where(d2min > 0, d2min, 1.0), np.inf)
        if not np.any(np.isfinite(key)):
            pos.append(int(idx[ok][0]) if ok.any() else -1)
            leads.append(np.inf)
            continue
        order = np.lexsort((idx, key))
        first, second = order[0], order[1] if n > 1 else order[0]
        pos.append(int(first))
        leads.append(float((key[second] - key[first]) / key[first]) if np.isfinite(key[second]) and n > 1 else np.inf)
    return np.array(pos, np.int32), np.array(leads)


def contingency(assign, truth, k, C, rows=None):
    """(counts int64 [k, C], skipped)"""
    truth = np.asarray(truth, np.int64)
    r, ok = list_rows(truth.size, rows)
    a = np.asarray(assign, np.int64).ravel()
    y = np.where(ok, truth[np.maximum(r, 0)], -1)
    good = (a >= 0) & (a < k) & (y >= 0) & (y < C)
    out = np.zeros((k, C), np.int64)
    np.add.at(out, (a[good], y[good]), 1)
    return out, int((~good).sum())


def cluster_scores(table):
    """host/kmeans.h's scores from the formulas, in float64 (Python integers for the pair counts)"""
    t = np.asarray(table, np.int64)
    a, b, N = t.sum(axis=1), t.sum(axis=0), int(t.sum())
    if N == 0:
        return dict(purity=0.0, homogeneity=1.0, completeness=1.0, v_measure=1.0, nmi=1.0, ari=1.0, entropy_classes=0.0, entropy_clusters=0.0, rows=0)

    def entropy(c):
        c = c[c > 0].astype(np.float64)
        return max(0.0, float(-np.sum(c / N * (np.log(c) - np.log(N)))))
    hc, hk = entropy(b), entropy(a)
    i, y = np.nonzero(t)
    n = t[i, y].astype(np.float64)
    mi = max(0.0, float(np.sum(n / N * ((np.log(n) - np.log(a[i])) + (np.log(N) - np.log(b[y]))))))
    h = mi / hc if hc > 0 else 1.0
    c = mi / hk if hk > 0 else 1.0
    v = 2 * h * c / (h + c) if h + c > 0 else 0.0
    nmi = 1.0 if hc == 0 and hk == 0 else (0.0 if mi == 0 else mi / ((hc + hk) / 2))
    sq = sum(int(v) ** 2 for v in t.ravel())
    tp, fp, fn = sq - N, sum(int(v) ** 2 for v in a) - sq, sum(int(v) ** 2 for v in b) - sq
    tn = N * N - N - tp - fp - fn
    ari = 1.0 if fp == 0 and fn == 0 else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    return dict(purity=float(t.max(axis=1).sum()) / N, homogeneity=h, completeness=c, v_measure=v, nmi=nmi, ari=float(ari), entropy_classes=hc,
                entropy_clusters=hk, rows=N)
