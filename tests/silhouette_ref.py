"""Float64 reference for the silhouette kernels (csrc/silhouette.hip) and the bounds their answers are held to.  numpy only.

Points.  x [n_table, dim] f32; list position i names row r = rows[i] (rows None: r = i) and carries labels[i].  A position is a
POINT when its label is in [0, k) and its row in [0, n_table); two positions that name one row are two points.  The row used is
x^ = x . inv[r] (inv None: x).  n_c = the points of label c.  With A = labels[i] (scikit-learn's silhouette_samples, euclidean):

    S(i, c) = sum of d(i, j) over the points j of label c, j != i by position
    a = S(i, A) / (n_A - 1), 0 when n_A = 1;  b = min over c != A with n_c > 0 of S(i, c) / n_c;  neighbor = the lowest such c
    s = (b - a) / max(a, b), 0 when n_A = 1 or max(a, b) = 0

Fewer than two non-empty labels: b = 0, s = 0, neighbor = -1.  A position that is no point: NaN, NaN, NaN, -1; its row of S is 0.

The bound.  u = 2^-24.  The kernel forms d^2 in f32 as (xn_i + xn_j) - 2 dot(x^_i, x^_j) and d = sqrtf(max(0, d^2)):
  * the dot of dim f32 products of rows that were themselves rounded once after scaling: (dim + 2) u |x_i| |x_j|, doubled;
  * each xn = (sumsq . inv) . inv: at most dim roundings of the sum and two of the scaling, (dim + 2) u xn;
  * the two f32 additions: 2 u (xn_i + xn_j + 2 |x_i| |x_j|) at most;
so |d^2' - d^2| <= e2 = (dim + 4) u (xn_i + xn_j + 2 |x_i| |x_j|) = (dim + 4) u (|x_i| + |x_j|)^2.  The square root of a value
within e2 of d^2 is within min(sqrt(e2), e2 / d) of d (|sqrt(p) - sqrt(q)| <= sqrt|p - q| and <= |p - q| / sqrt(q)), and sqrtf
rounds once: |d' - d| <= E(i, j) = min(sqrt(e2), e2 / d) + u d.  The float64 additions of S add at most n_c 2^-52 S.
E_S(i, c) = sum_j E(i, j) + n_c 2^-52 S(i, c); da = E_S(i, A) / (n_A - 1), dM(i, c) = E_S(i, c) / n_c, each plus 2^-52 of the
value for the one float64 division; db = max_c dM(i, c) (a minimum moves by no more than its most moved argument);
|ds| <= 2 (da + db) / max(a, b).  neighbor is decided where the two lowest means differ by more than the sum of their dM.
"""
import numpy as np

U = 2.0 ** -24


def list_rows(n_table, rows):
    r = np.arange(n_table, dtype=np.int64) if rows is None else np.asarray(rows, np.int64).ravel()
    ok = (r >= 0) & (r < n_table)
    return np.where(ok, r, 0), ok


def points_of(labels, k, n_table, rows=None):
    """(label per position with -1 where the position is no point, sizes int32 [k])"""
    r, ok = list_rows(n_table, rows)
    lab = np.asarray(labels, np.int64).ravel()
    assert lab.size == r.size
    lab = np.where(ok & (lab >= 0) & (lab < k), lab, -1)
    return lab, np.bincount(lab[lab >= 0], minlength=k).astype(np.int32)


def sums64(x, labels, k, inv=None, rows=None, f32_sqrt=False, bounds=False):
    """(sums float64 [n, k], sizes int32 [k]) and with `bounds` a third value E_S [n, k].  f32_sqrt: every distance is
    sqrt in f32 of the float64 d^2 rounded to f32 — the kernel's own value where every d^2 is an exact f32 integer."""
    x = np.asarray(x, np.float64)
    r, _ = list_rows(x.shape[0], rows)
    lab, sizes = points_of(labels, k, x.shape[0], rows)
    f = np.ones(x.shape[0]) if inv is None else np.asarray(inv, np.float64)
    xs = x[r] * f[r][:, None]
    xn = (xs ** 2).sum(axis=1)
    d2 = np.maximum(xn[:, None] + xn[None, :] - 2.0 * (xs @ xs.T), 0.0)
    d = np.sqrt(d2.astype(np.float32)).astype(np.float64) if f32_sqrt else np.sqrt(d2)
    n = r.size
    member = np.zeros((n, k))
    pts = lab >= 0
    member[np.flatnonzero(pts), lab[pts]] = 1.0
    d[np.arange(n), np.arange(n)] = 0.0                           # the self pair, by position
    d[~pts] = 0.0
    sums = d @ member                                             # exact where every term is an f32 and the total below 2^53 ulps
    if not bounds:
        return sums, sizes
    nrm = np.sqrt(xn)
    e2 = (x.shape[1] + 4) * U * (nrm[:, None] + nrm[None, :]) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        E = np.minimum(np.sqrt(e2), np.where(d > 0, e2 / d, np.inf)) + U * d
    E[np.arange(n), np.arange(n)] = 0.0
    E[~pts] = 0.0
    return sums, sizes, E @ member + sizes[None, :] * 2.0 ** -52 * sums


def widths(sums, labels, sizes, valid=None):
    """dict(s, a, b, neighbor, defined) from sums, by the kernel's own float64 expressions.  valid: which positions name a row of
    the table (None: all)."""
    sums = np.asarray(sums, np.float64)
    n, k = sums.shape
    sizes = np.asarray(sizes, np.int64)
    lab = np.asarray(labels, np.int64).ravel()
    pts = (lab >= 0) & (lab < k) & (np.ones(n, bool) if valid is None else np.asarray(valid, bool))
    A = np.where(pts, lab, 0)
    idx = np.arange(n)
    nA = sizes[A]
    a = np.where(nA > 1, sums[idx, A] / np.maximum(nA - 1, 1).astype(np.float64), 0.0)
    defined = int((sizes > 0).sum()) >= 2
    if defined:
        with np.errstate(divide="ignore", invalid="ignore"):
            means = np.where(sizes[None, :] > 0, sums / sizes[None, :].astype(np.float64), np.inf)
        means[idx, A] = np.inf
        nb = np.argmin(means, axis=1)                             # the first of equal means: the lowest label
        b = means[idx, nb]
        mx = np.maximum(a, b)
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.where((nA > 1) & (mx > 0), (b - a) / mx, 0.0)
    else:
        nb, b, s = np.full(n, -1), np.zeros(n), np.zeros(n)
    out = dict(s=np.where(pts, s, np.nan), a=np.where(pts, a, np.nan), b=np.where(pts, b, np.nan),
               neighbor=np.where(pts, nb, -1).astype(np.int32), defined=defined)
    return out


def width_bounds(sums, E_S, labels, sizes, valid=None):
    """dict(a, b, s: the bounds [n]; decided: bool [n], the reference's neighbor leads its runner-up by more than their bounds)"""
    sums = np.asarray(sums, np.float64)
    n, k = sums.shape
    sizes = np.asarray(sizes, np.int64)
    w = widths(sums, labels, sizes, valid)
    pts = ~np.isnan(w["s"])
    A = np.where(pts, np.asarray(labels, np.int64).ravel(), 0)
    idx = np.arange(n)
    nA = sizes[A]
    da = np.where(nA > 1, E_S[idx, A] / np.maximum(nA - 1, 1), 0.0) + 2.0 ** -52 * np.nan_to_num(w["a"])
    if not w["defined"]:
        return dict(a=da, b=np.zeros(n), s=np.zeros(n), decided=np.ones(n, bool))
    other = (sizes[None, :] > 0) & (np.arange(k)[None, :] != A[:, None])
    with np.errstate(divide="ignore", invalid="ignore"):
        means = np.where(other, sums / sizes[None, :], np.inf)
        dM = np.where(other, E_S / sizes[None, :] + 2.0 ** -52 * np.abs(means), 0.0)
    db = dM.max(axis=1)
    mx = np.maximum(np.nan_to_num(w["a"]), np.nan_to_num(w["b"]))
    with np.errstate(divide="ignore", invalid="ignore"):
        ds = np.where(mx > 0, 2.0 * (da + db) / mx, np.inf)
    first = np.argmin(means, axis=1)
    lead = means[idx, first].copy()
    dfirst = dM[idx, first]
    means[idx, first] = np.inf
    second = np.argmin(means, axis=1)
    with np.errstate(invalid="ignore"):
        decided = ~(means[idx, second] - lead <= dM[idx, second] + dfirst)      # a single other label: inf - x, decided
    return dict(a=da, b=db, s=ds, decided=decided | ~pts)


def blobs(n, dim, k, seed):
    """(x f32 [n, dim], labels int32 [n]): centres 2 N(0, I), points centre + 0.5 N(0, I), 10 % of the labels redrawn uniformly"""
    rng = np.random.default_rng(seed)
    centres = 2.0 * rng.standard_normal((k, dim))
    g = rng.integers(0, k, n)
    x = (centres[g] + 0.5 * rng.standard_normal((n, dim))).astype(np.float32)
    redraw = rng.random(n) < 0.1
    g[redraw] = rng.integers(0, k, int(redraw.sum()))
    return x, g.astype(np.int32)
