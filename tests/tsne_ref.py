"""Float64 reference of exact t-SNE as include/gcnhip_driver.h defines it (csrc/tsne.hip): dense P, gradient, KL, the update rule.
numpy only.  `f32=True` forms d2 in f32 by the kernel's formula, (xn_i + xn_j) - 2 dot, everything behind it in float64: the
difference between the two gradients is the reference's own sensitivity to f32 distances, and the GPU tests allow 8 times that."""
import numpy as np


def scaled_rows(x, rows=None, inv=None):
    """(x^ f32 [n, dim], ok bool [n]): the listed rows times inv, rounded to f32; ok = the position names a row of the table"""
    x = np.asarray(x, np.float32)
    r = np.arange(x.shape[0]) if rows is None else np.asarray(rows, np.int64).ravel()
    ok = (r >= 0) & (r < x.shape[0])
    r = np.where(ok, r, 0)
    f = np.ones(x.shape[0], np.float32) if inv is None else np.asarray(inv, np.float32)
    return (x[r] * f[r][:, None]).astype(np.float32), ok


def dist2(xs, ok, f32=False):
    """d2 [n, n], +inf at the self pair (by position) and where either position is no point"""
    t = np.float32 if f32 else np.float64
    a = xs.astype(t)
    xn = (a * a).sum(axis=1, dtype=t)
    d = np.maximum((xn[:, None] + xn[None, :]) - t(2) * (a @ a.T), t(0)).astype(np.float64)
    d[~ok, :] = np.inf
    d[:, ~ok] = np.inf
    np.fill_diagonal(d, np.inf)
    return d


def entropy(d2, beta):
    """(H, Z, m) per row at beta; rows without a finite entry give NaN"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = d2.min(axis=1)
        dd = np.where(np.isfinite(d2), d2 - m[:, None], 0.0)
        e = np.where(np.isfinite(d2), np.exp(-beta[:, None] * dd), 0.0)
        z = e.sum(axis=1)
        return np.log(z) + beta * (dd * e).sum(axis=1) / z, z, m


def bandwidths(d2, perplexity):
    """(beta, converged) by scikit-learn's search; a row that never gets there keeps the last beta that was evaluated"""
    n, target = d2.shape[0], np.log(perplexity)
    beta, lo, hi = np.ones(n), np.full(n, -np.inf), np.full(n, np.inf)
    live = np.isfinite(d2).any(axis=1)
    conv = np.zeros(n, bool)
    for step in range(100):
        idx = np.flatnonzero(live)
        if not idx.size:
            break
        diff = entropy(d2[idx], beta[idx])[0] - target
        done = np.abs(diff) <= 1e-5
        conv[idx[done]] = True
        live[idx[done]] = False
        if step == 99:
            break
        up, dn = idx[~done & (diff > 0)], idx[~done & (diff <= 0)]
        lo[up] = beta[up]
        beta[up] = np.where(np.isinf(hi[up]), beta[up] * 2, (beta[up] + hi[up]) / 2)
        hi[dn] = beta[dn]
        beta[dn] = np.where(np.isinf(lo[dn]), beta[dn] / 2, (beta[dn] + lo[dn]) / 2)
    return beta, conv


def joint(d2, beta):
    """dense P [n, n]: (e_i(j) / Z_i + e_j(i) / Z_j) / (2 n_points), 0 where d2 is inf"""
    ok = np.isfinite(d2).any(axis=1)
    _, z, m = entropy(d2, beta)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.where(np.isfinite(d2), np.exp(-beta[:, None] * (d2 - m[:, None])) / z[:, None], 0.0)
    c[~ok] = 0.0
    return (c + c.T) / (2.0 * ok.sum())


def gradient(P, y, exaggeration=1.0):
    """(grad [n, k], Zq, KL) at y; rows of P that are all zero (no point) get NaN"""
    y = np.asarray(y, np.float64)
    ok = P.any(axis=1)
    dy = y[:, None, :] - y[None, :, :]
    w = 1.0 / (1.0 + (dy ** 2).sum(axis=2))
    w[~ok, :] = 0.0
    w[:, ~ok] = 0.0
    np.fill_diagonal(w, 0.0)
    zq = w.sum()
    g = 4.0 * (exaggeration * ((P * w)[:, :, None] * dy).sum(axis=1) - ((w * w)[:, :, None] * dy).sum(axis=1) / zq)
    pos = P > 0
    kl = float((P[pos] * np.log(P[pos] * zq / w[pos])).sum())
    g[~ok] = np.nan
    return g, float(zq), kl


def auto_learning_rate(points, exaggeration=12.0):
    return max(points / exaggeration / 4.0, 50.0)


def run(P, y0, iters, exaggeration=12.0, exaggeration_iters=250, learning_rate=None):
    """the trajectory's end from y0: scikit-learn's gains, momentum 0.5 / 0.8, a fixed iteration count"""
    y = np.array(y0, np.float64)
    ok = P.any(axis=1)
    lr = auto_learning_rate(int(ok.sum()), exaggeration) if learning_rate is None else learning_rate
    up, gain = np.zeros_like(y), np.ones_like(y)
    for it in range(iters):
        early = it < exaggeration_iters
        g = np.nan_to_num(gradient(P, np.where(ok[:, None], y, 0.0), exaggeration if early else 1.0)[0])
        gain = np.maximum(np.where(up * g < 0.0, gain + 0.2, gain * 0.8), 0.01)
        up = (0.5 if early else 0.8) * up - lr * (gain * g)
        y = y + up
    y[~ok] = np.nan
    return y


def label_share(y, labels, k=10):
    """the mean share of each point's k nearest neighbours in y that carry its label"""
    y = np.asarray(y, np.float64)
    d = ((y[:, None, :] - y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    nb = np.argsort(d, axis=1, kind="stable")[:, :k]
    return float((labels[nb] == labels[:, None]).mean())


def pca_start(x, k=2):
    """(coords [n, k] on the leading k principal axes, the t-SNE start: coords scaled so that the first has a deviation of 1e-4)"""
    c = np.asarray(x, np.float64) - np.asarray(x, np.float64).mean(axis=0)
    co = c @ np.linalg.svd(c, full_matrices=False)[2][:k].T
    return co, co * (1e-4 / co[:, 0].std())
