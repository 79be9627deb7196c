"""float64 numpy reference of label propagation and Correct & Smooth as the GPU path computes them (no GPU here): one blend
step, the K-step recurrence, label propagation, the two row-local steps of Correct & Smooth and the whole scheme — each
with a propagated ERROR BOUND for an f32 implementation, so that no multi-iteration tolerance has to be guessed.

A graph is a triple csr = (indptr, indices, coef): the device object's own arrays (ops.Graph.csr()), or edge_coef()'s
copy of how the device forms its f32 coefficients.  The reference multiplies by those f32 numbers, exactly.

Error bound.  One f32 sum of terms t_i, in any order and with or without fused multiply-adds, is within 8 eps sum |t_i| of
the real sum for the row lengths used here (DESIGN §2's sum bound; eps = 2^-24).  An iterate that already carries an
entrywise error B_k, blended with a base that carries B_0, then satisfies

    B_{k+1} = alpha |A^| B_k + (1 - alpha) B_0 + 8 eps (alpha |A^| |Y_k| + (1 - alpha) |Y_0|)

because the blend is linear and the clamp is 1-Lipschitz (it never enlarges a difference).  With exact inputs B_0 = 0."""
import numpy as np

EPS = 2.0 ** -24
EXP_ATOL = 2e-6      # f32 expf of a log-probability: values <= 1, the relative tolerance the prediction tests use for prob


def edge_coef(indptr, indices):
    """the f32 coefficient of every edge as the device forms it: float sqrt of the integer degree product, divide in double,
    narrow (degrees = row lengths of the square adjacency)"""
    indptr = np.asarray(indptr, np.int64)
    deg = np.diff(indptr)
    rows = np.repeat(np.arange(deg.size), deg)
    prod = (deg[rows] * deg[np.asarray(indices, np.int64)]).astype(np.float32)
    return (1.0 / np.sqrt(prod).astype(np.float64)).astype(np.float32)


def aggregate(csr, x, absolute=False):
    """A^ . x in float64 (absolute: |A^| . |x|)"""
    indptr, indices, coef = csr
    indptr = np.asarray(indptr, np.int64)
    x = np.asarray(x, np.float64)
    c = np.asarray(coef, np.float64)
    terms = c[:, None] * x[np.asarray(indices, np.int64)]
    out = np.zeros((indptr.size - 1, x.shape[1]), np.float64)
    full = np.flatnonzero(np.diff(indptr) > 0)                    # (reduceat cannot express an empty row)
    if full.size:
        out[full] = np.add.reduceat(np.abs(terms) if absolute else terms, indptr[:-1][full], axis=0)
    return out


def blend_step(csr, x, base, alpha, beta, lo=-np.inf, hi=np.inf):
    """(clip(alpha . A^ x + beta . base, lo, hi), its f32 bound 8 eps (|alpha| sum |coef . x| + |beta . base|))"""
    base = np.asarray(base, np.float64)
    out = np.clip(alpha * aggregate(csr, x) + beta * base, lo, hi)
    return out, 8 * EPS * (abs(alpha) * aggregate(csr, x, absolute=True) + np.abs(beta * base))


def propagate(csr, y0, alpha, iters, lo=-np.inf, hi=np.inf, b0=0.0):
    """(Y_iters, B_iters): Y_{k+1} = clip(alpha A^ Y_k + (1 - alpha) Y_0, lo, hi), and the bound recurrence of the module
    docstring started from the entrywise input error b0 (scalar or array)"""
    y0 = np.asarray(y0, np.float64)
    b0 = np.broadcast_to(np.asarray(b0, np.float64), y0.shape)
    y, b = y0, b0
    for _ in range(int(iters)):
        nb = alpha * aggregate(csr, b, absolute=True) + (1 - alpha) * b0 + \
            8 * EPS * (alpha * aggregate(csr, y, absolute=True) + (1 - alpha) * np.abs(y0))
        y = np.clip(alpha * aggregate(csr, y) + (1 - alpha) * y0, lo, hi)
        b = nb
    return y, np.array(b)


def onehot_rows(truth, num_classes):
    """[n, C]: the one-hot row where truth is a class, a zero row elsewhere"""
    truth = np.asarray(truth, np.int64)
    y = np.zeros((truth.size, num_classes), np.float64)
    ok = (truth >= 0) & (truth < num_classes)
    y[np.flatnonzero(ok), truth[ok]] = 1.0
    return y


def label_propagation(csr, truth, num_classes, alpha=0.9, iters=50):
    """(pred, Y, B): propagate from the one-hot rows of the known nodes (truth = label where known, else -1), clamp [0, 1]"""
    y, b = propagate(csr, onehot_rows(truth, num_classes), alpha, iters, 0.0, 1.0)
    return np.argmax(y, axis=1), y, b


def error_rows(logp, truth, rows=None):
    """(E_0, (sum |E_0|, rows counted)): E_0[r] = onehot(truth[r]) - exp(logp[r]) on the listed rows (None: all) whose truth is a
    class, zero elsewhere"""
    logp = np.asarray(logp, np.float64)
    truth = np.asarray(truth, np.int64)
    n, c = logp.shape
    listed = np.zeros(n, bool)
    listed[np.arange(n) if rows is None else np.asarray(rows, np.int64)] = True
    ok = listed & (truth >= 0) & (truth < c)
    e = np.where(ok[:, None], onehot_rows(np.where(ok, truth, -1), c) - np.exp(logp), 0.0)
    return e, (float(np.abs(e).sum()), int(ok.sum()))


def autoscale(e_hat, sigma):
    """s[r] = (sigma[0] / sigma[1]) / sum_j |e_hat[r, j]|, 1 unless s <= 1000 (a zero row, inf and NaN included)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (np.float64(sigma[0]) / np.float64(sigma[1])) / np.abs(np.asarray(e_hat, np.float64)).sum(axis=1)
    return np.where(s <= 1000.0, s, 1.0)


def correct_rows(logp, e_hat, truth, sigma):
    """G_0: the one-hot row where truth is a class, else exp(logp) + s . e_hat"""
    logp = np.asarray(logp, np.float64)
    truth = np.asarray(truth, np.int64)
    c = logp.shape[1]
    known = (truth >= 0) & (truth < c)
    q = np.exp(logp) + autoscale(e_hat, sigma)[:, None] * np.asarray(e_hat, np.float64)
    return np.where(known[:, None], onehot_rows(truth, c), q)


def correct_and_smooth(csr, logp, truth, alpha_correct=0.8, iters_correct=50, alpha_smooth=0.8, iters_smooth=50):
    """Correct & Smooth from log-softmax rows and the truth of the known nodes (-1 elsewhere).  Returns a dict: E0, E_hat, G0,
    G, pred, and the f32 bounds B_E (of E_hat), B_G0, B_G.

    How the bounds chain.  E_0 passes through expf of a log-probability: EXP_ATOL per entry of a known row, exact zeros
    elsewhere; the correct stage propagates it (propagate's b0).  G_0 = P + s . E^ with s = sigma / n_r, sigma = S / m, S = the
    sum of |E_0| over the m known rows and n_r = sum_j |E^[r, j]|:  dS <= m C EXP_ATOL + 8 eps S,  dn_r <= sum_j B_E[r, j] +
    8 eps n_r, so  ds / s <= dS / S + dn_r / n_r + 4 eps  (two divisions), and
        B_G0[r, j] = EXP_ATOL + s B_E[r, j] + s |E^[r, j]| (ds / s) + 4 eps |G_0[r, j]|
    on unknown rows (without the ds term where the guard sets s = 1), 0 on known rows (exact one-hot).  A row whose unguarded s
    lies within 4 ds of 1000 could take the guard differently in f32: its bound also carries the distance between the two
    outcomes, |s - 1| |E^[r, j]|.  The smooth stage propagates B_G0.  `guard_margin` is the smallest |s / 1000 - 1| over the rows."""
    logp = np.asarray(logp, np.float64)
    truth = np.asarray(truth, np.int64)
    n, c = logp.shape
    known = (truth >= 0) & (truth < c)
    e0, sigma = error_rows(logp, truth)
    e_hat, b_e = propagate(csr, e0, alpha_correct, iters_correct, -1.0, 1.0, b0=np.where(known[:, None], EXP_ATOL, 0.0))
    g0 = correct_rows(logp, e_hat, truth, sigma)
    s = autoscale(e_hat, sigma)
    nr = np.abs(e_hat).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        raw = (sigma[0] / sigma[1]) / nr if sigma[1] else np.full(n, np.nan)
        ds_rel = (sigma[1] * c * EXP_ATOL + 8 * EPS * sigma[0]) / sigma[0] + (b_e.sum(axis=1) + 8 * EPS * nr) / nr + 4 * EPS
    with np.errstate(invalid="ignore"):
        margin = np.abs(raw / 1000.0 - 1.0)
        either = np.isfinite(raw) & (margin <= 4 * ds_rel)        # the guard could fall either way
    ds_rel = np.where(raw <= 1000.0, ds_rel, 0.0)                 # guard rows: s = 1 exactly
    b_g0 = EXP_ATOL + s[:, None] * b_e + s[:, None] * np.abs(e_hat) * ds_rel[:, None] + 4 * EPS * np.abs(g0)
    b_g0 = np.where(either[:, None], b_g0 + np.abs(np.where(either, raw, 1.0) - 1.0)[:, None] * np.abs(e_hat), b_g0)
    b_g0 = np.where(known[:, None], 0.0, b_g0)
    g, b_g = propagate(csr, g0, alpha_smooth, iters_smooth, 0.0, 1.0, b0=b_g0)
    return dict(E0=e0, sigma=sigma, E_hat=e_hat, G0=g0, G=g, pred=np.argmax(g, axis=1), B_E=b_e, B_G0=b_g0, B_G=b_g, scale=s,
                guard_margin=float(np.nanmin(np.where(np.isfinite(margin), margin, np.nan))) if np.isfinite(margin).any() else np.inf)


def clear_rows(y, bound):
    """rows whose top-two margin exceeds twice the row's largest bound: the argmax is decided whatever the rounding"""
    t = np.sort(np.asarray(y, np.float64), axis=1)
    if t.shape[1] < 2:
        return np.ones(t.shape[0], bool)
    return t[:, -1] - t[:, -2] > 2 * np.asarray(bound, np.float64).max(axis=1)
