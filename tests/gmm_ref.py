"""The float64 reference of the Gaussian mixture kernels (csrc/gmm.hip): plain numpy on the same f32 operands widened."""
import numpy as np

U = 2.0 ** -24
LOG_2PI = float(np.log(2.0 * np.pi))


def shifted(x, inv, shift):
    """x' as the kernels stage it: one f32 multiply (none without inv), one f32 subtract"""
    x = np.asarray(x, np.float32)
    return (x if inv is None else x * np.asarray(inv, np.float32)[:, None]) - np.asarray(shift, np.float32)


def operands(mu, var, w):
    """prec, mprec, cst of components (mu' f32, var f32, weights f32): float64 inside, rounded to f32 once"""
    mu, var, w = (np.asarray(a, np.float64) for a in (mu, var, w))
    with np.errstate(divide="ignore"):
        cst = np.log(w) - 0.5 * ((mu * mu / var + np.log(var)).sum(1) + mu.shape[1] * LOG_2PI)
    return (1.0 / var).astype(np.float32), (mu / var).astype(np.float32), cst.astype(np.float32)


def estep64(xp, prec, mprec, cst):
    """(lj64 [n, k], E [n, k], lse64 [n]) of shifted f32 rows under f32 operands; E is the bound of gmm.hip's header"""
    x, p, q, c = (np.asarray(a, np.float64) for a in (xp, prec, mprec, cst))
    lj = c - 0.5 * ((x * x) @ p.T - 2.0 * x @ q.T)
    a = 0.5 * ((x * x) @ p.T + 2.0 * np.abs(x) @ np.abs(q).T)
    steps = 32 * ((x.shape[1] + 15) // 16) + 2
    with np.errstate(invalid="ignore"):
        err = steps * U / (1.0 - steps * U) * a + U * np.abs(c)
        m = lj.max(1)
        lse = np.where(np.isfinite(m), m + np.log(np.exp(lj - np.where(np.isfinite(m), m, 0.0)[:, None]).sum(1)), m)
    return lj, err, lse


def tree_sum(v):
    """the float64 sum of f32 values in the order of gmm_lsepart_kernel / gmm_lsefinal_kernel; NaN entries are in no sum"""
    v = np.asarray(v, np.float64)

    def tree(red):
        w = 128
        while w:
            red[:w] += red[w:2 * w]
            w //= 2
        return red[0]

    parts = []
    for p0 in range(0, max(v.size, 1), 1024):
        blk = np.zeros(1024)
        blk[:v[p0:p0 + 1024].size] = np.nan_to_num(v[p0:p0 + 1024], nan=0.0)
        red = np.zeros(256)
        for b in range(4):
            red = red + blk[256 * b:256 * b + 256]
        parts.append(tree(red))
    red = np.zeros(256)
    for p, s in enumerate(parts):
        red[p % 256] += s
    return tree(red)


def sums64(xp, r):
    """(sums [k, 1 + 2 d], the same sums of absolute terms) of responsibilities r [n, k] over shifted rows, float64"""
    x, r = np.asarray(xp, np.float64), np.asarray(r, np.float64)
    b = np.concatenate([np.ones((x.shape[0], 1)), x, x * x], 1)
    return r.T @ b, np.abs(r).T @ np.abs(b)


def fit64(x, means0, iters, reg_covar=1e-6):
    """diagonal EM in float64 from initial means (hard assignment to the nearest first): (labels, lower bounds, the last E-step's
    parameters (mu, var, w))"""
    x = np.asarray(x, np.float64)
    r = np.zeros((x.shape[0], len(means0)))
    r[np.arange(x.shape[0]), ((x[:, None, :] - np.asarray(means0, np.float64)[None]) ** 2).sum(2).argmin(1)] = 1.0
    bounds = []
    for it in range(iters + 1):
        nk = r.sum(0)
        mu = r.T @ x / nk[:, None]
        var = np.maximum(r.T @ (x * x) / nk[:, None] - mu * mu, 0.0) + reg_covar
        w = nk / nk.sum()
        lj = np.log(w) - 0.5 * ((((x[:, None, :] - mu[None]) ** 2) / var[None]).sum(2) + np.log(var).sum(1) + x.shape[1] * LOG_2PI)
        lse = lj.max(1) + np.log(np.exp(lj - lj.max(1)[:, None]).sum(1))
        if it < iters:
            bounds.append(lse.mean())
            r = np.exp(lj - lse[:, None])
            last = (mu, var, w)
    return lj.argmax(1), np.array(bounds), last
