"""The float64 reference of the kernel two-sample sums (csrc/mmd.hip): plain numpy on the same f32 operands widened, and the error
bound of the kernel's chain evaluated per entry (DESIGN 4.31 derives it), never fitted."""
import numpy as np

U = 2.0 ** -24
F32_ULP = 2.0 ** -23                                       # HIP documents expf to 1 ulp
PART = 1024                                                # positions per part: the length of T's f32 chain


def gamma_err(m):
    return m * U / (1.0 - m * U)


def operands(table, rows, inv, shift):
    """(x' f32 [n, dim], ok [n]) as the pack kernel stages them: one f32 multiply (none without inv), one f32 subtract; what is
    no point is a zero row"""
    table = np.asarray(table, np.float32)
    rows = np.arange(table.shape[0]) if rows is None else np.asarray(rows)
    ok = (rows >= 0) & (rows < table.shape[0])
    r = np.where(ok, rows, 0)
    x = table[r] if inv is None else table[r] * np.asarray(inv, np.float32)[r][:, None]
    x = (x - np.asarray(shift, np.float32)).astype(np.float32)
    x[~ok] = 0
    return x, ok


def sums64(xp, ok, member, gamma):
    """dict(sums [3, Bp] = {AA | AB | BB}, err [3, Bp], witness [n], witness_err [n]) of the definition in include/gcnhip_driver.h,
    float64 throughout, with the bound of mmd.hip's header on every output"""
    x = np.asarray(xp, np.float64)
    n, dpad = x.shape[0], (x.shape[1] + 15) // 16 * 16
    xn = (x * x).sum(1)
    d2 = np.maximum(xn[:, None] + xn[None, :] - 2.0 * x @ x.T, 0.0)
    e_d2 = gamma_err(dpad + 3) * (xn[:, None] + xn[None, :] + 2.0 * np.abs(x) @ np.abs(x).T)
    g = float(np.float32(gamma))
    k = np.exp(-g * d2)
    e_arg = g * e_d2 + U * g * (d2 + e_d2)                 # d2's error, and the rounding of the product gamma . d2
    e_k = k * (np.exp(e_arg) * (1.0 + F32_ULP) - 1.0) + 2.0 ** -126   # expf's ulp; a denormal result may be flushed
    np.fill_diagonal(k, 1.0)
    np.fill_diagonal(e_k, 0.0)
    pair = ok[:, None] & ok[None, :]
    k, e_k = k * pair, e_k * pair
    s = (np.asarray(member) != 0) & ok[:, None]
    out = ok[:, None] & ~s
    t = k @ s
    e_t = (e_k @ s) * (1.0 + gamma_err(PART)) + gamma_err(PART) * t
    r, e_r = t[:, :1], e_t[:, :1]
    fold = (n + 64) * 2.0 ** -53
    sums = np.stack([(t * s).sum(0), (t * out).sum(0), ((r - t) * out).sum(0)])
    err = np.stack([(e_t * s).sum(0), (e_t * out).sum(0), ((e_r + e_t) * out).sum(0)]) + fold * np.stack([sums[0], sums[1], ((r + t) * out).sum(0)])
    m, rest = s[:, 1].sum(), out[:, 1].sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        wit = np.where(ok, t[:, 1] / m - (r[:, 0] - t[:, 1]) / rest, np.nan)
        e_wit = (e_t[:, 1] / m + (e_r[:, 0] + e_t[:, 1]) / rest) * (1 + 4 * U) + 2 * U * (t[:, 1] / m + r[:, 0] / rest) + 2.0 ** -126
    return dict(sums=sums, err=err, witness=wit, witness_err=e_wit, m=int(m), rest=int(rest))


def stats64(sums, m, rest):
    """(biased [cols], unbiased [cols], p) by the formulas of host/mmd.h from sums [3, cols]"""
    aa, ab, bb = np.asarray(sums, np.float64)
    biased = aa / m ** 2 + bb / rest ** 2 - 2 * ab / (m * rest)
    with np.errstate(divide="ignore", invalid="ignore"):
        unbiased = (aa - m) / (m * (m - 1)) + (bb - rest) / (rest * (rest - 1)) - 2 * ab / (m * rest) if m > 1 and rest > 1 else np.full(aa.shape, np.nan)
    return biased, unbiased, (1 + int((biased[1:] >= biased[0]).sum())) / biased.size


def membership(n, m, perms, rng, pad_to=None):
    """0/1 [n, 2 + perms (padded with zero columns to pad_to)]: ones, the first m positions, `perms` random groups of m positions"""
    s = np.zeros((n, pad_to or 2 + perms), bool)
    s[:, 0], s[:m, 1] = True, True
    for p in range(perms):
        s[rng.permutation(n)[:m], 2 + p] = True
    return s


def whole64(x, m, perms, seed, gamma=None):
    """the whole test in float64 on the host: (biased statistic, p) of rows x [n, d] whose first m are group A"""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    xc = x - x.mean(0)
    g = (n - 1) / (2.0 * (xc * xc).sum()) if gamma is None else gamma
    res = sums64((x - x.mean(0)).astype(np.float32), np.ones(n, bool), membership(n, m, perms, np.random.default_rng(seed)), g)
    biased, _, p = stats64(np.delete(res["sums"], 0, 1), m, n - m)
    return biased[0], p
