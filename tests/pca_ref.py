"""References for the PCA tests: the planted spectrum (x = (z . s) Q + offset, below), the scatter matrix in numpy.longdouble, the formulas
host/pca.h states (written out independently), the test matrices of the eigen solver and the two ratios it is held to."""
import numpy as np

EPS = 2.0 ** -52
U = 2.0 ** -53
PART = 1024                                # PCA_PART of csrc/pca.hip: part of the definition of the sums' order
SPECTRUM = [16, 8, 4, 2, 1.5, 1, .75, .5]


def spectrum(h):
    return np.array((SPECTRUM + [0.1] * h)[:h], np.float64)


def orthogonal(h, rng):
    q, r = np.linalg.qr(rng.standard_normal((h, h)))
    return q * np.sign(np.diag(r))


def planted(n, h, seed):
    """x = (z . s) Q + offset as f32: z standard normal, s the planted spectrum, Q random orthogonal, offset uniform in [0, 3)"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, h))
    return ((z * spectrum(h)) @ orthogonal(h, rng) + rng.uniform(0, 3, h)).astype(np.float32)


def planted_scatter(h, seed, n=1000):
    """the exactly symmetric float64 scatter matrix of a planted table"""
    x = planted(n, h, seed).astype(np.float64)
    c = x - x.mean(0)
    s = c.T @ c
    return (s + s.T) / 2


def rows_used(table, rows=None, inv_norm=None):
    """(x f32 [valid, dim] as the kernels form it, valid mask by list position)"""
    t = np.asarray(table, np.float32)
    r = np.arange(t.shape[0]) if rows is None else np.asarray(rows, np.int64)
    ok = (r >= 0) & (r < t.shape[0])
    x = t[r[ok]]
    if inv_norm is not None:
        x = (x * np.asarray(inv_norm, np.float32)[r[ok]][:, None]).astype(np.float32)
    return x, ok


def mean_ref(x):
    return (x.astype(np.longdouble).sum(0) / max(x.shape[0], 1)).astype(np.float64)


def scatter_ref(x, mean=None):
    """(S in longdouble rounded to float64, |c|^T |c| in float64) with c = (double)x - mean formed in float64, as defined"""
    c = x.astype(np.float64) - (0.0 if mean is None else np.asarray(mean, np.float64))
    cl = c.astype(np.longdouble)
    return (cl.T @ cl).astype(np.float64), np.abs(c).T @ np.abs(c)


def scatter_bound(n, absprod):
    return (n + 2) * U * absprod


def project_ref(x, mean, components, scale=None):
    """(y_ref float64 [n, k], the bound (h + 2) 2^-53 |scale| sum |c| |v| + 2^-24 |y_ref| on |y - y_ref|: h + 1 float64 roundings of the chain and the scale, one to f32)"""
    c = x.astype(np.float64) - (0.0 if mean is None else np.asarray(mean, np.float64))
    v = np.asarray(components, np.float64)
    sc = np.ones(v.shape[0]) if scale is None else np.asarray(scale, np.float64)
    y = ((c.astype(np.longdouble) @ v.T.astype(np.longdouble)) * sc.astype(np.longdouble)).astype(np.float64)
    h = x.shape[1]
    bound = (h + 2) * U * np.abs(sc) * (np.abs(c) @ np.abs(v.T)) + 2.0 ** -24 * np.abs(y)
    return y, bound


# ---- the eigen solver -----------------------------------------------------------------------------------------------------------

def residual_ratio(s, lam, v):
    h = s.shape[0]
    nf = np.linalg.norm(s)
    if nf == 0:
        return float(np.abs(s @ v - v * lam).max())
    return float(np.linalg.norm(s @ v - v * lam, axis=0).max() / (h * EPS * nf))


def orthogonality_ratio(v):
    h = v.shape[0]
    return float(np.abs(v.T @ v - np.eye(h)).max() / (h * EPS))


def residual_norms(s, lam, v):
    return np.linalg.norm(s @ v - v * lam, axis=0)


def sign_rule(v):
    """each column's entry of largest magnitude is positive, the lowest index on equal magnitude"""
    top = np.argmax(np.abs(v), axis=0)
    return bool(np.all(v[top, np.arange(v.shape[1])] > 0))


def eigh_desc(s):
    w, u = np.linalg.eigh(s)
    return w[::-1].copy(), u[:, ::-1].copy()


def solver_matrices(h, seed=0):
    """name -> symmetric float64 [h, h]: the cases the solver is held to"""
    rng = np.random.default_rng(1000 * h + seed)
    p = planted_scatter(h, seed + h)
    v = rng.standard_normal(h)
    half = h // 2
    q = orthogonal(h, rng)
    block = (q * np.array([3.0] * half + [1.0] * (h - half))) @ q.T        # two repeated eigenvalues, rotated
    block = (block + block.T) / 2
    g = rng.standard_normal((h, h))
    return {
        "planted": p,
        "diagonal": np.diag(rng.uniform(-2, 5, h)),
        "zero": np.zeros((h, h)),
        "rank1": np.outer(v, v),
        "cI": 2.5 * np.eye(h),
        "block": block,
        "indefinite": (g + g.T) / 2,
        "planted_1e-30": p * 1e-30,
        "planted_1e+30": p * 1e+30,
    }


# ---- what a fit derives from a scatter matrix ---------------------------------------------------------------------------------

def from_scatter_ref(lam_raw, rows, k, whiten=False):
    """host/pca.h's formulas on a solver's descending eigenvalues"""
    h = lam_raw.size
    lam = np.maximum(np.asarray(lam_raw, np.float64), 0.0)
    total = lam.sum()
    out = dict(eigenvalues=lam, explained_variance=lam / (rows - 1), explained_variance_ratio=lam / total if total > 0 else np.zeros(h),
               singular_values=np.sqrt(lam), rank=int(np.sum(lam > h * EPS * lam[0])))
    if whiten:
        sc = np.zeros(k)
        r = min(k, out["rank"])
        sc[:r] = 1.0 / np.sqrt(lam[:r] / (rows - 1))
        out["scale"] = sc
    return out
