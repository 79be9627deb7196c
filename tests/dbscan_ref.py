"""Float64 reference of DBSCAN as include/gcnhip_driver.h defines it (csrc/dbscan.hip): brute-force d2 of the f32 rows the kernel
sees, counts, core points, components by a plain search, border points, noise and the numbering.  numpy only."""
import numpy as np

from tests.tsne_ref import scaled_rows


def dist2(xs, ok):
    """d2 float64 [n, n] of the f32 rows xs; +inf where either position is no point; the diagonal is 0 at a point"""
    a = xs.astype(np.float64)
    xn = (a * a).sum(axis=1)
    d = np.maximum((xn[:, None] + xn[None, :]) - 2.0 * (a @ a.T), 0.0)
    np.fill_diagonal(d, 0.0)                                      # the self pair is a neighbour by position
    d[~ok, :] = np.inf
    d[:, ~ok] = np.inf
    return d


def counts(d2, eps2_list):
    """int32 [E, n]: the neighbourhood sizes, the point itself included; 0 where the position is no point"""
    return np.stack([(d2 <= e).sum(axis=1) for e in eps2_list]).astype(np.int32)


def dbscan(d2, eps2, min_samples):
    n = d2.shape[0]
    ok = np.isfinite(np.diag(d2))
    near = d2 <= eps2
    count = near.sum(axis=1).astype(np.int32)
    core = ok & (count >= min_samples)
    comp = np.full(n, -1, np.int64)
    for i in np.flatnonzero(core):                                # ascending: a component is named by its smallest position
        if comp[i] >= 0:
            continue
        comp[i] = i
        stack = [i]
        while stack:
            for j in np.flatnonzero(near[stack.pop()] & core & (comp < 0)):
                comp[j] = i
                stack.append(j)
    border, ambiguous = np.zeros(n, bool), 0
    for i in np.flatnonzero(ok & ~core):
        c = comp[near[i] & core]
        if c.size:
            border[i], comp[i] = True, c.min()                    # scikit-learn's visiting order: the first cluster to reach it
            ambiguous += np.unique(c).size > 1
    roots = np.unique(comp[comp >= 0])
    labels = np.where(comp >= 0, np.searchsorted(roots, comp), -1).astype(np.int32)
    return dict(labels=labels, core=core, counts=count, sizes=np.bincount(labels[labels >= 0], minlength=roots.size).astype(np.int32),
                n_clusters=int(roots.size), n_core=int(core.sum()), n_border=int(border.sum()), n_noise=int((ok & ~core & ~border).sum()),
                points=int(ok.sum()), ambiguous=int(ambiguous))


KEYS = ("labels", "core", "counts", "sizes", "n_clusters", "n_core", "n_border", "n_noise", "points")


def same(got, want):
    """the keys of `got` that differ from the reference"""
    return [k for k in KEYS if not np.array_equal(np.asarray(got[k]), np.asarray(want[k]))]


def bridges(dim, blocks=18):
    """per block {0, 1, 2, 3, 4, 6, 8, 9, 10, 11, 12, 50} + 100 b along the LAST column, permuted by default_rng(dim): at eps^2 = 4.5
    and min_samples 4 two clusters per block, the point at 6 a border point of both, the point at 50 noise"""
    pos = np.concatenate([np.array([0, 1, 2, 3, 4, 6, 8, 9, 10, 11, 12, 50]) + 100 * b for b in range(blocks)])
    t = np.zeros((pos.size, dim), np.float32)
    t[:, -1] = pos
    return t[np.random.default_rng(dim).permutation(pos.size)]


def intblobs(n, dim, k, seed):
    """integer centres in -8..8, noise in {-1, 0, 1}, 8 % of the rows uniform in -12..12: every d2 is an exact f32 integer"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, (k, dim))[rng.integers(0, k, n)] + rng.integers(-1, 2, (n, dim))
    out = rng.random(n) < 0.08
    x[out] = rng.integers(-12, 13, (int(out.sum()), dim))
    return x.astype(np.float32)


def gap_eps2(d2, xs, lo=0.03, hi=0.06):
    """(eps2, margin): the midpoint of the widest gap between consecutive sorted d2 values inside the lo..hi quantile window, and the
    least |d2 - eps2| / bound over all pairs, bound = (dim + 4) 2^-24 (xn_i + xn_j): above 1 no f32 d2 can fall on the other side"""
    iu = np.triu_indices(d2.shape[0], 1)
    v = d2[iu]
    xn = (xs.astype(np.float64) ** 2).sum(axis=1)
    bound = (xs.shape[1] + 4) * 2.0 ** -24 * (xn[iu[0]] + xn[iu[1]])
    fin = np.isfinite(v)
    s = np.sort(v[fin])
    w = s[int(lo * s.size):int(hi * s.size)]
    g = int(np.argmax(np.diff(w)))
    eps2 = 0.5 * (w[g] + w[g + 1])
    return eps2, float((np.abs(v[fin] - eps2) / bound[fin]).min())
