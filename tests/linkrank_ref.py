"""Plain reference for the link prediction ranks (csrc/linkrank.hip), in int64 / float64 numpy.

Query i = (s, d).  Candidates: every row c of the table except d, s (exclude_self) and the members of the filter set of row s.
above = #{c : score(s, c) > score(s, d)}, equal = #{c : score(s, c) == score(s, d)}; -1 / -1 when s or d is no row.
"""
import numpy as np


def integer_table(n, dim, seed, unit=False):
    """entries in {-3..3} (unit: in {-1, 1}, so that every row has the squared norm dim and equal dots stay equal cosines); at least
    30 % of the rows are copies of other rows, scattered so that ties straddle tile and chunk edges"""
    rng = np.random.default_rng(seed)
    t = (rng.integers(0, 2, (n, dim)) * 2 - 1 if unit else rng.integers(-3, 4, (n, dim))).astype(np.float32)
    if n >= 10:
        where = rng.choice(n, (3 * n + 9) // 10, replace=False)
        t[where] = t[rng.integers(0, n, where.size)]
    return t


def filter_sets(n, chunk_rows, src, dst, seed):
    """(x_ptr int32 [n + 1], x_ids int32, sets) — a sorted, distinct id set per table row, cycling through the kinds a walk in chunks
    of chunk_rows rows and tiles of 64 can get wrong: empty; the row's own query ends; columns 0 and 63 of a tile and the first and last
    row of a chunk; a whole tile; more than 64 members; ids outside the table.  Ids >= n arise on small tables too: they are ignored."""
    rng = np.random.default_rng(seed)
    cb = chunk_rows if 0 < chunk_rows < n else 0                 # the second chunk's first row (the first's when there is one chunk)
    ce = min(n, cb + (chunk_rows or n))
    d_of = {int(s): int(d) for s, d in zip(src[::-1], dst[::-1]) if 0 <= s < n}
    sets = []
    for r in range(n):
        kind = r % 6
        ids = [[], [r, d_of.get(r, r)], [0, cb, cb + 63, cb + 64, ce - 1, n - 1], range(cb + 64, cb + 128), range(max(cb - 20, 0), cb + 100),
               [-5, -1, n, n + 7] + list(rng.integers(0, n, 5))][kind]
        sets.append(np.unique(np.asarray(list(ids), np.int64)).astype(np.int32))
    x_ptr = np.zeros(n + 1, np.int32)
    np.cumsum([s.size for s in sets], out=x_ptr[1:])
    return x_ptr, np.concatenate(sets).astype(np.int32), sets


def link_ranks(scores_of, n, src, dst, sets=None, exclude_self=True):
    """(above, equal, removed_above, removed_equal) int64 [nq]; scores_of(s) = the scores of row s against every row.  removed_*: what
    the candidates taken out by the filter alone would have counted."""
    out = np.full((4, len(src)), -1, np.int64)
    for i, (s, d) in enumerate(zip(src, dst)):
        if not (0 <= s < n and 0 <= d < n):
            continue
        sc = np.asarray(scores_of(int(s)))
        cand = np.ones(n, bool)
        cand[d] = False
        if exclude_self:
            cand[s] = False
        gone = np.zeros(n, bool)
        if sets is not None:
            m = sets[s][(sets[s] >= 0) & (sets[s] < n)]
            gone[m] = True
        gone &= cand
        cand &= ~gone
        out[:, i] = (sc[cand] > sc[d]).sum(), (sc[cand] == sc[d]).sum(), (sc[gone] > sc[d]).sum(), (sc[gone] == sc[d]).sum()
    return out


def metrics(above, equal, ks):
    """the float64 metrics of the valid queries: (rank, mrr, mean_rank, hits)"""
    a, e = np.asarray(above, np.float64), np.asarray(equal, np.float64)
    ok = (a >= 0) & (e >= 0)
    rank = 1.0 + a[ok] + e[ok] / 2.0
    if not rank.size:
        return rank, 0.0, 0.0, {k: 0.0 for k in ks}
    return rank, float((1.0 / rank).mean()), float(rank.mean()), {k: float((rank <= k).mean()) for k in ks}
