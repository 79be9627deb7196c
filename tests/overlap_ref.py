"""The definitions of csrc/overlap.hip in Python sets and integers, and nothing else.

S(v) = the distinct u stored in row v with u != v and 0 <= u < n_rows; d(v) = |S(v)|; no transpose is built.
t2(v) = sum over u in S(v) of |S(v) & S(u)|; D(v) = d (d - 1); c(v) = t2 / D, 0 when d < 2.
A pair (a, b): cn = |S(a) & S(b)|, un = d(a) + d(b) - cn, wsum = sum of wt[w] over the common w; an end outside the rows gives
zeros and counts in skipped.  totals = [listed rows in range, rows with d >= 2, sum d, sum D, sum t2, max t2, max d, ratio_sum],
ratio_sum = sum over rows with d >= 2 of floor(t2 * 2^32 / D)."""
import math


def sets(indptr, indices):
    n = len(indptr) - 1
    return [{int(u) for u in indices[indptr[v]:indptr[v + 1]] if u != v and 0 <= u < n} for v in range(n)]


def rows(S, listed=None):
    """(t2, deg by list position, totals, skipped)"""
    n = len(S)
    t2, deg, tot, skipped = [], [], [0] * 8, 0
    for v in (range(n) if listed is None else listed):
        if not 0 <= v < n:
            skipped += 1
            t2.append(0)
            deg.append(0)
            continue
        t, d = sum(len(S[v] & S[u]) for u in S[v]), len(S[v])
        D = d * (d - 1)
        t2.append(t)
        deg.append(d)
        tot[0] += 1
        tot[2] += d
        tot[3] += D
        tot[4] += t
        tot[5] = max(tot[5], t)
        tot[6] = max(tot[6], d)
        if d >= 2:
            tot[1] += 1
            tot[7] += (t << 32) // D
    return t2, deg, tot, skipped


def pairs(S, src, dst, wt=None):
    """(cn, un, wsum, skipped)"""
    n = len(S)
    cn, un, ws, skipped = [], [], [], 0
    for a, b in zip(src, dst):
        if not (0 <= a < n and 0 <= b < n):
            skipped += 1
            cn.append(0), un.append(0), ws.append(0)
            continue
        common = S[a] & S[b]
        cn.append(len(common))
        un.append(len(S[a]) + len(S[b]) - len(common))
        ws.append(sum(int(wt[w]) for w in common) if wt is not None else 0)
    return cn, un, ws, skipped


def metrics(tot):
    """triangles, transitivity, avg_clustering from the totals; a zero denominator gives 0"""
    return tot[4] // 6, (tot[4] / tot[3] if tot[3] else 0.0), (tot[7] / 2.0 ** 32 / tot[0] if tot[0] else 0.0)


def weight_table(deg, kind):
    """the fixed-point table of a link score: round(2^32 / ln d) for adamic_adar (d >= 2), round(2^32 / d) for
    resource_allocation (d >= 1), 0 otherwise"""
    if kind == "adamic_adar":
        return [int(round(2.0 ** 32 / math.log(d))) if d >= 2 else 0 for d in deg]
    return [int(round(2.0 ** 32 / d)) if d >= 1 else 0 for d in deg]
