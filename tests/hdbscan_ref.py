"""Float64 reference of HDBSCAN as include/gcnhip_driver.h and host/hdbscan.h define it: core2 by a sort of the float64 d2, Kruskal over
the edges sorted by (w, lo, hi), then scikit-learn's condensed tree, EOM / leaf selection, labels and probabilities.  numpy only."""
import numpy as np


def core2(d2, min_samples):
    """the d2 to the (min_samples - 1)-th nearest other point (the sorted row holds the point itself first); 0 where no point"""
    ok = np.isfinite(np.diag(d2))
    return np.where(ok, np.sort(d2, axis=1)[:, min_samples - 1], 0.0)


def mst(d2, c2):
    """(lo, hi, w) of the minimum spanning tree of the points under w = max(d2, core2_i, core2_j) and (w, lo, hi), sorted by it"""
    w = np.maximum(d2, np.maximum(c2[:, None], c2[None, :]))
    ok = np.isfinite(np.diag(w))
    lo, hi = np.triu_indices(w.shape[0], 1)
    keep = ok[lo] & ok[hi]
    lo, hi = lo[keep], hi[keep]
    order = np.lexsort((hi, lo, w[lo, hi]))
    root = np.arange(w.shape[0])

    def find(x):
        while root[x] != x:
            root[x] = root[root[x]]
            x = root[x]
        return x
    out, need = [], int(ok.sum()) - 1
    for e in order:
        if len(out) == need:
            break
        a, b = find(lo[e]), find(hi[e])
        if a != b:
            root[max(a, b)] = min(a, b)
            out.append(e)
    out = np.array(out, np.int64)
    return lo[out].astype(np.int32), hi[out].astype(np.int32), w[lo[out], hi[out]]


def linkage(lo, hi, dist):
    """rows (left, right, distance, size) of a sorted tree on points 0..p-1; `left`: the end nearer to point 0 (scikit-learn's Prim)"""
    p = len(lo) + 1
    nbr = [[] for _ in range(p)]
    for a, b in zip(lo, hi):
        nbr[a].append(b)
        nbr[b].append(a)
    depth, queue = np.r_[0, np.full(p - 1, -1)], [0]
    for a in queue:
        for b in nbr[a]:
            if depth[b] < 0:
                depth[b] = depth[a] + 1
                queue.append(b)
    size, rows, parent = [1] * (2 * p - 1), [], list(range(2 * p - 1))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for e, (a, b) in enumerate(zip(lo, hi)):
        if depth[a] > depth[b]:
            a, b = b, a
        l, r = find(a), find(b)
        parent[l] = parent[r] = p + e
        size[p + e] = size[l] + size[r]
        rows.append((l, r, dist[e], size[p + e]))
    return rows


def bfs(rows, p, node):
    out, queue = [], [node]
    while queue:
        out += queue
        queue = [c for x in queue if x >= p for c in rows[x - p][:2]]
    return out


def condense(rows, p, mcs):
    """scikit-learn's _condense_tree: rows (parent, child, lambda, size) in its order"""
    root = 2 * (p - 1)
    relabel, nxt, out, ignore = {root: p}, p + 1, [], set()
    for node in bfs(rows, p, root):
        if node in ignore or node < p:
            continue
        l, r, d, _ = rows[node - p]
        lam = 1.0 / d if d > 0 else np.inf
        nl, nr = (rows[c - p][3] if c >= p else 1 for c in (l, r))
        for c, cnt, other in ((l, nl, nr), (r, nr, nl)):
            if cnt >= mcs and other >= mcs:
                relabel[c] = nxt
                nxt += 1
                out.append((relabel[node], relabel[c], lam, cnt))
            elif cnt >= mcs:
                relabel[c] = relabel[node]
            else:
                for s in bfs(rows, p, c):
                    if s < p:
                        out.append((relabel[node], s, lam, 1))
                    ignore.add(s)
    return out


def tree(lo, hi, d2, n, min_cluster_size=5, method="eom", allow_single_cluster=False):
    """labels, probabilities [n] and the linkage of the sorted tree (lo, hi, d2) over n list positions"""
    labels, prob = np.full(n, -1, np.int32), np.zeros(n)
    pts = np.unique(np.concatenate([lo, hi]))                     # at least one edge
    p = len(pts)
    rows = linkage(np.searchsorted(pts, lo), np.searchsorted(pts, hi), np.sqrt(np.asarray(d2, np.float64)))
    cond = condense(rows, p, min_cluster_size)
    n_cl = max(max(r[0] for r in cond), max(r[1] for r in cond)) - p + 1
    birth, stab, par, kids = np.full(n_cl, np.nan), np.zeros(n_cl), {}, {c: [] for c in range(p, p + n_cl)}
    birth[0] = 0.0
    for pa, ch, lam, sz in cond:
        if ch >= p:
            birth[ch - p] = lam
            par[ch] = pa
            kids[pa].append(ch)
    for pa, ch, lam, sz in cond:
        stab[pa - p] += (lam - birth[pa - p]) * sz
    nodes = list(range(p + n_cl - 1, p - (1 if allow_single_cluster else 0), -1))
    chosen = {c: True for c in nodes}
    if method == "eom":
        for c in nodes:
            sub = sum(stab[k - p] for k in kids[c])
            if sub > stab[c - p]:
                chosen[c] = False
                stab[c - p] = sub
            else:
                stack = list(kids[c])
                while stack:
                    k = stack.pop()
                    chosen[k] = False
                    stack += kids[k]
    else:
        chosen = {c: not kids[c] and c != p for c in nodes}
    clusters = sorted(c for c in chosen if chosen[c])
    number = {c: k for k, c in enumerate(clusters)}
    death, cur, best = np.zeros(n_cl), cond[0][0], cond[0][2]     # scikit-learn's max_lambdas: the LAST run of a parent's rows wins
    for pa, ch, lam, sz in cond[1:]:
        if pa == cur:
            best = max(best, lam)
        else:
            death[cur - p], cur, best = best, pa, lam
    death[cur - p] = best
    root_max = max(lam for pa, ch, lam, sz in cond if pa == p)
    for pa, ch, lam, sz in cond:
        if ch >= p:
            continue
        c = pa
        while c not in number and c != p:                         # the first kept cluster above the point
            c = par[c]
        if c in number and (c != p or lam >= root_max):         # the root as the single cluster keeps its densest points only
            labels[pts[ch]] = number[c]
            prob[pts[ch]] = 1.0 if death[c - p] == 0.0 or np.isinf(lam) else min(lam, death[c - p]) / death[c - p]
    return dict(labels=labels, probabilities=prob, linkage=np.array([(min(l, r), max(l, r), d, s) for l, r, d, s in rows], np.float64))


def run(d2, min_cluster_size=5, min_samples=None, **kw):
    c2 = core2(d2, min_samples or min_cluster_size)
    lo, hi, w = mst(d2, c2)
    return dict(tree(lo, hi, w, d2.shape[0], min_cluster_size, **kw), lo=lo, hi=hi, w=w, core2=c2)
