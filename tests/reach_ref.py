"""The definitions of csrc/reach.hip in Python integers: the level-by-level pull traversal from a seed list, weak components by
union-find with the lowest row as label, the counts of the components, the distance strata and the measures host/reach.h derives
from them — and the small graphs the reach tests walk.  Host only; shared by test_reach_cpu.py and test_reach_gpu.py."""
import numpy as np


def stored_rows(indptr, indices):
    indptr, indices = np.asarray(indptr).tolist(), np.asarray(indices).tolist()
    return [indices[indptr[v]:indptr[v + 1]] for v in range(len(indptr) - 1)]


def hop_distance(indptr, indices, seeds, max_hops=0):
    """dict(dist, nearest int32 [n], levels, level_counts int64 [levels + 1], skipped): level L gives distance L to every row
    without a distance that stores an entry u != v of distance L - 1; nearest = the lowest seed row among those entries' own"""
    rows = stored_rows(indptr, indices)
    n = len(rows)
    dist, nearest = [-1] * n, [-1] * n
    skipped = 0
    for s in np.asarray(seeds).tolist():
        if 0 <= s < n:
            dist[s], nearest[s] = 0, s
        else:
            skipped += 1
    counts = [sum(1 for d in dist if d == 0)]
    level = 0
    while counts[-1] and (max_hops == 0 or level < max_hops):
        level += 1
        new = []
        for v in range(n):
            if dist[v] >= 0:
                continue
            best = None
            for u in rows[v]:
                if u != v and 0 <= u < n and dist[u] == level - 1 and (best is None or nearest[u] < best):
                    best = nearest[u]
            if best is not None:
                new.append((v, best))
        for v, best in new:                                     # a level sees only the levels before it
            dist[v], nearest[v] = level, best
        counts.append(len(new))
    if counts[-1] == 0:
        counts.pop()
    counts = counts or [0]
    return dict(dist=np.array(dist, np.int32).reshape(n), nearest=np.array(nearest, np.int32).reshape(n), levels=len(counts) - 1,
                level_counts=np.array(counts, np.int64), skipped=skipped)


def components(indptr, indices):
    """comp int32 [n]: the smallest row of the weak component (every stored entry u != v of row v joins u and v)"""
    rows = stored_rows(indptr, indices)
    n = len(rows)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for v in range(n):
        for u in rows[v]:
            if u != v and 0 <= u < n:
                a, b = find(u), find(v)
                if a != b:
                    parent[max(a, b)] = min(a, b)               # the lower root stays: a root is its tree's smallest row
    return np.array([find(v) for v in range(n)], np.int32).reshape(n)


def component_counts(comp, mark=None):
    """(size int32 [n], marked int32 [n], totals int64 [6])"""
    comp = np.asarray(comp).tolist()
    n = len(comp)
    mark = [0] * n if mark is None else np.asarray(mark).tolist()
    size, marked = [0] * n, [0] * n
    for v, r in enumerate(comp):
        if 0 <= r < n:
            size[r] += 1
            marked[r] += 1 if mark[v] != 0 else 0
    roots = [v for v in range(n) if comp[v] == v]
    unmarked = [r for r in roots if marked[r] == 0]
    totals = [sum(1 for r in comp if 0 <= r < n), len(roots), max([size[r] for r in roots], default=0), len(unmarked),
              sum(size[r] for r in unmarked), sum(marked[r] for r in roots)]
    return np.array(size, np.int32).reshape(n), np.array(marked, np.int32).reshape(n), np.array(totals, np.int64)


def strata(dist, truth, num_classes, hops, nearest=None, pred=None, rows=None):
    """(strata int64 [hops + 2, 4], unlabelled)"""
    dist, truth = np.asarray(dist).tolist(), np.asarray(truth).tolist()
    n_rows = len(dist)
    nearest = None if nearest is None else np.asarray(nearest).tolist()
    pred = None if pred is None else np.asarray(pred).tolist()
    out = [[0] * 4 for _ in range(hops + 2)]
    unlabelled = 0
    for r in (range(n_rows) if rows is None else np.asarray(rows).tolist()):
        if not 0 <= r < n_rows:
            continue
        d = dist[r]
        b = hops + 1 if d < 0 else min(d, hops)
        out[b][0] += 1
        y = truth[r]
        if not 0 <= y < num_classes:
            unlabelled += 1
            continue
        out[b][1] += 1
        if pred is not None and pred[r] == y:
            out[b][2] += 1
        if nearest is not None and 0 <= nearest[r] < n_rows and truth[nearest[r]] == y:
            out[b][3] += 1
    return np.array(out, np.int64).reshape(hops + 2, 4), unlabelled


def metrics(st, hops, layers=2):
    """host/reach.h's measures from a strata table, in Python floats"""
    st = np.asarray(st).tolist()
    ratio = lambda a, b: a / b if b > 0 else 0.0

    def row(cells):
        rows, lab, ok, near = (sum(c[k] for c in cells) for k in range(4))
        return dict(rows=rows, labelled=lab, correct=ok, nearest_correct=near, accuracy=ratio(ok, lab), nearest_label_accuracy=ratio(near, lab))
    total = sum(c[0] for c in st)
    everything = row(st)
    return dict(by_distance=[row([c]) for c in st], inside_receptive_field=row(st[:layers + 1]), outside_receptive_field=row(st[layers + 1:]),
                all=everything, unreachable=st[hops + 1][0], unreachable_share=ratio(st[hops + 1][0], total),
                nearest_label_accuracy=everything["nearest_label_accuracy"], hops=hops, layers=layers)


def assert_metrics_equal(got, want):
    for key in ("unreachable", "hops", "layers"):
        assert got[key] == want[key], (key, got[key], want[key])
    for key in ("unreachable_share", "nearest_label_accuracy"):
        assert abs(got[key] - want[key]) <= 1e-15, (key, got[key], want[key])
    groups = [("inside_receptive_field", got["inside_receptive_field"], want["inside_receptive_field"]),
              ("outside_receptive_field", got["outside_receptive_field"], want["outside_receptive_field"]), ("all", got["all"], want["all"])]
    assert len(got["by_distance"]) == len(want["by_distance"])
    groups += [(("by_distance", b), g, w) for b, (g, w) in enumerate(zip(got["by_distance"], want["by_distance"]))]
    for name, g, w in groups:
        for key in ("rows", "labelled", "correct", "nearest_correct"):
            assert g[key] == w[key], (name, key, g, w)
        for key in ("accuracy", "nearest_label_accuracy"):      # one float64 division of the same two integers
            assert g[key] == w[key] and g[key] == g[key], (name, key, g, w)


# ---- graphs ------------------------------------------------------------------------------------------------------------------

def csr(n, src, dst, self_loops=True):
    """(indptr, indices) int32 with row s = [s, its dst in the order given] (the loader's layout)"""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    if self_loops:
        src, dst = np.concatenate([np.arange(n), src]), np.concatenate([np.arange(n), dst])
    order = np.argsort(src, kind="stable")
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum(np.bincount(src, minlength=n))
    return indptr.astype(np.int32), dst[order].astype(np.int32)


def path_graph(n, perm=None):
    """a path of n nodes, each pair stored both ways; perm: position p of the path is node perm[p]"""
    ids = np.arange(n) if perm is None else np.asarray(perm)
    a, b = ids[:-1], ids[1:]
    return csr(n, np.concatenate([a, b]), np.concatenate([b, a]))


def star_graph(leaves, hub_entries):
    """node 0 stores hub_entries entries over its `leaves` leaves (repeats), every leaf stores the hub"""
    n = leaves + 1
    to = 1 + np.arange(hub_entries) % leaves
    return csr(n, np.concatenate([np.zeros(hub_entries, np.int64), np.arange(1, n)]), np.concatenate([to, np.zeros(leaves, np.int64)]))


def random_mutual_graph(n, edges, seed):
    """`edges` random pairs, each stored both ways in shuffled order behind the self loop"""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n, edges), rng.integers(0, n, edges)
    keep = a != b
    a, b = a[keep], b[keep]
    src, dst = np.concatenate([a, b]), np.concatenate([b, a])
    p = rng.permutation(src.size)
    return csr(n, src[p], dst[p])


def random_seeds(n, share, seed):
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(n, max(1, int(round(n * share))), replace=False)).astype(np.int32)
