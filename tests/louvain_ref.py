"""The definitions of csrc/louvain.hip in Python integers and dicts, and nothing else.

A LEVEL is a weighted graph on n vertices: rows[v] = sorted [(u, w)], u distinct, u != v, w > 0; self_w[v].  Level 0 is the sets
S(v) of tests/overlap_ref.py with w = 1 and self_w = 0; no transpose is built (the quantity is the textbook modularity exactly
when the stored graph is symmetric).
k[v] = self_w[v] + sum w(v, .);  M2 = sum k;  for a labelling comm: tot[c] = sum of k over c, in[c] = sum over v in c of
(self_w[v] + sum of w(v, u), u in c);  num = M2 . sum in - sum tot^2;  Q = num / M2^2 (0 when M2 = 0).
A SWEEP s is synchronous: every vertex reads comm, tot, size of the sweep's start.  v in a: candidates c != a with K(v, c) =
sum of w(v, u), comm[u] = c, positive; only c > a on even s, c < a on odd s; not when size[a] = size[c] = 1 and c > a;
gain(c) = K(v, c) M2 - k[v] tot[c]; stay = K(v, a) M2 - k[v] (tot[a] - k[v]); v moves to the largest gain (ties: smallest c) iff it
is > stay.  A sweep after which num did not strictly rise is undone; a level ends after two undone sweeps in a row or max_sweeps
sweeps, and starts from singletons.
COARSENING: communities renumbered by ascending smallest member; w(C, D) = sum of w(v, u), v in C, u in D, C != D; self_w[C] =
in[C]; rows sorted.  The coarse rows are stored ragged: row C has room for bound[C] = min(sum of its members' row lengths,
coarse vertices - 1) entries, ptr = the prefix sums of bound."""


def level0(S):
    return [[(u, 1) for u in sorted(s)] for s in S], [0] * len(S)


def numerator(rows, self_w, comm):
    """(num, M2, tot) of a labelling"""
    n = len(rows)
    k = [self_w[v] + sum(w for _, w in rows[v]) for v in range(n)]
    tot, inner = [0] * n, 0
    for v in range(n):
        tot[comm[v]] += k[v]
        inner += self_w[v] + sum(w for u, w in rows[v] if comm[u] == comm[v])
    m2 = sum(k)
    return m2 * inner - sum(t * t for t in tot), m2, tot


def level(rows, self_w, max_sweeps=100):
    """one level from singletons to its end: (comm, tot, num, sweeps, moved)"""
    n = len(rows)
    comm = list(range(n))
    num, m2, tot = numerator(rows, self_w, comm)
    k, size = list(tot), [1] * n
    sweeps, undone, moved = 0, 0, False
    while m2 and sweeps < max_sweeps and undone < 2:
        nxt = list(comm)
        for v in range(n):
            a, K = comm[v], {}
            for u, w in rows[v]:
                K[comm[u]] = K.get(comm[u], 0) + w
            best = None
            for c, kc in K.items():
                if c == a or (c < a if sweeps % 2 == 0 else c > a) or (size[a] == 1 and size[c] == 1 and c > a):
                    continue
                gain = kc * m2 - k[v] * tot[c]
                if best is None or gain > best[0] or (gain == best[0] and c < best[1]):
                    best = (gain, c)
            if best and best[0] > K.get(a, 0) * m2 - k[v] * (tot[a] - k[v]):
                nxt[v] = best[1]
        new_num, _, new_tot = numerator(rows, self_w, nxt)
        sweeps += 1
        if new_num > num:
            comm, tot, num, undone, moved = nxt, new_tot, new_num, 0, True
            size = [0] * n
            for c in comm:
                size[c] += 1
        else:
            undone += 1
    return comm, tot, num, sweeps, moved


def coarsen(rows, self_w, comm):
    """(label per vertex, coarse rows, coarse self_w, ptr)"""
    n = len(rows)
    first = {}
    for v in range(n):
        first.setdefault(comm[v], v)
    order = {c: i for i, c in enumerate(sorted(first, key=first.get))}
    label = [order[comm[v]] for v in range(n)]
    nc = len(order)
    acc, self2, room = [{} for _ in range(nc)], [0] * nc, [0] * nc
    for v in range(n):
        C = label[v]
        self2[C] += self_w[v]
        room[C] += len(rows[v])
        for u, w in rows[v]:
            if label[u] == C:
                self2[C] += w
            else:
                acc[C][label[u]] = acc[C].get(label[u], 0) + w
    ptr = [0]
    for C in range(nc):
        ptr.append(ptr[-1] + min(room[C], nc - 1))
    return label, [sorted(a.items()) for a in acc], self2, ptr


def louvain(S, max_levels=32, max_sweeps=100):
    """(labels, [(vertices, sweeps, num)] per level, num, M2)"""
    rows, self_w = level0(S)
    labels, records, num, m2 = list(range(len(S))), [], 0, sum(len(s) for s in S)
    for _ in range(max_levels):
        comm, _, num, sweeps, moved = level(rows, self_w, max_sweeps)
        records.append((len(rows), sweeps, num))
        if not moved:
            break
        label, rows, self_w, _ = coarsen(rows, self_w, comm)
        labels = [label[c] for c in labels]
    return labels, records, num, m2
