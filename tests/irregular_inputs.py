"""Adjacencies and sparse feature matrices as data files really give them, plus a float64 reference of the three products.

The loader promises no regularity: `parseGraph` writes the self loop first and then the neighbours in FILE
order, so a row may be unsorted, list a neighbour twice, list the node itself again, or list j without row j listing it
back; an svmlight line may repeat a feature id or list ids in any order.  The reference's semantics on such input: degree =
stored row length (repeats included), a repeated entry contributes twice, forward and backward are the same row gather.

Everything here is host-side numpy, shared by test_irregular_cpu.py and test_irregular_gpu.py.

One reading note on `irregular_features`: "a column that never occurs" and "a row that is a permutation of ALL F columns"
cannot hold in one matrix, so they are variants — missing="last" / "first" leave columns unused (column F-1 / column 0
among them) and carry a row that permutes every column that IS in use; missing=None carries the permutation of all F.
Every other property is in every variant.
"""
import numpy as np

SEED_GRAPH, SEED_FEAT, SEED_MODEL = 20240611, 20240612, 20240613     # the seeds the GPU tests use (the CPU test checks these)


# ------------------------------------------------------------------------------------------------------------- generators
def irregular_graph(rng, n, hub_len=2500, rep_len=300, label=None):
    """(indptr, indices) int32 in the loader's layout: row i = [i, neighbours in drawn order].

    Contains, by construction (graph_properties counts each of them again from the arrays alone):
    shuffled neighbour order; pairs (i, j) stored twice; row `rep` listing one neighbour rep_len times; rows that list
    themselves again; >= 10 % of the stored edges without their mirror; rows with the self loop only; row `hub` of
    hub_len stored entries over fewer than 1 024 distinct neighbours (above the split length only through repeats); and a
    node no other row references.  label: optional classes, 70 % of the drawn neighbours then share the row's class."""
    assert n >= 200 and hub_len > 1024
    hub, rep, lonely = 0, 1, 2
    nbrs = [[] for _ in range(n)]

    def draw(i, k):
        out = rng.integers(0, n, k)
        if label is not None:
            same = np.flatnonzero(label == label[i])
            pick = rng.random(k) < 0.7
            out[pick] = same[rng.integers(0, same.size, int(pick.sum()))]
        return out

    # mutual edges (both directions stored) and one-directional ones
    for i in range(n):
        for j in draw(i, int(rng.integers(0, 5))):
            if j != i:
                nbrs[i].append(int(j)); nbrs[int(j)].append(i)
    for i in range(n):
        nbrs[i].extend(int(j) for j in draw(i, int(rng.integers(0, 6))) if j != i)
    special = {hub, rep, lonely}
    free = np.array([i for i in rng.permutation(n) if i not in special])
    only_self, again, twice = free[:n // 20], free[n // 20:n // 10], free[n // 10:n // 5]
    for i in again:                                         # the node itself, once or twice more
        nbrs[i].extend([int(i)] * int(rng.integers(1, 3)))
    for i in twice:                                         # a pair that occurs twice
        if nbrs[i]:
            nbrs[i].append(nbrs[i][int(rng.integers(0, len(nbrs[i])))])
    # one row that lists a single neighbour hundreds of times, among a few others
    nbrs[rep] = [int(j) for j in draw(rep, 6) if j != rep] + [int(free[-1])] * rep_len
    # the hub: about n / 2 (at most 900) distinct neighbours, the rest of its length from repeats of them
    distinct = rng.choice(free, min(900, n // 2), replace=False)
    nbrs[hub] = [hub] * 3 + list(map(int, distinct)) + list(map(int, rng.choice(distinct, hub_len - 4 - distinct.size)))
    for i in only_self:
        nbrs[i] = []
    for i in range(n):                                      # nobody points at `lonely`; it keeps its own neighbours
        if i != lonely:
            nbrs[i] = [j for j in nbrs[i] if j != lonely]
    nbrs[lonely] = [int(j) for j in free[-5:]]
    rows = []
    for i in range(n):
        r = np.array(nbrs[i], np.int64)
        rng.shuffle(r)                                      # file order, not id order
        rows.append(np.concatenate([[i], r]))
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum([r.size for r in rows])
    return indptr.astype(np.int32), np.concatenate(rows).astype(np.int32)


def graph_properties(indptr, indices):
    """the irregularities of an adjacency, counted from the arrays alone"""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    n = indptr.size - 1
    deg = np.diff(indptr)
    src = np.repeat(np.arange(n), deg)
    first = np.zeros(indices.size, bool)
    first[indptr[:-1]] = True
    key = src * n + indices
    ukey, cnt = np.unique(key, return_counts=True)
    mirror = np.isin(indices * n + src, ukey)
    tail = ~first                                           # everything after the leading self loop
    unsorted_rows = sum(1 for i in range(n) if deg[i] > 2 and np.any(np.diff(indices[indptr[i] + 1:indptr[i + 1]]) < 0))
    distinct = np.array([np.unique(indices[indptr[i]:indptr[i + 1]]).size for i in range(n)])
    referenced = np.zeros(n, bool)
    referenced[indices[tail & (indices != src)]] = True
    in_deg = np.bincount(indices, minlength=n)
    return dict(self_loop_first=bool(np.all(indices[indptr[:-1]] == np.arange(n))),
                unsorted_rows=int(unsorted_rows),
                repeated_pairs=int((cnt[ukey // n != ukey % n] >= 2).sum()),
                max_repeat=int(cnt.max()),
                rows_listing_themselves_again=int(np.unique(src[tail & (indices == src)]).size),
                one_way_share=float((~mirror).sum() / indices.size),
                self_only_rows=int((deg == 1).sum()),
                hub_len=int(deg.max()), hub_distinct=int(distinct[np.argmax(deg)]),
                unreferenced_nodes_with_neighbours=int((~referenced & (deg > 1)).sum()),
                rows_where_in_degree_differs=int((in_deg != deg).sum()))


def rows_repeating_one_entry(indptr, indices, at_least=100):
    """rows in which one stored entry occurs `at_least` times or more: their sum is a run of IDENTICAL terms, whose f32
    rounding errors do not cancel (see test_irregular_cpu.test_oracle_graphsum_vs_float64)"""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    n = indptr.size - 1
    src = np.repeat(np.arange(n), np.diff(indptr))
    ukey, cnt = np.unique(src * n + indices, return_counts=True)
    return np.unique(ukey[cnt >= at_least] // n)


def irregular_features(rng, n, F, missing="last", mean_len=8, long_repeat=0):
    """CSR (indptr, indices, values) int32/int32/float32 as the svmlight loader stores it: ids in FILE order.

    Every variant: unsorted ids; ids repeated inside a row (each copy with its own value); explicit 0.0 and -0.0 values;
    empty first and last rows; row 2 = F copies of a single id; row 1 = a permutation of every column in use.
    missing="last": the last three columns never occur; "first": the first three; None: every column occurs and row 1 is a
    permutation of all F.  long_repeat > 0: row 3 lists one id that many times (a column that is long only through one row)."""
    assert n >= 8 and F >= 1 and missing in ("last", "first", None)
    n_gap = min(3, F - 1) if missing else 0
    used = np.arange(F - n_gap) if missing == "last" else np.arange(n_gap, F)
    rows = []
    for i in range(n):
        if i in (0, n - 1):
            rows.append(np.zeros(0, np.int64))
        elif i == 1:
            rows.append(rng.permutation(used))
        elif i == 2:
            rows.append(np.full(F, used[used.size // 2]))
        elif i == 3 and long_repeat:
            rows.append(np.concatenate([np.full(long_repeat, used[used.size // 3]), rng.choice(used, min(4, used.size), replace=False)]))
        else:
            k = int(rng.integers(0, 2 * mean_len + 1))
            ids = rng.choice(used, min(k, used.size), replace=False)
            if ids.size and rng.random() < 0.3:             # repeats: one id two or three more times
                ids = np.concatenate([ids, np.full(int(rng.integers(1, 4)), ids[0])])
            rng.shuffle(ids)
            rows.append(ids)
    if used.size > 1:
        while np.all(np.diff(rows[1]) > 0):
            rows[1] = rng.permutation(used)
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum([r.size for r in rows])
    indices = np.concatenate(rows).astype(np.int32)
    values = rng.standard_normal(indices.size).astype(np.float32)
    z = rng.random(indices.size)
    values[z < 0.03] = np.float32(0.0)
    values[(z >= 0.03) & (z < 0.06)] = np.float32(-0.0)
    return indptr.astype(np.int32), indices, values


def feature_properties(indptr, indices, values, F):
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    n = indptr.size - 1
    lens = np.diff(indptr)
    rows = [indices[indptr[i]:indptr[i + 1]] for i in range(n)]
    v = np.asarray(values, np.float32)
    col = np.bincount(indices, minlength=F)
    row_of = np.repeat(np.arange(n), lens)
    by_row_col = np.unique(row_of * F + indices, return_counts=True)[1]
    longest = int(np.argmax(col))
    return dict(unsorted_rows=sum(1 for r in rows if r.size > 1 and np.any(np.diff(r) < 0)),
                rows_with_repeats=sum(1 for r in rows if np.unique(r).size < r.size),
                pos_zero=int(((v == 0) & ~np.signbit(v)).sum()), neg_zero=int(((v == 0) & np.signbit(v)).sum()),
                first_row_empty=bool(lens[0] == 0), last_row_empty=bool(lens[-1] == 0),
                empty_columns=np.flatnonzero(col == 0),
                full_permutation_rows=sum(1 for r in rows if r.size == F and np.unique(r).size == F and np.any(np.diff(r) < 0)),
                rows_of_F_copies=sum(1 for r in rows if r.size == F and F > 1 and np.unique(r).size == 1),
                longest_column=int(col.max()), longest_column_most_from_one_row=int(by_row_col.max()),
                longest_column_rows=int(np.unique(row_of[indices == longest]).size), nnz=int(indices.size))


def permuted_full_features(rng, n, F, row=None):
    """nnz == n.F with every row 0..F-1 in order except `row`, a non-identity permutation: NOT the dense layout.
    Returns (indptr, indices, values, row)."""
    row = n // 2 if row is None else row
    indices = np.tile(np.arange(F, dtype=np.int32), n).reshape(n, F)
    perm = rng.permutation(F)
    while F > 1 and np.array_equal(perm, np.arange(F)):
        perm = rng.permutation(F)
    indices[row] = perm
    values = rng.standard_normal(n * F).astype(np.float32)
    return (np.arange(n + 1, dtype=np.int64) * F).astype(np.int32), indices.reshape(-1), values, row


def sorted_rows(indptr, indices, values):
    """the same matrix with every row's (id, value) pairs in ascending id order (stable: repeats keep their order)"""
    indptr = np.asarray(indptr, np.int64)
    row_of = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    order = np.lexsort((np.arange(indices.size), indices, row_of))
    return indptr.astype(np.int32), np.asarray(indices, np.int32)[order], np.asarray(values, np.float32)[order]


def irregular_dataset(seed=SEED_MODEL, n=900, F=60, classes=5):
    """a dataset dict (the reference's GCNData) on irregular_graph + irregular_features with labels planted in both, so that
    training moves: 70 % of a row's drawn neighbours share its class, and every node carries a few ids of its class's block"""
    rng = np.random.default_rng(seed)
    label = rng.integers(0, classes, n).astype(np.int32)
    label[:classes] = np.arange(classes)
    gp, gi = irregular_graph(rng, n, label=label)
    fp, fi, fv = irregular_features(rng, n, F, missing="first")
    block = (F - 3) // classes
    rows, vals = [], []
    for i in range(n):
        a, b = fp[i], fp[i + 1]
        ids, v = fi[a:b], fv[a:b]
        if 3 < i < n - 1:                                   # the special rows and the empty last row stay as they are
            k = int(rng.integers(2, 6))
            own = 3 + label[i] * block + rng.integers(0, block, k)          # drawn with replacement: repeats again
            ids = np.concatenate([ids, own]).astype(np.int32)
            v = np.concatenate([v, (1.0 + 0.3 * rng.standard_normal(k))]).astype(np.float32)
            p = rng.permutation(ids.size)
            ids, v = ids[p], v[p]
        rows.append(ids); vals.append(v)
    fp = np.zeros(n + 1, np.int64)
    fp[1:] = np.cumsum([r.size for r in rows])
    split = rng.integers(1, 4, n).astype(np.int32)
    return dict(name="irregular", num_nodes=n, input_dim=F, output_dim=classes, g_indptr=gp, g_indices=gi,
                f_indptr=fp.astype(np.int32), f_indices=np.concatenate(rows).astype(np.int32),
                f_val=np.concatenate(vals).astype(np.float32), split=split, label=label)


def gpu_graph():
    """the adjacency the GPU tests aggregate on (n = 1 500, hub row of 2 500 stored entries)"""
    return irregular_graph(np.random.default_rng(SEED_GRAPH), 1500)


FEATURE_CASES = {"last": dict(n=600, F=67, missing="last"), "first": dict(n=600, F=64, missing="first"),
                 "full": dict(n=400, F=33, missing=None), "long": dict(n=300, F=40, missing="last", long_repeat=4500)}


def gpu_features(case):
    """the sparse matrices the GPU tests multiply with -> (indptr, indices, values, F)"""
    kw = dict(FEATURE_CASES[case])
    n, F = kw.pop("n"), kw.pop("F")
    return irregular_features(np.random.default_rng(SEED_FEAT + sorted(FEATURE_CASES).index(case)), n, F, **kw) + (F,)


# --------------------------------------------------------------------------------------------------- float64 reference
def dense_adjacency(indptr, indices):
    """Â as a dense float64 matrix: every stored entry (r, c) adds 1 / sqrt(len(row r) . len(row c)) — module.cpp:83-101 in
    exact arithmetic; np.add.at, so a repeated entry adds twice"""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    n = indptr.size - 1
    assert n <= 3000
    deg = np.diff(indptr).astype(np.float64)
    src = np.repeat(np.arange(n), np.diff(indptr))
    a = np.zeros((n, n), np.float64)
    np.add.at(a, (src, indices), 1.0 / np.sqrt(deg[src] * deg[indices]))
    return a


def dense_features(indptr, indices, values, F):
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    n = indptr.size - 1
    assert n <= 3000
    x = np.zeros((n, F), np.float64)
    np.add.at(x, (np.repeat(np.arange(n), np.diff(indptr)), indices), np.asarray(values, np.float64))
    return x


class dense_reference:
    """plain float64 numpy forms of the three products, each with the same product on absolute values (the `mag` argument
    of test_ops_gpu.close_mag).  The absolute-value matrices are built from |stored values| entry by entry, so two copies of
    one id with opposite signs do not cancel in the magnitude."""

    @staticmethod
    def graphsum(indptr, indices, x):
        a = dense_adjacency(indptr, indices)
        x = np.asarray(x, np.float64)
        return a @ x, a @ np.abs(x)

    @staticmethod
    def spmm_fwd(indptr, indices, values, F, w):
        w = np.asarray(w, np.float64)
        return dense_features(indptr, indices, values, F) @ w, dense_features(indptr, indices, np.abs(values), F) @ np.abs(w)

    @staticmethod
    def spmm_bwd(indptr, indices, values, F, dout):
        d = np.asarray(dout, np.float64)
        return dense_features(indptr, indices, values, F).T @ d, dense_features(indptr, indices, np.abs(values), F).T @ np.abs(d)

    @staticmethod
    def model_forward(ds, w1, w2, split=1, weight_decay=5e-4):
        """(reported loss over the rows of `split`, accuracy, logits) of the two-layer forward without dropout:
        Z = Â ReLU(Â X W1) W2 (gcn.cpp:21-54), mean cross-entropy as CrossEntropyLoss::forward (module.cpp:124-161) plus the
        L2 penalty weight_decay . |W1|^2 / 2 the reference adds to every reported loss (gcn.cpp:98-105)"""
        a = dense_adjacency(ds["g_indptr"], ds["g_indices"])
        x = dense_features(ds["f_indptr"], ds["f_indices"], ds["f_val"], ds["input_dim"])
        h = np.maximum(a @ (x @ np.asarray(w1, np.float64)), 0)
        z = a @ (h @ np.asarray(w2, np.float64))
        rows = np.flatnonzero(np.asarray(ds["split"]) == split)
        zs = z[rows] - z[rows].max(1, keepdims=True)
        t = np.asarray(ds["label"])[rows]
        loss = float((np.log(np.exp(zs).sum(1)) - zs[np.arange(rows.size), t]).mean())
        loss += weight_decay * float((np.asarray(w1, np.float64) ** 2).sum()) / 2
        return loss, float((z[rows].argmax(1) == t).mean()), z
