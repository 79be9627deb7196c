"""One GraphSum call in float64, field for field of the launch record (GsCall, csrc/graphsum.hip), and the planted graph
the option table runs on (test_graphsum_options_cpu.py proves both before a GPU sees them, test_graphsum_options_gpu.py
holds every kernel path to them).  Plain numpy, dense: graphs of a few hundred nodes only."""
import numpy as np

# stored row lengths (self loop included) of the planted hubs; with a segment length of 16 they give
# ceil(deg / 16) = 1, 2, 3, 4, 4, 5, 6, 7, 8, 9, 10 and 19 segments
HUB_DEGREES = (16, 17, 33, 49, 64, 65, 81, 100, 128, 129, 145, 300)
SPLIT = 16


def planted_graph(n=400, seed=5):
    """-> (indptr, indices, hubs): a symmetric graph in the loader's layout (self loop first).  hubs[i] has exactly
    HUB_DEGREES[i] stored entries and only leaf neighbours; the last six nodes carry only their self loop; leaf-leaf edges
    are sparse and random."""
    from cuda_gcn_amd import datagen
    rng = np.random.default_rng(seed)
    n_lonely = 6
    hubs = np.sort(rng.choice(n - n_lonely, len(HUB_DEGREES), replace=False))
    leaves = np.setdiff1d(np.arange(n - n_lonely), hubs)
    lo, hi = [], []
    for h, d in zip(hubs, HUB_DEGREES):
        nb = rng.choice(leaves, d - 1, replace=False)
        lo.append(np.full(d - 1, h)); hi.append(nb)
    lo.append(rng.choice(leaves, 150)); hi.append(rng.choice(leaves, 150))
    a, b = datagen._unique_undirected(np.concatenate(lo), np.concatenate(hi), n)
    indptr, indices = datagen.csr_with_self_loops(a, b, n)
    return indptr, indices, hubs


def planted_row_sets(indptr, hubs, seed=17):
    """-> (rows A, rows B, in_rows): two row selections — leaves at random; of the hubs A takes the degrees 17, 33, 64, 65, 100,
    129 and 300, B takes 17, 33, 49, 64, 81, 128 and 145, so the hubs of degree 65 and 300 are inside A and outside B, every
    segment count is selected at least once and each selection leaves split rows out — and the rows of the input that count
    as non-zero (the degree-300 hub among them)"""
    n = np.asarray(indptr).size - 1
    rng = np.random.default_rng(seed)
    a, b, nz = rng.random(n) < 0.4, rng.random(n) < 0.5, rng.random(n) < 0.6
    for sel, degs in ((a, (17, 33, 64, 65, 100, 129, 300)), (b, (17, 33, 49, 64, 81, 128, 145))):
        sel[hubs] = [d in degs for d in HUB_DEGREES]
    nz[hubs[HUB_DEGREES.index(300)]] = True
    return a, b, nz


def segments(indptr, split=SPLIT):
    """segments per row under a segment length of `split` (plan.h cut_segments): 1 = the row is not cut"""
    deg = np.diff(np.asarray(indptr, np.int64))
    return np.where(deg > split, (deg + split - 1) // split, 1)


def dinv_f32(indptr):
    """(dinv_row, dinv2_row) as gcnhip_graph_create stores them: float64 1/sqrt(deg) and 1/deg, narrowed to f32"""
    deg = np.maximum(np.diff(np.asarray(indptr, np.int64)), 1).astype(np.float64)
    return (1.0 / np.sqrt(deg)).astype(np.float32), (1.0 / deg).astype(np.float32)


def dense_operators(indptr, indices, keep_cols=None):
    """(A, A01) dense float64 [n, n]: coef(r, c) = 1 / sqrt(deg_r . deg_c) per stored entry and the entry counts; a repeated
    entry counts twice, deg = stored row length of the FULL graph; keep_cols (bool per column): the other columns are dropped"""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    n = indptr.size - 1
    deg = np.diff(indptr).astype(np.float64)
    src = np.repeat(np.arange(n), np.diff(indptr))
    a, a01 = np.zeros((n, n), np.float64), np.zeros((n, n), np.float64)
    np.add.at(a, (src, indices), 1.0 / np.sqrt(deg[src] * deg[indices]))
    np.add.at(a01, (src, indices), 1.0)
    if keep_cols is not None:
        off = ~np.asarray(keep_cols, bool)
        a[:, off] = 0.0
        a01[:, off] = 0.0
    return a, a01


def dropout_scale(p):
    """1 / (1 - p) in f32, as the launch computes it (module.cpp:212)"""
    return np.float32(1) / (np.float32(1) - np.float32(p))


def keep_decisions(n, dim, training, p=0.0, seed=0, epoch=0, elem_offset=0, keep_mask=None):
    """bool [n, dim]: the keep decision of element r . dim + c — from keep_mask when given, else from the Philox stream"""
    if not training:
        return np.ones((n, dim), bool)
    if keep_mask is not None:
        return np.asarray(keep_mask).reshape(n, dim) != 0
    from tests.test_ops_gpu import philox_keep, thr_of
    idx = np.arange(n * dim, dtype=np.uint64) + np.uint64(elem_offset)
    return philox_keep(seed, epoch, idx, thr_of(p)).reshape(n, dim)


def graphsum_ref(indptr, indices, x, *, keep_cols=None, rows=None, in_row_bits=None, out_row_bits=None, accumulate=0, prev=None,
                 scaling=0, relu_dropout=0, training=0, p=0.0, seed=0, epoch=0, elem_offset=0, keep_mask=None, keep=None,
                 cache=None, x_key=None):
    """-> (want, mag, touched) of one call, in float64.

    x [n, dim] (a bf16 table: pass the rounded values); keep_cols: a restricted operator; rows / out_row_bits: bool per
    row, the registered subset and the output-row bits; in_row_bits: bool per row of x, False = the row counts as zero;
    accumulate + prev: what `out` held; scaling 0: A . x, 1 / 2 / 3: (A01 . x) . dinv_row / dinv2_row / 1 with the f32
    factors of the object; relu_dropout, training, p, seed, epoch, elem_offset, keep_mask: the store epilogue (keep: the
    decisions already made, bool [n, dim]).  mag is the same expression on absolute values; touched marks the rows the
    call writes, every other row of want and mag is 0.  cache (a dict) + x_key: the dense operators and the two products
    of this (x, in_row_bits, keep_cols) are kept there between calls."""
    x = np.asarray(x, np.float64)
    n, dim = x.shape
    cache = cache if cache is not None else {}
    kc = None if keep_cols is None else np.asarray(keep_cols, bool).tobytes()
    ib = None if in_row_bits is None else np.asarray(in_row_bits, bool).tobytes()
    if ("ops", kc) not in cache:
        cache[("ops", kc)] = dense_operators(indptr, indices, keep_cols)
    a, a01 = cache[("ops", kc)]
    pk = ("prod", x_key, kc, ib, scaling != 0)
    if x_key is None or pk not in cache:
        xz = x if in_row_bits is None else np.where(np.asarray(in_row_bits, bool)[:, None], x, 0.0)
        op = a01 if scaling else a
        cache[pk] = (op @ xz, op @ np.abs(xz))
    s, m = cache[pk]
    if accumulate:
        s, m = np.asarray(prev, np.float64) + s, np.abs(np.asarray(prev, np.float64)) + m
    if scaling in (1, 2):
        post = dinv_f32(indptr)[scaling - 1].astype(np.float64)[:, None]
        s, m = s * post, m * post
    if relu_dropout:
        s = np.maximum(s, 0.0)
        if training:
            if keep is None:
                keep = keep_decisions(n, dim, training, p, seed, epoch, elem_offset, keep_mask)
            scale = float(dropout_scale(p))
            s, m = np.where(keep, s * scale, 0.0), m * scale
    touched = np.ones(n, bool)
    if rows is not None:
        touched &= np.asarray(rows, bool)
    if out_row_bits is not None:
        touched &= np.asarray(out_row_bits, bool)
    return np.where(touched[:, None], s, 0.0), np.where(touched[:, None], m, 0.0), touched


def pack_positive(out):
    """uint32 [n, dim / 32]: bit (c & 31) of word c >> 5 = (out[r, c] > 0)"""
    n, dim = out.shape
    return np.packbits((out > 0).reshape(n, dim // 32, 32), axis=2, bitorder="little").view(np.uint32).reshape(n, dim // 32)
