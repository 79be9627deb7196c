"""Node embeddings on the GPU: the kernels of csrc/embed.hip through ops.py — exactly, on small-integer tables whose every dot
product is an integer, and within the derived bound of tests/embed_ref.py on real-valued ones — then the model's embed / similar
/ score_edges against the reference on the model's own rows, what the embeddings are for (neighbours in the planted community),
no side effects on training, refusals, and the command line (GCN_EMBED, GCN_SIMILAR)."""
import os
import subprocess
import threading

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import embed_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def dev():
    from cuda_gcn_amd.ops import Device
    d = Device(0)
    yield d
    d.close()


# ---- kernels, exact cases -------------------------------------------------------------------------------------------------

def integer_table(n, dim, seed):
    """entries in {-3..3}; at least 30 % of the rows are copies of other rows, scattered so that ties straddle chunk boundaries"""
    rng = np.random.default_rng(seed)
    t = rng.integers(-3, 4, (n, dim)).astype(np.float32)
    if n >= 10:
        where = rng.choice(n, (3 * n + 9) // 10, replace=False)
        t[where] = t[rng.integers(0, n, where.size)]
    return t


def exact_answer(scores, q_rows, k, ids_of, exclude_self):
    """np.lexsort((ids, -scores))[:k] per query on the integer score matrix"""
    n = scores.shape[0]
    out_i = np.full((len(q_rows), k), -1, np.int32)
    out_s = np.full((len(q_rows), k), -np.inf, np.float32)
    for i, q in enumerate(q_rows):
        s = scores[q]
        order = np.lexsort((ids_of, -s))
        if exclude_self:
            order = order[order != q]
        order = order[:k]
        out_i[i, :order.size] = ids_of[order]
        out_s[i, :order.size] = s[order]
    return out_i, out_s


def query_rows(n, nq, seed):
    q = np.random.default_rng(seed).integers(0, n, nq).astype(np.int32)
    if nq > 1:
        q[-1] = q[0]                                              # a repeated query row
    return q


@pytest.mark.parametrize("dim", [1, 5, 16, 41, 128, 256])
def test_topk_is_exact_on_integer_tables(dev, dim):
    """n = 1000, both row strides (one that is no multiple of 4: the element-wise loads; one that is: the 16-byte loads with an
    element-wise tail), NaN in the padding, every chunk_rows x nq x k of the issue, ids through a permutation"""
    n = 1000
    t = integer_table(n, dim, dim)
    scores = (t.astype(np.int64) @ t.astype(np.int64).T).astype(np.float32)
    perm = np.random.default_rng(dim + 1).permutation(n).astype(np.int32)
    combo = 0
    for chunk_rows in (0, 64, 256, 333):
        for nq in (1, 19, 67):
            q = query_rows(n, nq, 7 * nq + chunk_rows)
            for k in (1, 10, 64):
                ld = dim + 3 if combo % 2 else (dim + 3) // 4 * 4 + 4
                row_id = perm if combo % 3 else None
                exclude = combo % 5 != 4
                combo += 1
                ids, sc, plan = dev.topk_rows(t, q, k, row_id=row_id, exclude_self=exclude, chunk_rows=chunk_rows, ld=ld, plan=True)
                want_i, want_s = exact_answer(scores, q, k, perm if row_id is not None else np.arange(n, dtype=np.int32), exclude)
                assert np.array_equal(ids, want_i) and same_bits(sc, want_s), (chunk_rows, nq, k, ld, row_id is not None, exclude)
                assert plan["n_chunks"] == (1 if chunk_rows == 0 else -(-n // chunk_rows))
    ids2, sc2 = dev.topk_rows(t, q, 64, row_id=perm, chunk_rows=64, ld=dim + 3)
    ids3, sc3 = dev.topk_rows(t, q, 64, row_id=perm, chunk_rows=64, ld=dim + 3)
    assert same_bits(ids2, ids3) and same_bits(sc2, sc3)


@pytest.mark.parametrize("chunk_rows,k", [(77, 10), (50, 10), (143, 10), (500, 33), (22, 7)])
def test_merge_with_a_last_round_shorter_than_k(dev, chunk_rows, k):
    """Shapes whose n_chunks . k leaves 1 .. k - 1 entries for the merge's last round of 64 (13 chunks x 10 = 130 = 2 x 64 + 2),
    so that lane k - 1 holds no entry there, with the decisive scores at or below zero: row 0 is (3, 3, 3, 3, 3), every other row
    is negative, and the rows whose dots with it are largest (-6 .. 0) sit at the end of the table, in the last chunk, under
    small permuted ids.  Random queries ride along (their dots have both signs)."""
    n, dim = 1000, 5
    assert 0 < (-(-n // chunk_rows) * k) % 64 < k
    rng = np.random.default_rng(chunk_rows)
    t = rng.integers(-3, 0, (n, dim)).astype(np.float32)
    t[0] = 3
    t[n - 40:] = 0
    t[n - 40:, 0] = -rng.integers(0, 3, 40)                       # dots 0, -3, -6 with row 0, many ties
    perm = np.arange(n, dtype=np.int32)[::-1].copy()              # the last rows carry the smallest ids
    scores = (t.astype(np.int64) @ t.astype(np.int64).T).astype(np.float32)
    q = np.concatenate([[0], rng.integers(0, n, 18)]).astype(np.int32)
    for row_id in (perm, None):
        ids, sc = dev.topk_rows(t, q, k, row_id=row_id, chunk_rows=chunk_rows, ld=dim + 3)
        want_i, want_s = exact_answer(scores, q, k, perm if row_id is not None else np.arange(n, dtype=np.int32), True)
        assert want_s[0, 0] == 0 and np.all(want_s[0] <= 0)
        assert np.array_equal(ids, want_i) and same_bits(sc, want_s), (chunk_rows, k, row_id is not None)
    # a general table of both signs at the same shapes
    t2 = integer_table(n, 41, chunk_rows)
    s2 = (t2.astype(np.int64) @ t2.astype(np.int64).T).astype(np.float32)
    ids, sc = dev.topk_rows(t2, q, k, row_id=perm, exclude_self=False, chunk_rows=chunk_rows, ld=44)
    want_i, want_s = exact_answer(s2, q, k, perm, False)
    assert np.array_equal(ids, want_i) and same_bits(sc, want_s)


def test_topk_with_fewer_candidates_than_k(dev):
    """n = 37 with k = 64: -1 / -inf past the candidates; n = 1 with exclude_self: nothing at all; a query row outside the table"""
    t = integer_table(37, 5, 0)
    scores = (t.astype(np.int64) @ t.astype(np.int64).T).astype(np.float32)
    q = np.array([0, 36, 5, 5], np.int32)
    for exclude, filled in ((True, 36), (False, 37)):
        for chunk_rows in (0, 16):
            ids, sc = dev.topk_rows(t, q, 64, exclude_self=exclude, chunk_rows=chunk_rows, ld=8)
            want_i, want_s = exact_answer(scores, q, 64, np.arange(37, dtype=np.int32), exclude)
            assert np.array_equal(ids, want_i) and same_bits(sc, want_s)
            assert np.all(ids[:, filled:] == -1) and np.all(np.isneginf(sc[:, filled:])) and np.all(ids[:, :filled] >= 0)
    one = np.array([[2.0, -1.0, 3.0]], np.float32)
    ids, sc = dev.topk_rows(one, [0, 0], 5)
    assert np.all(ids == -1) and np.all(np.isneginf(sc))
    ids, sc = dev.topk_rows(one, [0], 5, exclude_self=False)
    assert ids.tolist() == [[0, -1, -1, -1, -1]] and sc[0, 0] == 14.0
    ids, sc = dev.topk_rows(t, [3, 37, -1], 4)
    assert np.all(ids[1:] == -1) and np.all(np.isneginf(sc[1:])) and np.all(ids[0] >= 0)


def test_topk_in_batches_has_the_bits_of_one_pass(dev):
    """a scratch that holds one tile of 64 queries: 131 queries are answered in three batches, with the same bits"""
    t = integer_table(1000, 41, 3)
    q = query_rows(1000, 131, 1)
    ids, sc, plan = dev.topk_rows(t, q, 10, chunk_rows=128, ld=44, plan=True)
    assert plan["scratch_bytes"] == 3 * plan["scratch_bytes_min"] and plan["n_chunks"] == 8
    ids2, sc2 = dev.topk_rows(t, q, 10, chunk_rows=128, ld=44, scratch_bytes=plan["scratch_bytes_min"])
    assert same_bits(ids, ids2) and same_bits(sc, sc2)
    from cuda_gcn_amd.ops import GcnHipError
    with pytest.raises(GcnHipError, match="gcnhip_topk_rows: the scratch holds no tile"):
        dev.topk_rows(t, q, 10, chunk_rows=128, ld=44, scratch_bytes=plan["scratch_bytes_min"] - 8)


# ---- kernels, bounded cases -----------------------------------------------------------------------------------------------

def real_table(n, dim, seed):
    """standard-normal rows after a ReLU; row 2 all zero; row 9 a copy of row 4"""
    x = np.maximum(np.random.default_rng(seed).standard_normal((n, dim)), 0).astype(np.float32)
    x[2] = 0
    x[9] = x[4]
    return x


@pytest.mark.parametrize("n,dim,chunk_rows", [(1000, 41, 128), (1000, 128, 128), (20011, 128, 0)])
def test_kernels_hold_the_bound_on_real_tables(dev, n, dim, chunk_rows):
    """inverse norms, top-k under both metrics, pair scores and the export gather against float64 within the bounds of
    tests/embed_ref.py; the same bits on a second launch of every kernel.  20 011 rows is the smallest size the suite uses at
    which the automatic split must cut the table (its chunks hold at most 16 384 rows)."""
    x = real_table(n, dim, n + dim)
    ld = dim + 7
    # inverse norms
    inv = dev.embed_inv_norms(x, ld=ld)
    r64 = R.inv_norms64(x)
    assert inv[2] == 0 and inv.dtype == np.float32
    assert np.all(np.abs(inv - r64) <= R.inv_norm_bound(dim) * r64)
    assert same_bits(inv, dev.embed_inv_norms(x, ld=ld))
    # top-k: the zero row, the duplicated pair and a repeated query among the queries
    q = np.concatenate([[2, 4, 9, 4], np.random.default_rng(1).integers(0, n, 63)]).astype(np.int32)
    for metric, norms in (("dot", None), ("cosine", inv)):
        ids, sc, plan = dev.topk_rows(x, q, 10, inv_norm=norms, chunk_rows=chunk_rows, ld=ld, plan=True)
        assert plan["n_chunks"] > 1, plan
        R.check_topk(x, q, ids, sc, metric)
        ids2, sc2 = dev.topk_rows(x, q, 10, inv_norm=norms, chunk_rows=chunk_rows, ld=ld)
        assert same_bits(ids, ids2) and same_bits(sc, sc2)
        assert same_bits(ids[1], ids[3]) and same_bits(sc[1], sc[3])          # the repeated query
    # pair scores
    rng = np.random.default_rng(2)
    src, dst = rng.integers(0, n, 500), rng.integers(0, n, 500)
    src, dst = np.concatenate([src, np.arange(20)]), np.concatenate([dst, np.arange(20)])
    for metric, norms in (("dot", None), ("cosine", inv)):
        got = dev.pair_scores(x, src, dst, inv_norm=norms, ld=ld)
        s64, E = R.pair_scores64(x, src, dst, metric)
        assert np.all(np.abs(got - s64) <= E), float((np.abs(got - s64) - E).max())
        assert same_bits(got, dev.pair_scores(x, src, dst, inv_norm=norms, ld=ld))
        if metric == "cosine":
            assert got[500 + 2] == 0 and np.all(np.abs(np.delete(got[500:], 2) - 1) <= (2 * dim + 16) * R.U)
    # the export gather
    rows = np.array([5, 2, 2, n - 1, 0], np.int32)
    assert same_bits(dev.embed_rows(x, rows, ld=ld), x[rows]) and same_bits(dev.embed_rows(x, ld=ld, ld_out=dim + 1), x)
    unit = dev.embed_rows(x, rows, inv_norm=inv, ld=ld)
    assert same_bits(unit, x[rows] * inv[rows][:, None]) and same_bits(unit, dev.embed_rows(x, rows, inv_norm=inv, ld=ld))


def test_kernel_refusals(dev):
    from cuda_gcn_amd.ops import GcnHipError
    x = real_table(20, 8, 0)
    for k in (0, 65):
        with pytest.raises(GcnHipError, match=r"gcnhip_topk_plan: 1 <= k <= 64"):
            dev.topk_rows(x, [0], k)
    tb, ob = dev.padded(x, 8), dev.buf(np.zeros(20, np.float32))  # (the wrapper pads: the entry point itself, with a short stride)
    assert dev.lib.gcnhip_embed_inv_norms(dev.ctx, tb.ptr, 7, 20, 8, ob.ptr) == -1
    assert b"gcnhip_embed_inv_norms: the row stride is below dim" in dev.lib.gcnhip_last_error()
    wide = np.zeros((3, 257), np.float32)
    with pytest.raises(GcnHipError, match="gcnhip_topk_rows: 1 <= dim <= 256"):
        dev.topk_rows(wide, [0], 2)
    with pytest.raises(GcnHipError, match="gcnhip_pair_scores: 1 <= dim <= 256"):
        dev.pair_scores(wide, [0], [1])


# ---- the model ------------------------------------------------------------------------------------------------------------

PLANTED_EPOCHS = 30
# float64 reference on the CPU oracle's weights (seed 5, no dropout, 30 epochs, hidden 16) of this graph: share of a node's 10
# cosine neighbours inside its own planted community, for the raw features and for the hidden layer
REF_SHARE_X, REF_SHARE_H1 = 0.3306, 0.7396


def planted():
    return datagen.planted_communities(n_comm=8, size=128, p_in=0.5, feats=8)


@pytest.fixture(scope="module")
def trained_planted():
    """the case of the calibration test: 8 communities of 128 nodes, hidden 16, no dropout"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = planted()
    m = HipGCNModel(ds, seed=5, hidden_dim=16, dropout=0.0)
    m.run_epochs(PLANTED_EPOCHS, want_trace=False)
    yield ds, m
    m.close()


def rows_by_node(m, v):
    ids, _ = m.row_ids()
    out = np.empty_like(v)
    out[ids] = v
    return out


def check_model_embeddings(ds, m):
    n, h = ds["num_nodes"], m.params.hidden_dim
    m.eval(3)
    want = rows_by_node(m, m.var(3))
    emb = m.embed()
    assert emb.shape == (n, h) and same_bits(emb, want)
    assert same_bits(m.var(3), m.var(3)) and same_bits(rows_by_node(m, m.var(3)), emb)      # variable 3 holds the same matrix afterwards
    q = np.array([5, 3, 3, n - 1, 0], np.int32)
    assert same_bits(m.embed(nodes=q), emb[q]) and m.embed(nodes=[]).shape == (0, h)
    unit = m.embed(normalize=True)
    norm = np.sqrt((unit.astype(np.float64) ** 2).sum(axis=1))
    zero = ~emb.any(axis=1)
    assert np.all(norm[zero] == 0) and np.all(np.abs(norm[~zero] - 1) <= h * R.U)
    assert same_bits(m.embed(nodes=q, normalize=True), unit[q])
    # neighbours and pair scores against the reference on the model's own rows
    q = np.concatenate([q, np.random.default_rng(0).integers(0, n, 59)]).astype(np.int32)
    for metric in ("cosine", "dot"):
        ids, sc = m.similar(q, k=10, metric=metric)
        R.check_topk(emb, q, ids, sc, metric)
        ids_self, sc_self = m.similar(q, k=3, metric=metric, exclude_self=False)
        R.check_topk(emb, q, ids_self, sc_self, metric, exclude_self=False)
        src, dst = np.concatenate([q, q]), np.concatenate([q[::-1], q])
        got = m.score_edges(src, dst, metric=metric)
        s64, E = R.pair_scores64(emb, src, dst, metric)
        assert np.all(np.abs(got - s64) <= E)
    assert m.score_edges([], []).shape == (0,)
    return emb


def test_model_embeddings_on_the_planted_graph(trained_planted):
    """embed() has the bits of var(3) after eval(3) in node order (a dense X: the aggregate-first hidden layer alone); node
    queries, normalised rows, similar() and score_edges() against the reference on those rows"""
    ds, m = trained_planted
    check_model_embeddings(ds, m)


@pytest.mark.parametrize("kind", ["sparse", "multilabel", "wide"])
def test_model_embeddings_on_other_models(kind):
    """a sparse X (no aggregate-first form: the whole hooked forward stores the matrix), a multi-label model, hidden width 128"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.make_dataset("cora-syn" if kind != "multilabel" else "tiny-syn")
    kw = dict(hidden_dim=128 if kind == "wide" else 16, dropout=0.5)
    if kind == "multilabel":
        kw["multilabel"] = np.random.default_rng(0).random((ds["num_nodes"], ds["output_dim"])) < 0.3
    m = HipGCNModel(ds, seed=5, **kw)
    m.run_epochs(3, want_trace=False)
    check_model_embeddings(ds, m)
    m.close()


def test_neighbours_lie_in_the_planted_community(trained_planted):
    """What it is for.  In the float64 reference on the CPU oracle's weights 33.06 % of a node's 10 cosine neighbours by raw
    features lie in its own community and 73.96 % by the hidden layer (REF_SHARE_*).  Here: the float64 reference on the model's
    own rows shows more than half of that gain, and similar()'s neighbours differ from the reference's in their own-community
    count by no more than the number of queries whose 10th and 11th reference scores lie within 2 E — below 1 % of the queries."""
    ds, m = trained_planted
    n = ds["num_nodes"]
    q = np.arange(n)
    group = ds["label"]
    emb = m.embed()
    x = ds["f_val"].reshape(n, -1)
    ref_ids = R.topk64(emb, q, 10, "cosine")
    share_x = R.own_group_share(R.topk64(x, q, 10, "cosine"), group, q).mean()
    share_ref = R.own_group_share(ref_ids, group, q).mean()
    open_queries = R.near_ties(emb, q, 10, "cosine")
    ids, _ = m.similar(None, k=10, metric="cosine")
    share = R.own_group_share(ids, group, q).mean()
    print(f"planted: own-community share of 10 cosine neighbours: X {share_x:.4f}, H1 reference {share_ref:.4f}, GPU {share:.4f}; "
          f"{open_queries} of {n} queries open")
    assert share_ref - share_x > (REF_SHARE_H1 - REF_SHARE_X) / 2, (share_x, share_ref)
    assert open_queries < 0.01 * n, open_queries
    assert abs(share - share_ref) * n * 10 <= open_queries + 1e-9, (share, share_ref, open_queries)


@pytest.mark.parametrize("flags", ["0", "EVAL_LANE", "NO_GRAPH"])
def test_queries_between_epochs_change_nothing(flags):
    """3 epochs, the three queries, 2 more epochs: the bits of 5 epochs without them — traces, weights, test metrics, the logits of
    the last forward; and predict has the same bits before and after a query"""
    from cuda_gcn_amd import model as M
    f = getattr(M, flags) if flags != "0" else 0
    ds = datagen.make_dataset("cora-syn")
    a = M.HipGCNModel(ds, seed=6, flags=f, hidden_dim=16, dropout=0.5)
    b = M.HipGCNModel(ds, seed=6, flags=f, hidden_dim=16, dropout=0.5)
    ta, tb = [a.run_epochs(3)], [b.run_epochs(3)]
    before = b.predict(logp=True)
    b.embed(nodes=[4, 4, 9])
    b.similar([1, 2, 3], k=5)
    b.score_edges([1, 2], [3, 4], metric="cosine")
    b.embed(normalize=True)
    after = b.predict(logp=True)
    assert all(same_bits(x, y) for x, y in zip(before, after))
    ta.append(a.run_epochs(1))
    tb.append(b.run_epochs(1))
    b.similar(None, k=10, metric="dot")
    ta.append(np.array([a.train_epoch() + a.eval(2)], np.float32))
    tb.append(np.array([b.train_epoch() + b.eval(2)], np.float32))
    ta, tb = np.concatenate(ta), np.concatenate(tb)
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32)), (ta, tb)
    for k in (2, 5):
        assert same_bits(a.var(k), b.var(k)), k
    assert a.eval(3) == b.eval(3)
    assert same_bits(a.var(6), b.var(6)) and same_bits(a.var(3), b.var(3))
    a.close()
    b.close()


def test_refusals():
    """k = 0 and 65, an unknown metric, node id N, two logical ranks: GcnHostError naming the method, from the Python front end and
    from the C entry points called directly"""
    from cuda_gcn_amd.model import HipGCNModel, GcnHostError, _ck
    from tests.mr_threads import ThreadWorld
    ds = datagen.make_dataset("tiny-syn")
    n = ds["num_nodes"]
    m = HipGCNModel(ds, seed=1, hidden_dim=16)
    ids, sc, out = np.zeros(4 * 64, np.int32), np.zeros(4 * 64, np.float32), np.zeros(4 * 16, np.float32)
    ok, bad = np.array([0, 1], np.int32), np.array([0, n], np.int32)

    def similar(nodes=ok, k=5, metric=1):
        return m.lib.gcnhost_model_similar(m.h, nodes.ctypes.data, 2, k, metric, 1, ids.ctypes.data, sc.ctypes.data)
    for k in (0, 65, "ten", 2.5, None):
        with pytest.raises(GcnHostError, match="similar: k must be"):
            m.similar([0, 1], k=k)
    for k in (0, 65):
        with pytest.raises(GcnHostError, match=r"similar: k must be in 1\.\.64"):
            _ck(m.lib, similar(k=k), "call")
    for call in (lambda: m.similar([0], metric="l2"), lambda: m.score_edges([0], [1], metric="euclid")):
        with pytest.raises(GcnHostError, match="the metric is 'dot' or 'cosine'"):
            call()
    with pytest.raises(GcnHostError, match=r"similar: the metric is 0 \(dot\) or 1 \(cosine\)"):
        _ck(m.lib, similar(metric=2), "call")
    with pytest.raises(GcnHostError, match=r"score_pairs: the metric is 0 \(dot\) or 1 \(cosine\)"):
        _ck(m.lib, m.lib.gcnhost_model_score_pairs(m.h, ok.ctypes.data, ok.ctypes.data, 2, -1, out.ctypes.data), "call")
    for what, call in (("embed", lambda: m.embed(nodes=[0, n])), ("similar", lambda: m.similar([n])), ("score_edges", lambda: m.score_edges([0], [n])),
                       ("similar", lambda: m.similar([-1]))):
        with pytest.raises(GcnHostError, match=f"{what}: .*not a node of the dataset"):
            call()
    for what, rc in (("embed", lambda: m.lib.gcnhost_model_embed(m.h, bad.ctypes.data, 2, out.ctypes.data, 0)), ("similar", lambda: similar(nodes=bad)),
                     ("score_pairs", lambda: m.lib.gcnhost_model_score_pairs(m.h, ok.ctypes.data, bad.ctypes.data, 2, 0, out.ctypes.data))):
        with pytest.raises(GcnHostError, match=f"{what}: node {n} is not a node of the dataset"):
            _ck(m.lib, rc(), "call")
    m.close()
    # two logical ranks: every query is refused on each
    tw = ThreadWorld(2)
    seen, errors = [None, None], []

    def body(rank):
        try:
            ag, ar = tw.callbacks(rank)
            r = HipGCNModel(ds, seed=4, device=0, rank=rank, world=2, host_allgather=ag, host_allreduce=ar, hidden_dim=16, dropout=0.5)
            msgs = []
            for call in (lambda: r.embed(nodes=[0]), lambda: r.similar([0]), lambda: r.score_edges([0], [1])):
                try:
                    call()
                    msgs.append("no error")
                except GcnHostError as e:
                    msgs.append(str(e))
            seen[rank] = msgs
            r.close()
        except BaseException as e:                                # a failed rank must not leave the other at a barrier forever
            errors.append((rank, e))
            tw.barrier.abort()
    threads = [threading.Thread(target=body, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for msgs in seen:
        assert "embed: one rank only" in msgs[0] and "similar: one rank only" in msgs[1] and "score_pairs: one rank only" in msgs[2], msgs


# ---- the command line -----------------------------------------------------------------------------------------------------

def test_cli_embed_and_similar(tmp_path):
    """gcn-hip cora-syn with GCN_EMBED and GCN_SIMILAR: stdout keeps its lines; the files parse to the Python calls on the same
    weights (handed over through a weights file, 0 epochs)"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.make_dataset("cora-syn")
    n = ds["num_nodes"]
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "cora-syn.gcnbin"))
    m = HipGCNModel(ds, seed=3, hidden_dim=16, dropout=0.5)
    m.run_epochs(6, want_trace=False)
    w = str(tmp_path / "w.gcnw")
    m.save_weights(w)
    emb = m.embed()
    ids, sc = m.similar(None, k=10, metric="cosine")
    m.close()
    args = ["cora-syn", "-", "-", "16", "-", "0.5", "-", "-", "0"]
    e, s = str(tmp_path / "e.txt"), str(tmp_path / "s.txt")
    env = dict(os.environ, GCN_SEED="3", GCN_LOAD_WEIGHTS=w, GCN_EMBED=e, GCN_SIMILAR=s)
    r = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1].startswith("test_loss=")
    rows = np.loadtxt(e, ndmin=2)
    assert rows.shape == (n, 17) and np.array_equal(rows[:, 0], np.arange(n))
    assert same_bits(rows[:, 1:].astype(np.float32), emb)         # %.9g round-trips an f32
    lines = open(s).read().strip().splitlines()
    assert len(lines) == n
    for i, line in enumerate(lines):
        parts = line.split()
        assert int(parts[0]) == i and len(parts) == 11
        got_i = [int(p.split(":")[0]) for p in parts[1:]]
        got_s = np.array([float(p.split(":")[1]) for p in parts[1:]], np.float32)
        assert got_i == ids[i].tolist() and same_bits(got_s, sc[i]), i
    bad = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=dict(env, GCN_GPUS="2"), capture_output=True, text=True)
    assert bad.returncode != 0 and "GCN_EMBED / GCN_SIMILAR run on one GPU" in bad.stderr, bad.stderr[-500:]
