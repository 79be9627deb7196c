"""HipGCNModel.ranking on small planted datasets — a single-label model with 7 classes and a multi-label one with 40 — against
tests/ranking_ref.py on the model's own score rows: the rows are predict()'s logp (variable 6's logits on a multi-label model)
bit for bit, the integers are exact, ap_sum is within P . 2^-52 relative, the derived metrics are ranking_report's; queries with
repeats, every row, batching, a set temperature, unlabelled rows, no side effects on training, and the refusals."""
import ctypes as C
import threading

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import ranking_ref as R

pytestmark = pytest.mark.gpu
INTS = ("pos", "neg", "u2", "invalid")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_result(a, b):
    return a.keys() == b.keys() and all(same_bits(np.asarray(a[k]), np.asarray(b[k])) for k in a)


def single(epochs=10, label=None):
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.planted_communities(n_comm=7, size=64, p_in=0.5, feats=8, classes=7)
    if label is not None:
        ds = dict(ds, label=label(ds))
    m = HipGCNModel(ds, seed=5, hidden_dim=16, dropout=0.5)
    if epochs:
        m.run_epochs(epochs, want_trace=False)
    return ds, m


def multi(epochs=15):
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.planted_multilabel(n_comm=8, size=64, classes=40)
    m = HipGCNModel(ds, seed=3, hidden_dim=32, dropout=0.5, learning_rate=0.05, multilabel=ds["multilabel"])
    for _ in range(epochs):
        m.train_epoch()
    return ds, m


def listed(m, ds, split, nodes):
    """the dataset ids of the listed rows, in list order: a query as given, else local rows ascending"""
    ids, _ = m.row_ids()
    if nodes is not None:
        return np.asarray(nodes, np.int64)
    return ids if split is None else ids[ds["split"][ids] == split]


def check(m, ds, split=None, nodes=None, **kw):
    """ranking() against the reference on its own scores and the dataset's truth of the listed rows; returns the dict"""
    from cuda_gcn_amd.model import ranking_report
    r = m.ranking(split=split, nodes=nodes, return_scores=True, **kw)
    who = listed(m, ds, split, nodes)
    c = ds["output_dim"]
    truth = ds["multilabel"][who] if m.multilabel else ds["label"][who]
    assert r["rows"] == who.size and r["scores"].shape == (who.size, c) and r["scores"].dtype == np.float32
    st = R.table_stats(r["scores"], truth)
    for k in INTS:
        assert r[k].dtype == np.int64 and np.array_equal(r[k], st[k]), (k, r[k], st[k])
    assert r["unlabelled"] == st["unlabelled"]
    err, bound = np.abs(r["ap_sum"] - st["ap_sum"]), st["pos"] * 2.0 ** -52 * st["ap_sum"]
    print("ap_sum: largest error", err.max(), "of bound", bound[np.argmax(err)])
    assert np.all(err <= bound)
    rep = ranking_report(u2=r["u2"], ap_sum=r["ap_sum"], pos=r["pos"], neg=r["neg"])
    for k, v in rep.items():
        assert same_bits(np.asarray(r[k]), np.asarray(v)), k
    want = R.report(r["u2"], r["ap_sum"], r["pos"], r["neg"])
    for k, v in want.items():
        assert np.array_equal(np.asarray(r[k]), np.asarray(v)), k
    return r


def test_single_label_model():
    """the test split: scores are predict(test nodes, logp) bit for bit; the same for a query with repeats and for every row;
    one class per batch gives the same dict bit for bit; a trained planted model ranks better than chance; under a set
    temperature the scores follow predict()'s scaled logp and the metrics follow them; back at T = 1 nothing has changed"""
    ds, m = single()
    n = ds["num_nodes"]
    queries = (dict(split=3), dict(nodes=np.array([5, 3, 3, n - 1, 0, 5, 17] + list(range(0, n, 3)), np.int32)), dict())
    first = []
    for q in queries:
        r = check(m, ds, **q)
        who = listed(m, ds, q.get("split"), q.get("nodes"))
        assert same_bits(r["scores"], m.predict(nodes=who.astype(np.int32), logp=True)[2])
        assert same_result(r, m.ranking(**dict(dict(split=None), **q), return_scores=True, scratch_bytes=1))
        assert same_result(r, m.ranking(**dict(dict(split=None), **q), return_scores=True, scratch_bytes=3 * 16 * who.size))
        first.append(r)
    r = first[0]
    assert r["classes_defined"] == 7 and r["macro_auc"] > 0.5 and not r["invalid"].any() and r["unlabelled"] == 0
    assert np.array_equal(r["pos"] + r["neg"], np.full(7, r["rows"]))
    assert same_result(r, m.ranking(return_scores=True))       # the default is the test split
    empty = m.ranking(split=None, nodes=[], return_scores=True)
    assert empty["rows"] == 0 and empty["scores"].shape == (0, 7) and not empty["pos"].any() and empty["classes_defined"] == 0 and empty["macro_auc"] == 0.0
    m.set_temperature(2.0)
    for q, old in zip(queries, first):
        r = check(m, ds, **q)
        who = listed(m, ds, q.get("split"), q.get("nodes"))
        assert same_bits(r["scores"], m.predict(nodes=who.astype(np.int32), logp=True)[2]) and not same_bits(r["scores"], old["scores"])
        assert same_result(r, m.ranking(**dict(dict(split=None), **q), return_scores=True, scratch_bytes=1))
    m.set_temperature(1.0)
    for q, old in zip(queries, first):
        assert same_result(old, m.ranking(**dict(dict(split=None), **q), return_scores=True))
    m.close()


def test_multilabel_model():
    """40 classes scored on the logits: the rows of variable 6 after eval(3), matched through the local-row map; a query with
    repeats, every row, one class per batch"""
    ds, m = multi()
    n = ds["num_nodes"]
    r = check(m, ds, split=3)
    ids, _ = m.row_ids()
    m.eval(3)
    assert same_bits(r["scores"], np.ascontiguousarray(m.var(6)[ds["split"][ids] == 3][:, :40]))
    assert r["unlabelled"] == 0 and not r["invalid"].any() and np.array_equal(r["pos"] + r["neg"], np.full(40, r["rows"]))
    assert r["macro_auc"] > 0.5
    assert same_result(r, m.ranking(split=3, return_scores=True, scratch_bytes=1))
    q = np.concatenate([np.arange(0, n, 2), [7, 7, 7, n - 1]]).astype(np.int32)
    rq = check(m, ds, nodes=q)
    assert same_result(rq, m.ranking(split=None, nodes=q, return_scores=True, scratch_bytes=5 * 16 * q.size))
    ra = check(m, ds)
    assert ra["rows"] == n and same_bits(ra["scores"][np.argsort(ids)][q], rq["scores"])
    m.close()


def test_unlabelled_rows_are_in_no_class():
    """a tenth of the labels at -1: counted in `unlabelled`, in no class's positives or negatives"""
    def label(ds):
        rng = np.random.default_rng(2)
        return np.where(rng.random(ds["num_nodes"]) < 0.1, -1, ds["label"]).astype(np.int32)
    ds, m = single(epochs=0, label=label)
    for q in (dict(split=3), dict(), dict(nodes=np.arange(0, ds["num_nodes"], 2, dtype=np.int32))):
        r = check(m, ds, **q)
        who = listed(m, ds, q.get("split"), q.get("nodes"))
        assert r["unlabelled"] == (ds["label"][who] < 0).sum() > 0
        assert np.array_equal(r["pos"] + r["neg"], np.full(7, r["rows"] - r["unlabelled"]))
    m.close()


@pytest.mark.parametrize("multilabel", [False, True])
def test_ranking_between_epochs_changes_nothing(multilabel):
    """two models with the same seed train in lockstep, one calling ranking() between epochs: their run_epochs traces (the
    captured epoch graph replayed), weights, test metrics and the logits of the last forward are bit-identical, and so is the
    current split's variable 6 around a call"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.planted_multilabel(classes=41, size=128) if multilabel else datagen.make_dataset("cora-syn")
    kw = dict(seed=6, hidden_dim=16, dropout=0.5, multilabel=ds["multilabel"] if multilabel else None)
    a, b = HipGCNModel(ds, **kw), HipGCNModel(ds, **kw)
    ta, tb = [], []
    q = np.arange(0, ds["num_nodes"], 7, dtype=np.int32)
    for e in range(3):
        ta.append(a.run_epochs(1))
        tb.append(b.run_epochs(1))
        b.ranking()
        b.ranking(split=2, scratch_bytes=1 if e == 0 else 0)
        b.ranking(split=None, nodes=q, return_scores=True)
        b.ranking(split=None)
    ta.append(np.array([a.train_epoch() + a.eval(2)], np.float32))
    tb.append(np.array([b.train_epoch() + b.eval(2)], np.float32))
    ta, tb = np.concatenate(ta), np.concatenate(tb)
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32)), (ta, tb)
    for k in (2, 5):
        assert same_bits(a.var(k), b.var(k)), k
    ea = a.eval(3)
    before = b.eval(3), b.var(6)
    b.ranking()
    b.ranking(split=1)
    assert same_bits(before[1], b.var(6)) and before[0] == ea and same_bits(a.var(6), b.var(6))
    assert a.eval(3) == b.eval(3) == ea
    a.close()
    b.close()


def test_refusals():
    """65 classes, a split outside 1..3, a split and a query together, a node outside the dataset, more than 2^24 listed rows, a
    score buffer that is too small, a negative scratch cap, two ranks: an error naming the call, from the Python front end
    and from the C entry point called directly (a multi-label model above 256 classes cannot be built at all)"""
    from cuda_gcn_amd.model import HipGCNModel, GcnHostError, _ck
    from tests.mr_threads import ThreadWorld
    ds = datagen.make_dataset("tiny-syn")
    n, c = ds["num_nodes"], ds["output_dim"]

    def direct(m, split=3, nodes=None, n_nodes=0, scores=None, cap=0):
        out = [np.zeros(max(m.params.output_dim, 1), np.int64) for _ in range(4)]
        ap = np.zeros(max(m.params.output_dim, 1), np.float64)
        return m.lib.gcnhost_model_ranking(m.h, split, nodes, n_nodes, 0, out[0].ctypes.data, ap.ctypes.data, out[1].ctypes.data, out[2].ctypes.data,
                                           out[3].ctypes.data, None, None, scores, cap)

    wide = HipGCNModel(dict(ds, output_dim=65, label=(np.arange(n) % 65).astype(np.int32)), seed=1, hidden_dim=16)
    with pytest.raises(GcnHostError, match="ranking: at most 64 classes"):
        wide.ranking()
    with pytest.raises(GcnHostError, match="ranking: at most 64 classes"):
        _ck(wide.lib, direct(wide), "call")
    wide.close()
    m = HipGCNModel(ds, seed=1, hidden_dim=16)
    assert direct(m) == 0
    for bad in (0, 4, -1, "test"):
        with pytest.raises(ValueError, match="ranking: split is 1"):
            m.ranking(split=bad)
    with pytest.raises(ValueError, match="ranking: give a split or a node query, not both"):
        m.ranking(split=2, nodes=[1])
    with pytest.raises(ValueError, match="ranking: scratch_bytes must be >= 0"):
        m.ranking(scratch_bytes=-1)
    for split in (4, -1):
        with pytest.raises(GcnHostError, match="ranking: invalid argument"):
            _ck(m.lib, direct(m, split=split), "call")
    for bad in ([n], [0, -1]):
        with pytest.raises(GcnHostError, match="ranking: node .* is not a node of the dataset"):
            m.ranking(split=None, nodes=bad)
    one = np.zeros(1, np.int32)
    with pytest.raises(GcnHostError, match=r"ranking: at most 2\^24 listed rows"):
        _ck(m.lib, direct(m, split=0, nodes=one.ctypes.data, n_nodes=2 ** 24 + 1), "call")
    small = np.zeros(c, np.float32)
    with pytest.raises(GcnHostError, match="ranking: the scores need room for"):
        _ck(m.lib, direct(m, scores=small.ctypes.data, cap=small.size), "call")
    m.close()
    # two logical ranks: refused on each
    tw = ThreadWorld(2)
    seen, errors = [None, None], []

    def body(rank):
        try:
            ag, ar = tw.callbacks(rank)
            r = HipGCNModel(ds, seed=4, device=0, rank=rank, world=2, host_allgather=ag, host_allreduce=ar, hidden_dim=16, dropout=0.5)
            try:
                r.ranking()
                seen[rank] = "no error"
            except GcnHostError as e:
                seen[rank] = str(e)
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
    assert all("ranking: one rank only" in s for s in seen), seen
