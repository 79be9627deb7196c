"""Explaining a logit on the GPU, model level: HipGCNModel.explain / feature_importance against the float64 reference of
tests/explain_ref.py evaluated on the model's own hidden rows and weights — every share within its bound, the three splits adding
up to the logit, the logit within bound of a float64 forward, default classes, batches, feature_importance, no side effects on
training, refusals — and what the shares are for: the planted feature column of the planted-communities data."""
import threading

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import explain_ref as R

pytestmark = pytest.mark.gpu

# The float64 reference on weights trained by the CPU oracle (planted_communities(8, 128, deg 16, p_in 0.5, 32 features, 8 classes,
# seed 5), hidden 16, no dropout, seed 5, 30 epochs), measured on the CPU before any GPU run by tests/validation/explain_planted_cpu.py
# (DESIGN §4.12): the share of the 193
# test nodes whose largest feature share for the predicted class is the planted column pred % feats, and the share of open queries.
REF_TOP_FEATURE, REF_OPEN = 0.9378, 0.0
PLANTED_EPOCHS = 30


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def planted():
    return datagen.planted_communities(n_comm=8, size=128, deg=16, p_in=0.5, feats=32, classes=8, seed=5)


def dense_x(ds):
    n, nf = ds["num_nodes"], ds["input_dim"]
    x = np.zeros((n, nf), np.float64)
    rows = np.repeat(np.arange(n), np.diff(ds["f_indptr"]))
    np.add.at(x, (rows, ds["f_indices"]), ds["f_val"].astype(np.float64))
    return x


class ModelReference:
    """the reference's inputs taken from a model: its own hidden rows (variable 3 as stored, the factor divided out in float64),
    its weights, and the dataset's graph and features with the coefficients the model multiplies by"""

    def __init__(self, ds, m):
        n = ds["num_nodes"]
        self.n = n
        ids, _ = m.row_ids()
        assert np.array_equal(ids, np.arange(n))                  # one rank: rows are nodes
        self.indptr, self.indices = ds["g_indptr"].astype(np.int64), ds["g_indices"].astype(np.int64)
        self.src = np.repeat(np.arange(n), np.diff(self.indptr))
        dinv32, self.factored = m.row_scale()
        deg = np.diff(self.indptr).astype(np.float64)
        if self.factored:
            d = dinv32.astype(np.float64)
            self.coef = d[self.src] * d[self.indices]
        else:
            d = np.ones(n)
            self.coef = 1.0 / np.sqrt(deg[self.src] * deg[self.indices])
        self.dinv = d
        self.w1, self.w2 = m.var(2).astype(np.float64), m.var(5).astype(np.float64)
        self.x = dense_x(ds)
        self.s, self.s_abs, self.terms = R.layer1(self.indptr, self.indices, self.coef, self.x)
        self.e_h1 = R.first_layer_bound(self.s_abs, self.w1, np.diff(self.indptr))     # a priori: explain_ref's docstring
        self.z64 = R.layer1(self.indptr, self.indices, self.coef, np.maximum(self.s @ self.w1, 0) @ self.w2)[0]

    def hidden_rows(self, m):
        return m.var(3).astype(np.float64) / self.dinv[:, None]

    def check(self, ex, nodes, h1, features=True):
        """every query of an explain() answer against the reference on hidden rows h1"""
        worst = 0.0
        for i, v in enumerate(nodes):
            a, b = int(ex["nbr_ptr"][i]), int(ex["nbr_ptr"][i + 1])
            ids = ex["nbr_ids"][a:b]
            stored = self.indices[self.indptr[v]:self.indptr[v + 1]]
            assert np.array_equal(np.sort(ids), np.sort(stored)), v    # the stored edges of the row, in the device's order
            c = int(ex["classes"][i])
            # the reference walks the row in the returned order (equal ids carry equal terms)
            ref = R.explain64(np.array([0, b - a]), ids.astype(np.int64), self.coef_of(v, ids), h1, self.w2, 0, c, w1=self.w1, s=self.s,
                              s_abs=self.s_abs, terms=self.terms, row_lengths=np.diff(self.indptr))
            got = dict(rows=ids, logit=ex["logit"][i], nbr=ex["nbr_values"][a:b], hid=ex["hidden"][i], feat=ex["features"][i] if features else None)
            assert R.violations(got, ref, features=features) == [], (v, c)
            assert R.sum_violations(got, ref, features=features) == [], (v, c)
            # the logit within bound of a float64 forward from X: the hops' bound plus the first layer's a priori rounding
            w = np.abs(self.w2[:, c])
            first = float((np.abs(self.coef_of(v, ids))[:, None] * self.e_h1[ids] * w[None, :]).sum())
            assert abs(float(ex["logit"][i]) - self.z64[v, c]) <= ref["E_logit"] + first, (v, c)
            if features:
                worst = max(worst, float(np.max(np.abs(got["feat"] - ref["feat"]) / np.maximum(ref["E_feat"], 1e-300))))
        return worst

    def check_default_classes(self, m, ex, nodes, C):
        """the default class is the argmax of the logits the stored hidden rows imply: every class explained in turn, the default
        one's logit is not below another's by more than both E_logit and, twice each, the first layer's a priori rounding (the
        class was chosen on the forward's own logits, whose hidden layer a fused launch may have rounded differently)"""
        logits, slack = np.zeros((nodes.size, C)), np.zeros((nodes.size, C))
        h1 = None
        for c in range(C):
            exc = m.explain(nodes, classes=np.full(nodes.size, c, np.int32), features=False)
            h1 = self.hidden_rows(m) if h1 is None else h1
            logits[:, c] = exc["logit"]
            for i, v in enumerate(nodes):
                a, b = int(exc["nbr_ptr"][i]), int(exc["nbr_ptr"][i + 1])
                ids = exc["nbr_ids"][a:b].astype(np.int64)
                coef = self.coef_of(v, ids)
                ref = R.explain64(np.array([0, b - a]), ids, coef, h1, self.w2, 0, c)
                slack[i, c] = ref["E_logit"] + 2 * float((np.abs(coef)[:, None] * self.e_h1[ids] * np.abs(self.w2[:, c])[None, :]).sum())
        chosen = ex["classes"]
        rows = np.arange(nodes.size)
        assert same_bits(logits[rows, chosen].astype(np.float32), ex["logit"])
        gap = logits - logits[rows, chosen][:, None]
        assert np.all(gap <= slack + slack[rows, chosen][:, None]), float(np.max(gap - slack - slack[rows, chosen][:, None]))
        clear = np.all((gap < -(slack + slack[rows, chosen][:, None])) | (np.arange(C)[None, :] == chosen[:, None]), axis=1)
        assert np.array_equal(chosen[clear], logits.argmax(1)[clear])
        return int(clear.sum())

    def coef_of(self, v, ids):
        if self.factored:
            return self.dinv[v] * self.dinv[ids]
        deg = np.diff(self.indptr).astype(np.float64)
        return 1.0 / np.sqrt(deg[v] * deg[ids])


def make_model(kind, form):
    from cuda_gcn_amd import model as M
    flags = dict(default=0, edge_coef=M.EDGE_COEF, no_agg_first=M.NO_AGG_FIRST_EVAL)[form]
    if kind == "planted":
        ds, kw, epochs = planted(), dict(hidden_dim=16, dropout=0.0), 10
    elif kind == "wide":                                          # hidden 128: the evaluation forward keeps the hidden layer in registers
        ds, kw, epochs = planted(), dict(hidden_dim=128, dropout=0.5), 5
    elif kind == "sparse":
        ds, kw, epochs = datagen.make_dataset("tiny-syn"), dict(hidden_dim=16, dropout=0.5), 5
    else:
        ds, epochs = datagen.make_dataset("tiny-syn"), 5
        kw = dict(hidden_dim=16, dropout=0.5, multilabel=np.random.default_rng(0).random((ds["num_nodes"], ds["output_dim"])) < 0.3)
    m = M.HipGCNModel(ds, seed=5, flags=flags, **kw)
    m.run_epochs(epochs, want_trace=False)
    return ds, m


@pytest.mark.parametrize("kind,form", [("planted", "default"), ("planted", "edge_coef"), ("planted", "no_agg_first"), ("sparse", "default"),
                                       ("sparse", "edge_coef"), ("multilabel", "default"), ("wide", "default")])
def test_model_explanations_against_the_reference(kind, form):
    """dense X with A^.X (the _agg path), dense X without it (the walk on a dense object), sparse X (the walk); factored and
    per-edge coefficients; single- and multi-label; hidden 128, where the forward that gives the default classes does not store
    its hidden layer and the layer's own product does"""
    ds, m = make_model(kind, form)
    n, C = ds["num_nodes"], ds["output_dim"]
    ref = ModelReference(ds, m)
    rng = np.random.default_rng(1)
    nodes = np.concatenate([[0, n - 1, 5, 5], rng.integers(0, n, 36)]).astype(np.int32)
    ex = m.explain(nodes)
    h1 = ref.hidden_rows(m)                                        # variable 3 as the query's forward left it
    assert ex["features"].shape == (nodes.size, ds["input_dim"]) and ex["hidden"].shape == (nodes.size, m.params.hidden_dim)
    worst = ref.check(ex, nodes, h1)
    print(f"{kind}/{form}: worst |feat - ref| / E_feat = {worst:.3f}")
    # default classes: predict()'s on a single-label model, the largest logit (lowest class on a tie) everywhere
    if kind != "multilabel":
        assert np.array_equal(ex["classes"], m.predict(nodes=nodes)[0])
    clear = ref.check_default_classes(m, ex, nodes, C)
    print(f"{kind}/{form}: {clear} of {nodes.size} default classes are clear of every other class's logit")
    # given classes, repeats, no features
    given = np.concatenate([[0, C - 1], rng.integers(0, C, nodes.size - 2)]).astype(np.int32)
    ex2 = m.explain(nodes, classes=given, features=False)
    assert ex2["features"] is None and np.array_equal(ex2["classes"], given)
    ref.check(dict(ex2, features=None), nodes, ref.hidden_rows(m), features=False)
    # batched equals unbatched; a query alone equals the same query inside the list; two calls give the same bits
    small = m.explain(nodes, scratch_bytes=3 * ds["input_dim"] * 4)
    again = m.explain(nodes)
    one = m.explain(nodes[7:8], classes=ex["classes"][7:8])
    for key in ("logit", "classes", "hidden", "features", "nbr_ptr", "nbr_ids", "nbr_values"):
        assert same_bits(small[key], ex[key]) and same_bits(again[key], ex[key]), key
    a, b = int(ex["nbr_ptr"][7]), int(ex["nbr_ptr"][8])
    assert same_bits(one["features"], ex["features"][7:8]) and same_bits(one["hidden"], ex["hidden"][7:8]) and same_bits(one["nbr_values"], ex["nbr_values"][a:b])
    assert m.explain([])["logit"].shape == (0,)
    # feature_importance = the mean of |explain().features| per explained class
    for split, q in ((3, np.flatnonzero(ds["split"] == 3).astype(np.int32)), (None, nodes)):
        mean_abs, count = m.feature_importance(split=split) if split else m.feature_importance(nodes=q)
        exq = m.explain(q)
        want = np.zeros((C, ds["input_dim"]), np.float64)
        np.add.at(want, exq["classes"], np.abs(exq["features"].astype(np.float64)))    # rows in query order, as the kernel adds them
        cnt = np.bincount(exq["classes"], minlength=C)
        assert np.array_equal(count, cnt)
        want[cnt > 0] /= cnt[cnt > 0, None]
        assert same_bits(mean_abs, want)
        tiny = m.feature_importance(split=split, scratch_bytes=5 * ds["input_dim"] * 4) if split else m.feature_importance(nodes=q, scratch_bytes=5 * ds["input_dim"] * 4)
        assert same_bits(tiny[0], mean_abs) and np.array_equal(tiny[1], count)
    m.close()


def test_explain_every_node_matches_a_node_list():
    ds, m = make_model("sparse", "default")
    n = ds["num_nodes"]
    every, listed = m.explain(None), m.explain(np.arange(n))
    for key in every:
        assert same_bits(every[key], listed[key]), key
    assert every["nbr_ptr"][-1] == ds["g_indices"].size
    m.close()


def test_the_largest_feature_share_is_the_planted_column():
    """What it is for.  On the CPU oracle's weights the float64 reference ranks the planted column pred % feats first for 93.78 % of
    the 193 test nodes (chance: 1 / 32) and no query is open (REF_*).  Here: the reference on the model's own rows is above the
    midpoint between chance and that figure, fewer than 1 % of the queries are open, and explain()'s largest share is the
    reference's on every query that is not open."""
    from cuda_gcn_amd.model import HipGCNModel
    ds = planted()
    m = HipGCNModel(ds, seed=5, hidden_dim=16, dropout=0.0)
    m.run_epochs(PLANTED_EPOCHS, want_trace=False)
    ref = ModelReference(ds, m)
    test = np.flatnonzero(ds["split"] == 3).astype(np.int32)
    ex = m.explain(test)
    h1 = ref.hidden_rows(m)
    refs = []
    for i, v in enumerate(test):
        a, b = int(ex["nbr_ptr"][i]), int(ex["nbr_ptr"][i + 1])
        ids = ex["nbr_ids"][a:b].astype(np.int64)
        refs.append(R.explain64(np.array([0, b - a]), ids, ref.coef_of(v, ids), h1, ref.w2, 0, int(ex["classes"][i]), w1=ref.w1, s=ref.s, s_abs=ref.s_abs,
                                terms=ref.terms, row_lengths=np.diff(ref.indptr)))
    hit, opened, agree = R.top_feature_agreement(ex["features"], refs, ex["classes"] % ds["input_dim"])
    print(f"planted: largest feature share is the planted column for {hit:.4f} of {test.size} test nodes (reference on the model's rows); open {opened:.4f}")
    assert hit > (1 / ds["input_dim"] + REF_TOP_FEATURE) / 2, hit
    assert opened < 0.01, opened
    assert agree
    m.close()


@pytest.mark.parametrize("flags", ["0", "EVAL_LANE", "NO_GRAPH"])
def test_explanations_between_epochs_change_nothing(flags):
    """3 epochs, the queries, 2 more epochs: the bits of 5 epochs without them — traces, weights, test metrics, the last logits"""
    from cuda_gcn_amd import model as M
    f = getattr(M, flags) if flags != "0" else 0
    ds = datagen.make_dataset("cora-syn")
    a = M.HipGCNModel(ds, seed=6, flags=f, hidden_dim=16, dropout=0.5)
    b = M.HipGCNModel(ds, seed=6, flags=f, hidden_dim=16, dropout=0.5)
    ta, tb = [a.run_epochs(3)], [b.run_epochs(3)]
    before = b.predict(logp=True)
    b.explain([4, 4, 9])
    b.explain([1, 2, 3], classes=[0, 1, 2], features=False)
    b.feature_importance(nodes=[5, 6, 7, 8])
    after = b.predict(logp=True)
    assert all(same_bits(x, y) for x, y in zip(before, after))
    ta.append(a.run_epochs(1))
    tb.append(b.run_epochs(1))
    b.explain([0, 1])
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
    """a node id or class out of range, a split without rows, a hidden width above 256, more than 256 classes, bf16 tables, two
    logical ranks: GcnHostError naming the method, from
    the Python front end and from the C entry points called directly"""
    from cuda_gcn_amd import model as M
    from cuda_gcn_amd.model import HipGCNModel, GcnHostError, _ck
    from tests.mr_threads import ThreadWorld
    import ctypes as C
    ds = datagen.make_dataset("tiny-syn")
    n, nc = ds["num_nodes"], ds["output_dim"]
    m = HipGCNModel(ds, seed=1, hidden_dim=16)
    for call in (lambda: m.explain([0, n]), lambda: m.explain([-1]), lambda: m.feature_importance(nodes=[n])):
        with pytest.raises(GcnHostError, match="not a node of the dataset"):
            call()
    for call in (lambda: m.explain([0, 1], classes=[0, nc]), lambda: m.explain([0], classes=[-1])):
        with pytest.raises(GcnHostError, match="explain: classes holds a class the model does not have"):
            call()
    with pytest.raises(GcnHostError, match="explain: 1 classes for 2 nodes"):
        m.explain([0, 1], classes=[0])
    with pytest.raises(GcnHostError, match="feature_importance: split is 1"):
        m.feature_importance(split=4)
    # the C entry points
    ok, bad = np.array([0, 1], np.int32), np.array([0, n], np.int32)
    cls_bad = np.array([0, nc], np.int32)
    total = C.c_int64(0)
    oc, lg, hd = np.zeros(2, np.int32), np.zeros(2, np.float32), np.zeros((2, 16), np.float32)
    ptr, ids, vals = np.zeros(3, np.int64), np.zeros(4096, np.int32), np.zeros(4096, np.float32)

    def explain(nodes, classes=None, sizes_only=False):
        return m.lib.gcnhost_model_explain(m.h, nodes.ctypes.data, None if classes is None else classes.ctypes.data, 2, 0, oc.ctypes.data, lg.ctypes.data,
                                           hd.ctypes.data, None, ptr.ctypes.data, None if sizes_only else ids.ctypes.data, vals.ctypes.data, C.byref(total))
    with pytest.raises(GcnHostError, match=f"explain: node {n} is not a node of the dataset"):
        _ck(m.lib, explain(bad), "call")
    with pytest.raises(GcnHostError, match=f"explain: node {n} is not a node of the dataset"):
        _ck(m.lib, explain(bad, sizes_only=True), "call")
    with pytest.raises(GcnHostError, match=f"explain: class {nc} is not a class of the model"):
        _ck(m.lib, explain(ok, cls_bad), "call")
    _ck(m.lib, explain(ok, sizes_only=True), "call")
    assert total.value == int(np.diff(ds["g_indptr"])[:2].sum())
    ma, cnt = np.zeros((nc, ds["input_dim"]), np.float64), np.zeros(nc, np.int64)
    with pytest.raises(GcnHostError, match="feature_importance: invalid argument"):
        _ck(m.lib, m.lib.gcnhost_model_feature_importance(m.h, 7, None, 0, 0, ma.ctypes.data, cnt.ctypes.data), "call")
    m.close()
    # a split without rows
    empty = dict(ds, split=np.where(ds["split"] == 3, 0, ds["split"]).astype(np.int32))
    m = HipGCNModel(empty, seed=1, hidden_dim=16)
    with pytest.raises(GcnHostError, match="feature_importance: split 3 has no rows"):
        m.feature_importance(split=3)
    m.close()
    # a hidden width above 256, more than 256 classes: refused by the front end and by the C entry points, and nothing ran —
    # variable 3 keeps the bits of the training pass (an explanation's forward would store the evaluation's hidden layer)
    wide = HipGCNModel(ds, seed=1, hidden_dim=257, dropout=0.5)
    wide.train_epoch()
    before = wide.var(3)
    for what, call in (("explain", lambda: wide.explain([0])), ("feature_importance", lambda: wide.feature_importance())):
        with pytest.raises(GcnHostError, match=f"{what}: a hidden width of at most 256, this model has 257"):
            call()
    hd257 = np.zeros((2, 257), np.float32)
    with pytest.raises(GcnHostError, match="explain: a hidden width of at most 256"):
        _ck(wide.lib, wide.lib.gcnhost_model_explain(wide.h, ok.ctypes.data, None, 2, 0, oc.ctypes.data, lg.ctypes.data, hd257.ctypes.data, None,
                                                     ptr.ctypes.data, ids.ctypes.data, vals.ctypes.data, C.byref(total)), "call")
    with pytest.raises(GcnHostError, match="explain: a hidden width of at most 256"):
        _ck(wide.lib, wide.lib.gcnhost_model_explain(wide.h, ok.ctypes.data, None, 2, 0, None, None, None, None, None, None, None, C.byref(total)), "call")
    ma257 = np.zeros((nc, ds["input_dim"]), np.float64)
    with pytest.raises(GcnHostError, match="feature_importance: a hidden width of at most 256"):
        _ck(wide.lib, wide.lib.gcnhost_model_feature_importance(wide.h, 3, None, 0, 0, ma257.ctypes.data, cnt.ctypes.data), "call")
    assert same_bits(wide.var(3), before)
    wide.close()
    big = datagen.make_dataset("cora-syn")
    big = dict(big, output_dim=300, label=(np.arange(big["num_nodes"]) % 300).astype(np.int32))
    many = HipGCNModel(big, seed=1, hidden_dim=16, dropout=0.5)      # untrained: the single-label loss itself stops at 256 classes
    before = many.var(3)
    with pytest.raises(GcnHostError, match="feature_importance: at most 256 classes, this model has 300"):
        many.feature_importance()
    ma300, cnt300 = np.zeros((300, big["input_dim"]), np.float64), np.zeros(300, np.int64)
    with pytest.raises(GcnHostError, match=r"feature_importance: at most 256 classes \(a thread keeps"):
        _ck(many.lib, many.lib.gcnhost_model_feature_importance(many.h, 3, None, 0, 0, ma300.ctypes.data, cnt300.ctypes.data), "call")
    assert same_bits(many.var(3), before)
    many.close()
    # bf16 tables
    m = HipGCNModel(ds, seed=1, hidden_dim=16, flags=M.BF16_TABLES)
    for what, call in (("explain", lambda: m.explain([0])), ("feature_importance", lambda: m.feature_importance())):
        with pytest.raises(GcnHostError, match=f"{what}: not with bf16 tables"):
            call()
    m.close()
    # two logical ranks: refused on each
    tw = ThreadWorld(2)
    seen, errors = [None, None], []

    def body(rank):
        try:
            ag, ar = tw.callbacks(rank)
            r = HipGCNModel(ds, seed=4, device=0, rank=rank, world=2, host_allgather=ag, host_allreduce=ar, hidden_dim=16, dropout=0.5)
            msgs = []
            for call in (lambda: r.explain([0]), lambda: r.feature_importance()):
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
        assert "explain: one rank only" in msgs[0] and "feature_importance: one rank only" in msgs[1], msgs


# ---- the command line -----------------------------------------------------------------------------------------------------

def test_cli_explain(tmp_path):
    """gcn-hip on the text files datagen.write_text makes, with GCN_EXPLAIN: stdout keeps its lines; the file's lines are the
    Python explain() / feature_importance() of the same weights (handed over through a weights file, 0 epochs), the five largest
    shares first with ties by ascending id or column; refused on two GPUs"""
    import os
    import subprocess
    from cuda_gcn_amd.model import HipGCNModel
    hip = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cuda_gcn_amd", "bin", "gcn-hip")
    ds = datagen.make_dataset("tiny-syn")
    datagen.write_text(ds, str(tmp_path / "data"), "tiny-syn")
    m = HipGCNModel(ds, seed=3, hidden_dim=16, dropout=0.5)
    m.run_epochs(6, want_trace=False)
    w = str(tmp_path / "w.gcnw")
    m.save_weights(w)
    test = np.flatnonzero(ds["split"] == 3).astype(np.int32)
    ex = m.explain(test)
    mean_abs, count = m.feature_importance(split=3)
    m.close()
    args = ["tiny-syn", "-", "-", "16", "-", "0.5", "-", "-", "0"]
    out = str(tmp_path / "x.txt")
    env = dict(os.environ, GCN_SEED="3", GCN_LOAD_WEIGHTS=w, GCN_EXPLAIN=out)
    r = subprocess.run(["timeout", "-k", "10", "50", hip] + args, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1].startswith("test_loss=")
    lines = open(out).read().strip().splitlines()
    assert len(lines) == test.size + ds["output_dim"]

    def top(values, labels, k):
        order = np.lexsort((labels, -values.astype(np.float64)))[:k]
        return [(int(labels[j]), values[j]) for j in order]

    def pairs(text, dtype):
        return [(int(p.split(":")[0]), dtype(p.split(":")[1])) for p in text.split()]
    cols = np.arange(ds["input_dim"])
    for i, line in enumerate(lines[:test.size]):
        head, nbr, feat = [part.strip() for part in line.split("|")]
        node, cls, logit = head.split()
        assert int(node) == test[i] and int(cls) == ex["classes"][i] and np.float32(logit) == ex["logit"][i]
        a, b = int(ex["nbr_ptr"][i]), int(ex["nbr_ptr"][i + 1])
        assert pairs(nbr, np.float32) == top(ex["nbr_values"][a:b], ex["nbr_ids"][a:b], 5), i
        assert pairs(feat, np.float32) == top(ex["features"][i], cols, 5), i
    for c, line in enumerate(lines[test.size:]):
        head, feat = [part.strip() for part in line.split("|")]
        assert head == f"class {c} nodes={count[c]}"
        got, want = pairs(feat, np.float64), top(mean_abs[c], cols, 10)
        assert [g[0] for g in got] == [x[0] for x in want] and np.allclose([g[1] for g in got], [x[1] for x in want], rtol=1e-8, atol=0)
    bad = subprocess.run(["timeout", "-k", "10", "50", hip] + args, cwd=str(tmp_path), env=dict(env, GCN_GPUS="2"), capture_output=True, text=True)
    assert bad.returncode != 0 and "GCN_EXPLAIN runs on one GPU" in bad.stderr, bad.stderr[-500:]
