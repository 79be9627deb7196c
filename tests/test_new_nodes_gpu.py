"""Unseen nodes on the GPU (HipGCNModel.predict_new_nodes, ModelQueries::predict_new): new rows attached to a trained graph,
against the reference's CPU forward on the augmented dataset, against a second model built on the augmented dataset, at a
temperature, on a multi-label model, between epochs, refused inputs, and the command line (GCN_NEW_NODES, GCN_NEW_PREDICT)."""
import faulthandler
import os
import signal
import subprocess

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests.test_predict_gpu import cpu_eval_logits, log_softmax, clear_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")
TEST_LIMIT_S = 120
M_ALL = 300
SIZES = (1, 65, 300)
HUB_LIST = 3000


@pytest.fixture(autouse=True)
def _time_limit():
    """every test of this file ends within TEST_LIMIT_S (test_predict_gpu.py's scheme)"""
    def expire(signum, frame):
        raise TimeoutError(f"test exceeded {TEST_LIMIT_S} s")
    old = signal.signal(signal.SIGALRM, expire)
    signal.alarm(TEST_LIMIT_S)
    faulthandler.dump_traceback_later(TEST_LIMIT_S + 30, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def new_nodes(ds, seed=11):
    """M_ALL new nodes for a dataset: features = scaled copies of dataset rows (CSR), lists of 0-7 ids.  The rows are built so
    that every prefix of 1, 65 or 300 of them is a call of its own — row i of a prefix of m lists ids in [0, N + m) only — and,
    since new rows influence nobody else and a new neighbour's length does not depend on the call, gives the logits those rows
    have in the full batch: one reference serves the three sizes.  Row 0 lists HUB_LIST dataset ids (repeats among them) and
    itself again; rows 1 .. 64 link to each other, also to later ones; some rows list nothing."""
    rng = np.random.default_rng(seed)
    N = ds["num_nodes"]
    fp, fi, fv = ds["f_indptr"].astype(np.int64), ds["f_indices"], ds["f_val"]
    src = rng.integers(0, N, M_ALL)
    scale = rng.uniform(0.5, 1.5, M_ALL).astype(np.float32)
    x_ptr = np.concatenate([[0], np.cumsum(fp[src + 1] - fp[src])]).astype(np.int32)
    x_idx = np.concatenate([fi[fp[s]:fp[s + 1]] for s in src]).astype(np.int32)
    x_val = np.concatenate([fv[fp[s]:fp[s + 1]] * scale[i] for i, s in enumerate(src)]).astype(np.float32)
    lists = []
    for i in range(M_ALL):
        limit = N + (1 if i < 1 else 65 if i < 65 else M_ALL)
        if i == 0:
            lists.append(np.concatenate([rng.integers(0, N, HUB_LIST - 1), [N]]))
        else:
            k = int(rng.integers(0, 8))
            ids = rng.integers(0, limit, k)
            if k >= 2:
                ids[0] = rng.integers(N, limit)                # a link to a new node: itself, an earlier or a later one
            lists.append(ids)
    nbr_ptr = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    nbr_ids = np.concatenate(lists).astype(np.int32)
    return dict(x=(x_ptr, x_idx, x_val), nbr_ptr=nbr_ptr, nbr_ids=nbr_ids)


def prefix(nn, m, F=None):
    """the first m new nodes as a call: (features, nbr_ptr, nbr_ids); F: the features as a dense [m, F] array"""
    x_ptr, x_idx, x_val = nn["x"]
    feats = (x_ptr[:m + 1], x_idx[:x_ptr[m]], x_val[:x_ptr[m]])
    if F is not None:
        dense = np.zeros((m, F), np.float32)
        rows = np.repeat(np.arange(m), np.diff(feats[0]))
        dense[rows, feats[1]] = feats[2]
        feats = dense
    return feats, nn["nbr_ptr"][:m + 1], nn["nbr_ids"][:nn["nbr_ptr"][m]]


def augmented(ds, nn, multilabel=None):
    """the dataset with the new rows appended: self loop first, then the listed ids; nobody lists them back"""
    N, m = ds["num_nodes"], M_ALL
    x_ptr, x_idx, x_val = nn["x"]
    rows = [np.concatenate([[N + i], nn["nbr_ids"][nn["nbr_ptr"][i]:nn["nbr_ptr"][i + 1]]]) for i in range(m)]
    out = dict(ds)
    out["num_nodes"] = N + m
    out["g_indptr"] = np.concatenate([ds["g_indptr"], ds["g_indptr"][-1] + np.cumsum([len(r) for r in rows])]).astype(np.int32)
    out["g_indices"] = np.concatenate([ds["g_indices"]] + rows).astype(np.int32)
    out["f_indptr"] = np.concatenate([ds["f_indptr"], ds["f_indptr"][-1] + x_ptr[1:]]).astype(np.int32)
    out["f_indices"] = np.concatenate([ds["f_indices"], x_idx]).astype(np.int32)
    out["f_val"] = np.concatenate([ds["f_val"], x_val]).astype(np.float32)
    out["split"] = np.concatenate([ds["split"], np.zeros(m, np.int32)])           # in no split
    if ds.get("label") is not None:
        out["label"] = np.concatenate([ds["label"], np.zeros(m, np.int32)])
    if multilabel is not None:
        out["multilabel"] = np.concatenate([multilabel, np.zeros((m, multilabel.shape[1]), multilabel.dtype)])
    return out


_CASES = {}


@pytest.fixture(scope="module")
def cases(oracle):
    """(dataset, flags) -> the trained model, its new nodes, the reference's logits of the augmented dataset: made once"""
    from cuda_gcn_amd import model as M

    def get(name, flags):
        key = (name, flags)
        if key not in _CASES:
            hidden = 16 if name == "cora-syn" else 128
            ds = datagen.make_dataset(name)
            mdl = M.HipGCNModel(ds, seed=3, flags=getattr(M, flags) if flags != "0" else 0, hidden_dim=hidden, dropout=0.5)
            for _ in range(10 if name == "cora-syn" else 3):
                mdl.train_epoch()
            nn = new_nodes(ds)
            aug = augmented(ds, nn)
            z = cpu_eval_logits(oracle, aug, mdl.var(2), mdl.var(5)).reshape(aug["num_nodes"], -1)
            _CASES[key] = dict(ds=ds, model=mdl, nn=nn, aug=aug, z=z, dense=name != "cora-syn")
        return _CASES[key]
    yield get
    for c in _CASES.values():
        c["model"].close()
    _CASES.clear()


MODELS = [("cora-syn", "0"), ("cora-syn", "EDGE_COEF"), ("reddit-mini", "0"), ("reddit-mini", "EDGE_COEF")]


@pytest.mark.parametrize("name,flags", MODELS)
@pytest.mark.parametrize("m", SIZES)
def test_new_nodes_match_the_reference_forward_on_the_augmented_dataset(cases, name, flags, m):
    c = cases(name, flags)
    N, F = c["ds"]["num_nodes"], c["ds"]["input_dim"]
    z = c["z"]
    tol = 1e-4 * max(1.0, float(np.abs(z).max()))
    zn = z[N:N + m]
    ok = clear_rows(zn, tol)
    assert ok.mean() >= 0.9, ok.mean()                     # a condition on the reference alone
    feats, nbr_ptr, nbr_ids = prefix(c["nn"], m, F if c["dense"] else None)       # dense X: an [m, F] array; sparse X: the CSR triple
    pred, prob, logp = c["model"].predict_new_nodes(feats, nbr_ptr, nbr_ids, logp=True)
    assert pred.shape == (m,) and pred.dtype == np.int32 and prob.shape == (m,) and logp.shape == (m, z.shape[1])
    lz = log_softmax(zn)
    err = float(np.abs(logp - lz).max())
    print(f"{name} {flags} m {m}: max |logp - reference| {err:.3e} (tolerance {tol:.3e}), clear rows {ok.mean():.3f}")
    assert np.allclose(logp, lz, rtol=0, atol=tol)
    assert np.allclose(prob, np.exp(lz.max(axis=1)), rtol=0, atol=1e-5)
    assert np.array_equal(pred[ok], np.argmax(zn, axis=1)[ok])
    # without logp: the same predictions, bit for bit; the other form of the features: the same bits too
    p2, q2 = c["model"].predict_new_nodes(feats, nbr_ptr, nbr_ids)
    assert np.array_equal(p2, pred) and np.array_equal(q2.view(np.uint32), prob.view(np.uint32))
    if not c["dense"]:
        dense, _, _ = prefix(c["nn"], m, F)
        p3, q3, l3 = c["model"].predict_new_nodes(dense, nbr_ptr, nbr_ids, logp=True)
        print(f"    dense form of the same features: max |logp - reference| {float(np.abs(l3 - lz).max()):.3e}")
        assert np.allclose(l3, lz, rtol=0, atol=tol) and np.array_equal(p3[ok], pred[ok])


@pytest.mark.parametrize("name,flags", MODELS)
def test_new_nodes_match_a_model_built_on_the_augmented_dataset(cases, name, flags):
    from cuda_gcn_amd import model as M
    c = cases(name, flags)
    N = c["ds"]["num_nodes"]
    first = c["model"]
    second = M.HipGCNModel(c["aug"], seed=9, flags=getattr(M, flags) if flags != "0" else 0, hidden_dim=first.params.hidden_dim, dropout=0.5)
    second.set_weights(first.var(2), first.var(5))
    tol = 1e-4 * max(1.0, float(np.abs(c["z"]).max()))
    q = np.arange(N, N + M_ALL, dtype=np.int32)
    pred2, prob2, logp2 = second.predict(nodes=q, logp=True)
    for m in SIZES:
        feats, nbr_ptr, nbr_ids = prefix(c["nn"], m)
        pred, prob, logp = first.predict_new_nodes(feats, nbr_ptr, nbr_ids, logp=True)
        ok = clear_rows(logp2[:m], tol)
        assert np.allclose(logp, logp2[:m], rtol=0, atol=tol) and np.allclose(prob, prob2[:m], rtol=0, atol=1e-5)
        assert np.array_equal(pred[ok], pred2[:m][ok])
    # the new rows influence no dataset node: the second model's rows below N are the first model's
    old = np.arange(0, N, 3, dtype=np.int32)
    pa, qa, la = first.predict(nodes=old, logp=True)
    pb, qb, lb = second.predict(nodes=old, logp=True)
    ok = clear_rows(la, tol)
    assert np.allclose(la, lb, rtol=0, atol=tol) and np.allclose(qa, qb, rtol=0, atol=1e-5) and np.array_equal(pa[ok], pb[ok])
    second.close()


def test_temperature(cases):
    c = cases("cora-syn", "0")
    N, mdl = c["ds"]["num_nodes"], c["model"]
    feats, nbr_ptr, nbr_ids = prefix(c["nn"], 65)
    pred1, _ = mdl.predict_new_nodes(feats, nbr_ptr, nbr_ids)
    mdl.set_temperature(2.0)
    try:
        pred, prob, logp = mdl.predict_new_nodes(feats, nbr_ptr, nbr_ids, logp=True)
    finally:
        mdl.set_temperature(1.0)
    zn = c["z"][N:N + 65]
    tol = 1e-4 * max(1.0, float(np.abs(c["z"]).max()))
    lz = log_softmax(zn / 2.0)
    assert np.allclose(logp, lz, rtol=0, atol=tol) and np.allclose(prob, np.exp(lz.max(axis=1)), rtol=0, atol=1e-5)
    assert np.array_equal(pred, pred1)


def test_multilabel_sets_and_thresholds(oracle):
    """70 classes: the class gather takes more than 64 columns and stores the logits; gcnhip_bce_predict_rows decides"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.planted_multilabel(classes=70)
    N, C = ds["num_nodes"], 70
    mdl = HipGCNModel(ds, seed=5, hidden_dim=16, dropout=0.5, multilabel=ds["multilabel"])
    for _ in range(5):
        mdl.train_epoch()
    nn = new_nodes(ds, seed=12)
    aug = augmented(ds, nn, ds["multilabel"])
    aug["output_dim"] = C
    z = cpu_eval_logits(oracle, aug, mdl.var(2), mdl.var(5)).reshape(N + M_ALL, -1)
    tol = 1e-4 * max(1.0, float(np.abs(z).max()))
    thr = np.random.default_rng(0).uniform(-0.5, 0.5, C).astype(np.float32)
    for m in SIZES:
        feats, nbr_ptr, nbr_ids = prefix(nn, m)
        zn = z[N:N + m]
        sets, prob = mdl.predict_new_nodes(feats, nbr_ptr, nbr_ids, prob=True)
        assert sets.shape == (m, C) and sets.dtype == bool and prob.shape == (m, C)
        sure = np.abs(zn) > tol
        assert sure.mean() > 0.9
        assert np.array_equal(sets[sure], (zn > 0)[sure])
        assert np.allclose(prob, 1.0 / (1.0 + np.exp(-zn)), rtol=0, atol=tol)       # |d sigmoid / dz| <= 1/4
        cut = mdl.predict_new_nodes(feats, nbr_ptr, nbr_ids, thresholds=thr)
        sure = np.abs(zn - thr[None, :]) > tol
        assert np.array_equal(cut[sure], (zn >= thr[None, :])[sure])
    e = mdl.predict_new_nodes(np.zeros((0, ds["input_dim"]), np.float32), [0], [])
    assert e.shape == (0, C)
    with pytest.raises(ValueError, match="69 thresholds for 70 classes"):
        mdl.predict_new_nodes(*prefix(nn, 1), thresholds=thr[:-1])
    mdl.close()


@pytest.mark.parametrize("flags", ["0", "EVAL_LANE", "NO_GRAPH", "MODULAR", "EDGE_COEF"])
def test_predict_new_nodes_between_epochs_changes_nothing(flags):
    """test_predict_between_epochs_changes_nothing's scheme: two models with the same seed train in lockstep, one calling
    predict_new_nodes between epochs: traces, weights and test metrics are bit-identical; the same call twice gives the same bits"""
    from cuda_gcn_amd import model as M
    f = getattr(M, flags) if flags != "0" else 0
    ds = datagen.make_dataset("cora-syn")
    a = M.HipGCNModel(ds, seed=6, flags=f, hidden_dim=16, dropout=0.5)
    b = M.HipGCNModel(ds, seed=6, flags=f, hidden_dim=16, dropout=0.5)
    nn = new_nodes(ds)
    big, small = prefix(nn, 300), prefix(nn, 1)
    ta, tb = [], []
    for e in range(4):
        ta.append(a.run_epochs(1))
        tb.append(b.run_epochs(1))
        r1 = b.predict_new_nodes(*big, logp=True)
        b.predict_new_nodes(*small)
        r2 = b.predict_new_nodes(*big, logp=True)
        for x, y in zip(r1, r2):
            assert x.tobytes() == y.tobytes()
    ta.append(np.array([a.train_epoch() + a.eval(2)], np.float32))
    tb.append(np.array([b.train_epoch() + b.eval(2)], np.float32))
    ta, tb = np.concatenate(ta), np.concatenate(tb)
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32)), (ta, tb)
    for k in (2, 5):
        assert np.array_equal(a.var(k).view(np.uint32), b.var(k).view(np.uint32)), k
    assert a.eval(3) == b.eval(3)
    assert np.array_equal(a.var(6).view(np.uint32), b.var(6).view(np.uint32))     # the logits of the last forward
    a.close()
    b.close()


def test_refusals_leave_the_model_answering(cases):
    from cuda_gcn_amd import model as M
    c = cases("cora-syn", "0")
    mdl, N, F = c["model"], c["ds"]["num_nodes"], c["ds"]["input_dim"]
    m = 65                                                 # (a prefix of new_nodes' rows is a call of its own at 1, 65 and 300)
    feats, nbr_ptr, nbr_ids = prefix(c["nn"], m)
    before = mdl.predict()
    bad_ids = nbr_ids.copy()
    bad_ids[-1] = N + m
    with pytest.raises(M.GcnHostError, match=rf"id {N + m} is outside \[0, {N + m}\)"):
        mdl.predict_new_nodes(feats, nbr_ptr, bad_ids)
    with pytest.raises(ValueError, match=rf"the model takes \[m, {F}\]"):
        mdl.predict_new_nodes(np.zeros((m, F + 1), np.float32), nbr_ptr, nbr_ids)
    wide = (feats[0], feats[1].copy(), feats[2])
    wide[1][0] = F
    with pytest.raises(M.GcnHostError, match=rf"feature column {F} is outside the model's input width {F}"):
        mdl.predict_new_nodes(wide, nbr_ptr, nbr_ids)
    with pytest.raises(M.GcnHostError, match="single-label model"):
        mdl.predict_new_nodes(feats, nbr_ptr, nbr_ids, thresholds=np.zeros(c["ds"]["output_dim"], np.float32))
    down = nbr_ptr.copy()
    down[1] = down[2] + 1                                  # row 0 lists 3 000 ids, row 1 fewer than 8: the pointer steps back
    with pytest.raises(M.GcnHostError, match="nbr_ptr decreases at new node 1"):
        mdl.predict_new_nodes(feats, down, nbr_ids)
    e = mdl.predict_new_nodes(np.zeros((0, F), np.float32), [0], [])
    assert e[0].shape == (0,) and e[1].shape == (0,)
    after = mdl.predict()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
    bf = M.HipGCNModel(c["ds"], seed=3, flags=M.BF16_TABLES, hidden_dim=16, dropout=0.5)
    with pytest.raises(M.GcnHostError, match="not with bf16 tables"):
        bf.predict_new_nodes(feats, nbr_ptr, nbr_ids)
    assert bf.predict()[0].shape == (N,)
    bf.close()


def test_cli_new_nodes(cases, tmp_path):
    """gcn-hip cora-syn with GCN_LOAD_WEIGHTS and 0 epochs, GCN_NEW_NODES=<stem> and GCN_NEW_PREDICT=<file>: the file's classes
    are the Python call's, its node ids N + i"""
    c = cases("cora-syn", "0")
    ds, mdl, N = c["ds"], c["model"], c["ds"]["num_nodes"]
    m = 65
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "cora-syn.gcnbin"))
    w, out, stem = str(tmp_path / "w.gcnw"), str(tmp_path / "new.txt"), str(tmp_path / "incoming")
    mdl.save_weights(w)
    feats, nbr_ptr, nbr_ids = prefix(c["nn"], m)
    with open(stem + ".graph", "w") as f:
        for i in range(m):
            f.write(" ".join(map(str, nbr_ids[nbr_ptr[i]:nbr_ptr[i + 1]].tolist())) + "\n")
    with open(stem + ".svmlight", "w") as f:
        for i in range(m):
            toks = ["%d:%.9g" % (k, v) for k, v in zip(feats[1][feats[0][i]:feats[0][i + 1]].tolist(), feats[2][feats[0][i]:feats[0][i + 1]].tolist())]
            f.write("0" + (" " if toks else "") + " ".join(toks) + "\n")           # the label column is read and ignored
    r = subprocess.run(["timeout", "-k", "10", "50", HIP, "cora-syn", "-", "-", "16", "-", "0.5", "-", "-", "0"], cwd=str(tmp_path),
                       env=dict(os.environ, GCN_SEED="3", GCN_LOAD_WEIGHTS=w, GCN_NEW_NODES=stem, GCN_NEW_PREDICT=out), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert f"predictions of {m} new nodes" in r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1].startswith("test_loss=")                                       # stdout is unchanged
    rows = np.loadtxt(out, ndmin=2)
    pred, prob, logp = mdl.predict_new_nodes(feats, nbr_ptr, nbr_ids, logp=True)
    assert rows.shape == (m, 3) and np.array_equal(rows[:, 0], np.arange(N, N + m))
    # the program's model is another object (its own lanes and schedule): classes on the rows that no last bit decides
    ok = clear_rows(logp, 1e-4 * max(1.0, float(np.abs(c["z"]).max())))
    assert ok.mean() >= 0.9 and np.array_equal(rows[ok, 1].astype(np.int64), pred[ok])
    assert np.allclose(rows[:, 2], prob, rtol=0, atol=1e-5)                         # (printed with %.6g)
    # only one of the two variables: refused before the GPU is touched
    r = subprocess.run(["timeout", "-k", "10", "50", HIP, "cora-syn", "-", "-", "16", "-", "0.5", "-", "-", "0"], cwd=str(tmp_path),
                       env=dict(os.environ, GCN_NEW_NODES=stem), capture_output=True, text=True)
    assert r.returncode != 0 and "go together" in r.stderr
