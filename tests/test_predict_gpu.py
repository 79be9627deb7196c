"""Prediction (gcnhip_graphsum_predict, HipGCN::predict) and the weights file on the GPU: the prediction epilogue against the
stored logits of the existing aggregation, the model's predictions against a CPU forward (oracle) from its own weights,
node queries, no side effects on training, save / load, several ranks, and the command line (GCN_SAVE_WEIGHTS,
GCN_LOAD_WEIGHTS, GCN_PREDICT)."""
import faulthandler
import os
import signal
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from cuda_gcn_amd import datagen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")
TEST_LIMIT_S = 120


@pytest.fixture(autouse=True)
def _time_limit():
    """every test of this file ends within TEST_LIMIT_S: an alarm fails it; if the process is stuck inside a call that never
    returns, faulthandler prints the stacks and ends the process shortly after"""
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


def bf16_round(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def log_softmax(z):
    z = np.asarray(z, np.float64)
    s = z - z.max(axis=1, keepdims=True)
    return s - np.log(np.exp(s).sum(axis=1, keepdims=True))


def clear_rows(z, tol):
    """rows whose largest logit leads the second by more than tol (argmax is decided whatever the rounding)"""
    t = np.sort(np.asarray(z, np.float64), axis=1)
    return t[:, -1] - t[:, -2] > tol


# ---- the kernel entry point ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,dim", [("cora-syn", 7), ("reddit-mini", 41), ("reddit-mini", 64), ("tiny-syn", 3), ("cora-syn", 1)])
def test_predict_epilogue_matches_stored_logits(name, dim):
    """gcnhip_graphsum_predict against gcnhip_graphsum_ex / gcnhip_graphsum_bf16 on the same operands: the logits are
    bit-identical (f32 per-edge, factored, bf16 table; all rows and a row subset; split rows take the finalize kernel), pred
    is numpy.argmax of them, prob = 1 / sum(exp(z - max)), logp the log-softmax"""
    from cuda_gcn_amd.ops import Device
    ds = datagen.make_dataset(name)
    dev = Device(0)
    gp, gi = ds["g_indptr"], ds["g_indices"]
    N = ds["num_nodes"]
    g = dev.graph(gp, gi)
    x = np.random.default_rng(dim).standard_normal((N, dim)).astype(np.float32) * 3
    subset = np.random.default_rng(1).random(N) < 0.3
    rs = g.add_rowset(subset)
    t = dev.to_bf16(x)
    cases = [
        ("per-edge", dict(x=x, scaling=0), lambda rows: dev.graphsum_ex(g, x, 0, rows=rows)),
        ("factored", dict(x=x, scaling=1), lambda rows: dev.graphsum_ex(g, x, 1, rows=rows)),
        ("bf16", dict(table_bf16=t, dim=dim), lambda rows: dev.graphsum_bf16(g, t, dim, ld_out=(dim + 3) // 4 * 4, out_rows=rows)),
    ]
    for label, kw, ref in cases:
        for rows, mask in ((None, np.ones(N, bool)), (rs, subset)):
            want = ref(rows)
            got = dev.graphsum_predict(g, rows=rows, **kw)
            assert np.array_equal(got["logits"][mask].view(np.uint32), want[mask].view(np.uint32)), label
            assert np.all(np.isnan(got["logits"][~mask])) and np.all(got["pred"][~mask] == -1), label       # untouched
            z = want[mask]
            assert np.array_equal(got["pred"][mask], np.argmax(z, axis=1)), label
            se = np.exp(z.astype(np.float64) - z.max(axis=1, keepdims=True)).sum(axis=1)
            assert np.allclose(got["prob"][mask], 1.0 / se, rtol=2e-6, atol=0), label
            assert np.allclose(got["logp"][mask], log_softmax(z), rtol=0, atol=2e-5 * max(1.0, float(np.abs(z).max()))), label
            # without the logits stored and without logp: the same predictions, bit for bit
            lean = dev.graphsum_predict(g, rows=rows, logp=False, store_logits=False, **kw)
            assert np.array_equal(lean["pred"], got["pred"]) and np.array_equal(lean["prob"].view(np.uint32), got["prob"].view(np.uint32))
    # every logit row constant: each row is one tie of all classes, and the lowest class wins (numpy.argmax's rule)
    tie = dev.graphsum_predict(g, x=np.ones((N, dim), np.float32), scaling=1)
    assert np.all(tie["pred"] == 0)
    assert np.allclose(tie["prob"], 1.0 / dim, rtol=1e-6)
    g.remove_rowset(rs)
    with pytest.raises(Exception):
        dev.graphsum_predict(g, x=np.zeros((N, 65), np.float32))        # more than 64 classes: an error, not a wrong answer


# ---- the model ----------------------------------------------------------------------------------------------------------

def cpu_eval_logits(oracle, ds, w1, w2):
    """the reference's evaluation forward (gcn.cpp:120-128, no dropout) on the CPU from the model's own weights"""
    N, F = ds["num_nodes"], ds["input_dim"]
    h, C = w2.shape
    gp, gi = ds["g_indptr"], ds["g_indices"]
    if ds.get("f_indices") is not None:
        h0 = oracle.spmm_fwd(ds["f_indptr"], ds["f_indices"], ds["f_val"], w1, h)
    else:
        h0 = oracle.matmul_fwd(ds["f_val"].reshape(N, F), w1, N, F, h)
    h1 = oracle.graphsum(gp, gi, h0, h)
    h1, _ = oracle.relu_fwd(h1, training=False)
    z0 = oracle.matmul_fwd(h1.reshape(N, h), w2, N, h, C)
    return oracle.graphsum(gp, gi, z0, C)


@pytest.mark.parametrize("name,hidden,flags", [
    ("cora-syn", 16, 0), ("cora-syn", 16, "EDGE_COEF"), ("cora-syn", 16, "BF16_TABLES"), ("cora-syn", 16, "ALL_ROWS"),
    ("reddit-mini", 128, 0), ("reddit-mini", 128, "EDGE_COEF"), ("reddit-mini", 128, "BF16_TABLES"), ("reddit-mini", 128, "ALL_ROWS|BF16_TABLES"),
])
def test_predict_matches_oracle_forward(oracle, name, hidden, flags):
    from cuda_gcn_amd import model as M
    f = 0
    for k in str(flags).split("|"):
        f |= getattr(M, k) if k != "0" else 0
    ds = datagen.make_dataset(name)
    m = M.HipGCNModel(ds, seed=3, flags=f, hidden_dim=hidden, dropout=0.5)
    for _ in range(10 if name == "cora-syn" else 3):
        m.train_epoch()
    pred, prob, logp = m.predict(logp=True)
    assert pred.shape == (ds["num_nodes"],) and pred.dtype == np.int32
    if f & M.BF16_TABLES:
        # the logit aggregation gathers the bf16-rounded Z0 of this forward (variable 4: stored, not factored in this format)
        z = oracle.graphsum(ds["g_indptr"], ds["g_indices"], bf16_round(m.var(4)), ds["output_dim"]).reshape(ds["num_nodes"], -1)
        tol = 2e-5 * max(1.0, float(np.abs(z).max()))
    else:
        z = cpu_eval_logits(oracle, ds, m.var(2), m.var(5)).reshape(ds["num_nodes"], -1)
        tol = 1e-4 * max(1.0, float(np.abs(z).max()))        # (aggregate-first evaluation: reassociated f32 sums)
    ok = clear_rows(z, tol)
    assert ok.mean() > 0.9, ok.mean()
    assert np.array_equal(pred[ok], np.argmax(z, axis=1)[ok])
    lz = log_softmax(z)
    assert np.allclose(prob[ok], np.exp(lz.max(axis=1))[ok], rtol=0, atol=1e-5)
    assert np.allclose(logp, lz, rtol=0, atol=tol)
    # split 3: the share of nodes whose prediction is the label is eval(3)'s printed accuracy (the reference counts a tie with
    # the true class as correct; numpy.argmax takes the lowest class: the two agree when there is no exact tie — assert that)
    test = ds["split"] == 3
    _, acc = m.eval(3)
    top = np.sort(m.var(6)[test], axis=1)                 # eval(3) computed these rows
    assert not np.any(top[:, -1] == top[:, -2]), "exact tie in the logits"
    assert abs(float(np.mean(pred[test] == ds["label"][test])) - acc) <= 1e-6
    m.close()


def test_query_subsets_equal_the_full_prediction():
    """predict(nodes=q) for shuffled queries of 1, 63, 64, 65 and 1000 nodes (and repeated ids) = the matching entries of
    predict(), bit for bit; the same query twice reuses its row subset; bad ids are errors"""
    from cuda_gcn_amd.model import HipGCNModel, GcnHostError
    ds = datagen.make_dataset("reddit-mini")
    m = HipGCNModel(ds, seed=2, hidden_dim=128, dropout=0.5)
    m.train_epoch()
    pred, prob, logp = m.predict(logp=True)
    rng = np.random.default_rng(0)
    N = ds["num_nodes"]
    for n in (1, 63, 64, 65, 1000):
        q = rng.permutation(N)[:n].astype(np.int32)
        for qq in (q, np.concatenate([q, q[::-1], q[:1]])):
            a, b, c = m.predict(nodes=qq, logp=True)
            assert np.array_equal(a, pred[qq]) and np.array_equal(b.view(np.uint32), prob[qq].view(np.uint32))
            assert np.array_equal(c.view(np.uint32), logp[qq].view(np.uint32))
    # the hub rows (split into segments: the finalize kernel) are in a query of their own
    hubs = np.argsort(np.diff(ds["g_indptr"]))[-65:].astype(np.int32)
    a, b = m.predict(nodes=hubs)
    assert np.array_equal(a, pred[hubs]) and np.array_equal(b.view(np.uint32), prob[hubs].view(np.uint32))
    a, b = m.predict(nodes=np.zeros(0, np.int32))
    assert a.size == 0 and b.size == 0
    for bad in ([-1], [N], [0, N + 5]):
        with pytest.raises(GcnHostError):
            m.predict(nodes=bad)
    m.close()


@pytest.mark.parametrize("flags", ["0", "EVAL_LANE", "NO_GRAPH", "BF16_TABLES", "MODULAR"])
def test_predict_between_epochs_changes_nothing(flags):
    """two models with the same seed train in lockstep, one calling predict() between epochs: their run_epochs traces, weights
    and test metrics are bit-identical (captured epoch replay by default; the validation lane; eager epochs)"""
    from cuda_gcn_amd import model as M
    f = getattr(M, flags) if flags != "0" else 0
    ds = datagen.make_dataset("cora-syn")
    a = M.HipGCNModel(ds, seed=6, flags=f, hidden_dim=16, dropout=0.5)
    b = M.HipGCNModel(ds, seed=6, flags=f, hidden_dim=16, dropout=0.5)
    ta, tb = [], []
    q = np.arange(0, ds["num_nodes"], 7, dtype=np.int32)
    for e in range(4):
        ta.append(a.run_epochs(1))
        tb.append(b.run_epochs(1))
        b.predict()
        b.predict(nodes=q, logp=True)
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


def same_result(x, y):
    """results of one query on two models: integer and bool arrays equal, float arrays equal bit for bit, the rest =="""
    if isinstance(x, dict):
        return x.keys() == y.keys() and all(same_result(x[k], y[k]) for k in x)
    if isinstance(x, tuple):
        return len(x) == len(y) and all(same_result(p, q) for p, q in zip(x, y))
    if isinstance(x, np.ndarray):
        return x.dtype == y.dtype and x.shape == y.shape and np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()
    return x == y or (x != x and y != y)                 # (a metric of an empty class may be NaN)


def check_any_order(a, b, steps):
    """model a runs the queries top to bottom, model b (the same weights) bottom to top: scratch that an earlier, larger or
    smaller query sized must not show in any result"""
    ra = [call(a) for _, call in steps]
    rb = [call(b) for _, call in reversed(steps)][::-1]
    for (name, _), x, y in zip(steps, ra, rb):
        assert same_result(x, y), name
    return ra, rb


def test_queries_in_any_order_single_label():
    """the twelve single-label queries — node queries of 3, 5, 1000 and 1500 ids, splits, 64- and 3-wide propagation, Correct &
    Smooth, a fit — give the same bits whichever way round they run; the first and the last (the same 3 ids) agree too"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.make_dataset("cora-syn")
    N = ds["num_nodes"]
    a = HipGCNModel(ds, seed=6, hidden_dim=16, dropout=0.5)
    b = HipGCNModel(ds, seed=6, hidden_dim=16, dropout=0.5)
    for _ in range(3):
        a.train_epoch()
    b.set_weights(a.var(2), a.var(5))
    rng = np.random.default_rng(0)
    q3, q5 = rng.permutation(N)[:3].astype(np.int32), rng.permutation(N)[:5].astype(np.int32)
    q1000, q1500 = rng.integers(0, N, 1000).astype(np.int32), rng.integers(0, N, 1500).astype(np.int32)
    y64, y3 = rng.random((N, 64), np.float32), rng.random((N, 3), np.float32)
    steps = [("predict 3", lambda m: m.predict(nodes=q3)),
             ("evaluate split 3", lambda m: m.evaluate(split=3)),
             ("calibration 1000", lambda m: m.calibration(nodes=q1000, temperature=1.5, bins=7)),
             ("predict logp", lambda m: m.predict(logp=True)),
             ("propagate 64", lambda m: m.propagate(y64, 0.8, 2)),
             ("propagate 3 argmax", lambda m: m.propagate(y3, 0.8, 2, argmax=True)),
             ("correct_and_smooth", lambda m: m.correct_and_smooth(iters_correct=2, iters_smooth=2)),
             ("evaluate 5", lambda m: m.evaluate(nodes=q5)),
             ("predict 1500 logp", lambda m: m.predict(nodes=q1500, logp=True)),
             ("calibrate", lambda m: m.calibrate(apply=False)),
             ("label_propagation", lambda m: m.label_propagation(iters=2)),
             ("predict 3 again", lambda m: m.predict(nodes=q3))]
    ra, rb = check_any_order(a, b, steps)
    assert ra[9] == rb[9]                                                                # calibrate's dict: plain numbers
    assert same_result(ra[0], ra[11]) and same_result(rb[0], rb[11])
    a.close()
    b.close()


def test_queries_in_any_order_multilabel():
    """the same for a multi-label model: queries of 2 and 700 ids, the test split and every row"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.planted_multilabel(classes=41)
    N = ds["num_nodes"]
    kw = dict(seed=6, hidden_dim=16, dropout=0.5, multilabel=ds["multilabel"])
    a, b = HipGCNModel(ds, **kw), HipGCNModel(ds, **kw)
    for _ in range(3):
        a.train_epoch()
    b.set_weights(a.var(2), a.var(5))
    rng = np.random.default_rng(1)
    q2, q700 = rng.permutation(N)[:2].astype(np.int32), rng.integers(0, N, 700).astype(np.int32)
    steps = [("predict_multilabel 2", lambda m: m.predict_multilabel(nodes=q2)),
             ("predict_multilabel 700 prob", lambda m: m.predict_multilabel(nodes=q700, prob=True)),
             ("evaluate split 3", lambda m: m.evaluate(split=3)),
             ("predict_multilabel", lambda m: m.predict_multilabel()),
             ("predict_multilabel 2 again", lambda m: m.predict_multilabel(nodes=q2))]
    ra, rb = check_any_order(a, b, steps)
    assert same_result(ra[0], ra[4]) and same_result(rb[0], rb[4])
    a.close()
    b.close()


def test_save_and_load_weights(tmp_path):
    """a model saves its weights; a model with a different seed loads them: eval(2), eval(3) and predict() are bit-identical;
    a file with other widths is refused"""
    from cuda_gcn_amd.model import HipGCNModel, GcnHostError, read_weights
    ds = datagen.make_dataset("reddit-mini")
    a = HipGCNModel(ds, seed=1, hidden_dim=128, dropout=0.5)
    for _ in range(3):
        a.train_epoch()
    p = str(tmp_path / "w.gcnw")
    a.save_weights(p)
    w1, w2 = read_weights(p)
    assert np.array_equal(w1, a.var(2)) and np.array_equal(w2, a.var(5))
    b = HipGCNModel(ds, seed=2, hidden_dim=128, dropout=0.5)
    assert not np.array_equal(b.var(2), w1)
    b.load_weights(p)
    # the data terms are bit-identical; the L2 term of the reported loss is sum(W1^2) reduced by Adam's launch in `a` and by
    # set_weights' reduction in `b` (same value, possibly another last bit)
    for s in (2, 3):
        (la, aa), (lb, ab) = a.eval(s), b.eval(s)
        assert aa == ab and abs(la - lb) <= 1e-6 * max(1.0, abs(la)), (s, la, lb)
    pa, qa = a.predict()
    pb, qb = b.predict()
    assert np.array_equal(pa, pb) and np.array_equal(qa.view(np.uint32), qb.view(np.uint32))
    b.train_epoch()                                       # a loaded model trains on (Adam from scratch)
    c = HipGCNModel(ds, seed=1, hidden_dim=64, dropout=0.5)
    with pytest.raises(GcnHostError, match="hidden_dim=128"):
        c.load_weights(p)
    with pytest.raises(GcnHostError):
        c.load_weights(str(tmp_path / "missing.gcnw"))
    for m in (a, b, c):
        m.close()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("name,flags", [("cora-syn", 0), ("planted", 2097152), ("planted", 4194304)])
def test_two_ranks_predict_the_single_rank_result(tmp_path, name, flags):
    """world 2 (host-callback transport, both ranks on GPU 0): the union of the ranks' predictions, mapped by node id, equals
    the one-rank prediction with the same weights — with the ids kept and with the nodes renumbered by structure"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.planted_communities() if name == "planted" else datagen.make_dataset(name)
    one = HipGCNModel(ds, seed=4, hidden_dim=16, dropout=0.5)
    for _ in range(3):
        one.train_epoch()
    wpath, out = str(tmp_path / "w.gcnw"), str(tmp_path / "mr.npz")
    one.save_weights(wpath)
    pred, prob, logp = one.predict(logp=True)
    test = one.eval(3)
    one.close()
    port, world = _free_port(), 2
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mr_predict_worker.py"), name, wpath, out, str(flags), "16"],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=TEST_LIMIT_S - 30)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} failed:\n{outs[r][-3000:]}"
    got = np.load(out)
    if flags == 2097152:
        assert bool(got["renumbered"])
    if flags == 4194304:
        assert not bool(got["renumbered"])
    assert np.all(got["pred"] >= 0)
    tol = 2e-5 * max(1.0, float(np.abs(logp).max()))
    ok = clear_rows(logp, tol)
    assert ok.mean() > 0.98
    assert np.array_equal(got["pred"][ok], pred[ok])
    assert np.allclose(got["prob"], prob, rtol=0, atol=1e-5)
    assert np.allclose(got["logp"], logp, rtol=0, atol=tol)
    assert np.abs(got["test"] - np.array(test, np.float32)).max() <= 2e-5


# ---- the command line ---------------------------------------------------------------------------------------------------

def test_cli_save_load_predict(tmp_path):
    """gcn-hip reddit-mini with GCN_SAVE_WEIGHTS and GCN_PREDICT, then epochs 0 with GCN_LOAD_WEIGHTS: the same test line and
    the same predictions file, whose accuracy on the test split is the printed test_acc"""
    ds = datagen.make_dataset("reddit-mini")
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "reddit-mini.gcnbin"))
    w, p1, p2 = str(tmp_path / "w.gcnw"), str(tmp_path / "p1.txt"), str(tmp_path / "p2.txt")
    base = ["reddit-mini", "-", "-", "128", "-", "0.5", "-", "-"]

    def run(epochs, **env):
        r = subprocess.run(["timeout", "-k", "10", "50", HIP] + base + [epochs], cwd=str(tmp_path), env=dict(os.environ, GCN_SEED="3", **env),
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        return r.stdout.strip().splitlines(), r.stderr
    a, ea = run("4", GCN_SAVE_WEIGHTS=w, GCN_PREDICT=p1)
    b, eb = run("0", GCN_LOAD_WEIGHTS=w, GCN_PREDICT=p2)
    assert "weights written" in ea and "weights loaded" in eb and "predictions of 23296 nodes" in eb
    assert len([l for l in a if l.startswith("epoch=")]) == 4
    b = b[b.index("RUNNING ON GPU"):]                     # (the Parser's own note on the cache comes first)
    assert b[1] == "total training time=0.00000" and len(b) == 3, b

    def fields(line):
        return {k: float(v) for k, v in (t.split("=") for t in line.split())}
    ta, tb = fields(a[-1]), fields(b[-1])
    assert a[-1].startswith("test_loss=") and b[-1].startswith("test_loss=")
    assert ta["test_acc"] == tb["test_acc"] and abs(ta["test_loss"] - tb["test_loss"]) <= 1e-5
    t1, t2 = open(p1).read(), open(p2).read()
    assert t1 == t2
    rows = np.loadtxt(p1, ndmin=2)
    assert rows.shape == (ds["num_nodes"], 3) and np.array_equal(rows[:, 0], np.arange(ds["num_nodes"]))
    assert np.all((rows[:, 2] > 0) & (rows[:, 2] <= 1))
    test = ds["split"] == 3
    acc = float(np.mean(rows[test, 1].astype(np.int64) == ds["label"][test]))
    assert f"{acc:.5f}" == f"{ta['test_acc']:.5f}"
    # a weights file of another width is refused with a message
    bad = str(tmp_path / "bad.gcnw")
    from cuda_gcn_amd.model import write_weights
    write_weights(bad, np.zeros((602, 16), np.float32), np.zeros((16, 41), np.float32))
    r = subprocess.run(["timeout", "-k", "10", "50", HIP] + base + ["0"], cwd=str(tmp_path), env=dict(os.environ, GCN_LOAD_WEIGHTS=bad),
                       capture_output=True, text=True)
    assert r.returncode != 0 and "hidden_dim=16" in r.stderr
