"""Per-class evaluation on the GPU: the two count kernels (gcnhip_confusion_rows, gcnhip_bce_class_counts_rows) against numpy,
HipGCN::evaluate against the model's own predictions and the dataset's truth (splits, node queries, flags, multi-label),
no side effects on training, several ranks, and the command line (GCN_REPORT)."""
import faulthandler
import os
import signal
import socket
import subprocess
import sys

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


def np_confusion(pred, truth, C, rows=None):
    """(matrix by numpy.add.at, listed rows whose truth is outside [0, C))"""
    pred, truth = np.asarray(pred, np.int64), np.asarray(truth, np.int64)
    if rows is not None:
        pred, truth = pred[rows], truth[rows]
    ok = (truth >= 0) & (truth < C)
    m = np.zeros((C, C), np.int64)
    np.add.at(m, (truth[ok], pred[ok]), 1)
    return m, int((~ok).sum())


def np_class_counts(sets, y):
    sets, y = np.asarray(sets, bool), np.asarray(y, bool)
    return np.stack([(sets & y).sum(0), (sets & ~y).sum(0), (~sets & y).sum(0)]).astype(np.int64)


# ---- the kernel entry points --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 3, 7, 41, 64])
def test_confusion_kernel_against_numpy(C):
    """random pred / truth, some truths at -1, all rows and a row list with repeats, sizes around the block and wave steps:
    exactly numpy.add.at's matrix and the right out-of-range count; the same launch twice gives the same output; n = 0 zeros"""
    from cuda_gcn_amd.ops import Device
    dev = Device(0)
    rng = np.random.default_rng(C)
    for n in (1, 63, 64, 65, 1023, 2049, 100003):
        pred = rng.integers(0, C, n).astype(np.int32)
        truth = rng.integers(0, C, n).astype(np.int32)
        truth[rng.random(n) < 0.1] = -1
        got, bad = dev.confusion_rows(pred, truth, C)
        want, wbad = np_confusion(pred, truth, C)
        assert np.array_equal(got, want) and bad == wbad, n
        assert int(got.sum()) + bad == n
        rows = rng.integers(0, n, 2 * n // 3 + 1).astype(np.int32)              # repeats, any order
        got, bad = dev.confusion_rows(pred, truth, C, rows=rows)
        want, wbad = np_confusion(pred, truth, C, rows)
        assert np.array_equal(got, want) and bad == wbad, n
        again, bad2 = dev.confusion_rows(pred, truth, C, rows=rows)
        assert np.array_equal(again, got) and bad2 == bad
    got, bad = dev.confusion_rows(pred, truth, C, rows=np.zeros(0, np.int32))
    assert not got.any() and bad == 0
    got, bad = dev.confusion_rows(np.zeros(0, np.int32), np.zeros(0, np.int32), C)
    assert not got.any() and bad == 0
    dev.close()


def test_confusion_kernel_skew_and_limits():
    """90 % of the rows in one cell (the worst case of the LDS atomics) is still exact; a truth of C or above is out of range;
    65 classes are refused"""
    from cuda_gcn_amd.ops import Device, GcnHipError
    dev = Device(0)
    rng = np.random.default_rng(9)
    C, n = 7, 400000
    pred = rng.integers(0, C, n).astype(np.int32)
    truth = rng.integers(0, C, n).astype(np.int32)
    hot = rng.random(n) < 0.9
    pred[hot], truth[hot] = 2, 2
    got, bad = dev.confusion_rows(pred, truth, C)
    want, wbad = np_confusion(pred, truth, C)
    assert np.array_equal(got, want) and bad == wbad == 0
    assert got[2, 2] > 0.9 * n
    pred[:] = 3
    truth[:] = 3                                               # every lane of every wave on one cell
    got, bad = dev.confusion_rows(pred, truth, C)
    assert got[3, 3] == n and int(got.sum()) == n and bad == 0
    truth[:1000] = C
    truth[1000:1500] = 2 ** 30
    got, bad = dev.confusion_rows(pred, truth, C)
    assert bad == 1500 and got[3, 3] == n - 1500
    with pytest.raises(GcnHipError):
        dev.confusion_rows(np.zeros(10, np.int32), np.zeros(10, np.int32), 65)
    dev.close()


@pytest.mark.parametrize("C", [1, 31, 32, 33, 64, 121, 256])
def test_class_counts_kernel_against_numpy(C):
    """random logits with exact zeros (not predicted: the rule is z > 0) and large finite magnitudes, random multi-hot truth:
    TP / FP / FN per class exactly numpy's, their sums the counts of gcnhip_bce_fwd_rows on the same inputs; all rows and a
    row list with repeats; twice the same output; n = 0 zeros"""
    from cuda_gcn_amd.ops import Device
    dev = Device(0)
    rng = np.random.default_rng(C)
    n = 3001
    z = (rng.standard_normal((n, C)) * 3).astype(np.float32)
    z[rng.random((n, C)) < 0.05] = 0.0
    z[rng.random((n, C)) < 0.02] = 3e38
    z[rng.random((n, C)) < 0.02] = -3e38
    y = rng.random((n, C)) < 0.3
    ld = (C + 3) // 4 * 4
    for rows in (None, rng.integers(0, n, 2000).astype(np.int32), np.arange(0, n, 64, dtype=np.int32)):
        got = dev.bce_class_counts_rows(z, y, rows=rows, ld=ld)
        sel = slice(None) if rows is None else rows
        want = np_class_counts(z[sel] > 0, y[sel])
        assert np.array_equal(got, want)
        assert np.array_equal(dev.bce_class_counts_rows(z, y, rows=rows, ld=ld), got)
        loss = dev.bce_fwd_rows(z, y, rows=rows, training=False, ld=ld)
        assert (loss["tp"], loss["fp"], loss["fn"]) == tuple(int(v) for v in got.sum(axis=1))
    assert not dev.bce_class_counts_rows(z, y, rows=np.zeros(0, np.int32)).any()
    dev.close()


def test_class_counts_kernel_refuses_more_than_256_classes():
    from cuda_gcn_amd.ops import Device, GcnHipError
    dev = Device(0)
    with pytest.raises(GcnHipError):
        dev.bce_class_counts_rows(np.zeros((4, 257), np.float32), np.zeros((4, 257), bool))
    dev.close()


# ---- the model ----------------------------------------------------------------------------------------------------------

def flag(names):
    from cuda_gcn_amd import model as M
    f = 0
    for k in str(names).split("|"):
        f |= getattr(M, k) if k != "0" else 0
    return f


def check_single_label(m, ds, splits=(1, 2, 3)):
    """evaluate(split) against numpy on the model's own predict() and the labels, and against eval(split)'s accuracy"""
    C = ds["output_dim"]
    pred, _, logp = m.predict(logp=True)
    for s in splits:
        sel = np.flatnonzero(ds["split"] == s)
        r = m.evaluate(s)
        want, unl = np_confusion(pred, ds["label"], C, sel)
        assert r["confusion"].dtype == np.int64 and r["confusion"].shape == (C, C)
        assert np.array_equal(r["confusion"], want), s
        assert r["unlabelled"] == unl and r["rows"] == int(want.sum())
        assert np.array_equal(r["support"], want.sum(axis=1).astype(np.float64))
        # eval's accuracy counts a tie of the true class with the top as correct; predict takes the lowest class of a tie
        top = np.sort(logp[sel], axis=1)
        ties = int(np.sum(top[:, -1] == top[:, -2])) if C > 1 else 0
        _, acc = m.eval(s)
        print(f"split {s}: rows {r['rows']} trace {np.trace(want)} accuracy {r['accuracy']:.7f} eval {acc:.7f} ties {ties} macro_f1 {r['macro_f1']:.5f}")
        assert abs(np.trace(want) / r["rows"] - acc) <= ties / r["rows"] + 1e-6
        assert ties == 0                                       # expected on these generated sets: the check above stays tight
        assert r["accuracy"] == np.trace(want) / r["rows"] and abs(r["micro_f1"] - r["accuracy"]) <= 1e-15


@pytest.mark.parametrize("name,hidden,epochs", [("cora-syn", 16, 10), ("tiny-syn", 16, 10), ("reddit-mini", 128, 3)])
def test_evaluate_matches_own_predictions(name, hidden, epochs):
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.make_dataset(name)
    m = HipGCNModel(ds, seed=3, hidden_dim=hidden, dropout=0.5)
    for _ in range(epochs):
        m.train_epoch()
    check_single_label(m, ds)
    # all nodes, and a random query with repeats
    pred, _ = m.predict()
    C = ds["output_dim"]
    r = m.evaluate()
    want, unl = np_confusion(pred, ds["label"], C)
    assert np.array_equal(r["confusion"], want) and r["unlabelled"] == unl and r["rows"] + unl == ds["num_nodes"]
    rng = np.random.default_rng(0)
    for n in (1, 65, 1000):
        q = rng.integers(0, ds["num_nodes"], n).astype(np.int32)
        q = np.concatenate([q, q[: n // 2 + 1]])
        r = m.evaluate(nodes=q)
        want, unl = np_confusion(pred, ds["label"], C, q)
        assert np.array_equal(r["confusion"], want) and r["unlabelled"] == unl
    r = m.evaluate(nodes=np.zeros(0, np.int32))
    assert not r["confusion"].any() and r["rows"] == 0 and r["macro_f1"] == 0.0
    m.close()


@pytest.mark.parametrize("flags", ["0", "EDGE_COEF", "BF16_TABLES", "NO_AGG_FIRST_EVAL", "ALL_ROWS", "MODULAR"])
def test_evaluate_agrees_with_predict_under_flags(flags):
    """each variant against ITS OWN predict() (a different rounding may move an argmax between variants)"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.make_dataset("reddit-mini" if flags not in ("MODULAR",) else "cora-syn")
    m = HipGCNModel(ds, seed=5, flags=flag(flags), hidden_dim=128 if ds["num_nodes"] > 10000 else 16, dropout=0.5)
    for _ in range(3):
        m.train_epoch()
    check_single_label(m, ds, splits=(2, 3))
    m.close()


def test_evaluate_argument_errors():
    from cuda_gcn_amd.model import HipGCNModel, GcnHostError
    ds = datagen.make_dataset("tiny-syn")
    m = HipGCNModel(ds, seed=1, hidden_dim=16, dropout=0.5)
    with pytest.raises(ValueError):
        m.evaluate(split=4)
    with pytest.raises(ValueError):
        m.evaluate(split=2, nodes=[1])
    with pytest.raises(GcnHostError):
        m.evaluate(nodes=[ds["num_nodes"]])
    m.close()
    # more classes than the kernel takes: an error with a message, never a wrong answer
    big = dict(ds, output_dim=65)
    m = HipGCNModel(big, seed=1, hidden_dim=16, dropout=0.5)
    with pytest.raises(GcnHostError, match="64 classes"):
        m.evaluate(2)
    m.close()


@pytest.mark.parametrize("C", [41, 121])
def test_evaluate_multilabel(C):
    """tp / fp / fn per class equal numpy's from predict_multilabel() and the truth, for every split, all nodes and a query with
    repeats; micro_f1 is eval(split)'s F1 to float32 rounding"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.planted_multilabel(classes=C)
    y = ds["multilabel"]
    m = HipGCNModel(ds, seed=3, hidden_dim=32, dropout=0.5, learning_rate=0.05, multilabel=y)
    for _ in range(15):
        m.train_epoch()
    sets = m.predict_multilabel()
    for s in (1, 2, 3):
        sel = ds["split"] == s
        r = m.evaluate(s)
        want = np_class_counts(sets[sel], y[sel])
        assert np.array_equal(np.stack([r["tp"], r["fp"], r["fn"]]), want), s
        assert r["tp"].dtype == np.int64 and r["rows"] == int(sel.sum()) and "confusion" not in r
        _, f1 = m.eval(s)
        print(f"C {C} split {s}: micro_f1 {r['micro_f1']:.8f} eval {f1:.8f} macro_f1 {r['macro_f1']:.5f}")
        assert abs(r["micro_f1"] - f1) <= 1e-6 * max(abs(f1), 1e-30)
        assert np.array_equal(r["support"], y[sel].sum(axis=0).astype(np.float64))
    r = m.evaluate()
    assert np.array_equal(np.stack([r["tp"], r["fp"], r["fn"]]), np_class_counts(sets, y))
    q = np.random.default_rng(1).integers(0, ds["num_nodes"], 700).astype(np.int32)
    q = np.concatenate([q, q[:100]])
    r = m.evaluate(nodes=q)
    assert np.array_equal(np.stack([r["tp"], r["fp"], r["fn"]]), np_class_counts(sets[q], y[q])) and r["rows"] == q.size
    m.close()


@pytest.mark.parametrize("flags,multilabel", [("0", False), ("EVAL_LANE", False), ("NO_GRAPH", False), ("0", True)])
def test_evaluate_between_epochs_changes_nothing(flags, multilabel):
    """two models with the same seed train in lockstep, one calling evaluate() between epochs: their run_epochs traces (the
    captured epoch graph replayed by default), weights, test metrics and the logits of the last forward are bit-identical"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.planted_multilabel(classes=41, size=128) if multilabel else datagen.make_dataset("cora-syn")
    kw = dict(seed=6, flags=flag(flags), hidden_dim=16, dropout=0.5, multilabel=ds["multilabel"] if multilabel else None)
    a, b = HipGCNModel(ds, **kw), HipGCNModel(ds, **kw)
    ta, tb = [], []
    q = np.arange(0, ds["num_nodes"], 7, dtype=np.int32)
    for e in range(4):
        ta.append(a.run_epochs(1))
        tb.append(b.run_epochs(1))
        b.evaluate(2)
        b.evaluate(1)
        b.evaluate()
        b.evaluate(nodes=q)
    ta.append(np.array([a.train_epoch() + a.eval(2)], np.float32))
    tb.append(np.array([b.train_epoch() + b.eval(2)], np.float32))
    ta, tb = np.concatenate(ta), np.concatenate(tb)
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32)), (ta, tb)
    for k in (2, 5):
        assert np.array_equal(a.var(k).view(np.uint32), b.var(k).view(np.uint32)), k
    assert a.eval(3) == b.eval(3)
    assert np.array_equal(a.var(6).view(np.uint32), b.var(6).view(np.uint32))
    a.close()
    b.close()


# ---- several ranks ------------------------------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("name,world,flags", [("cora-syn", 2, 0), ("cora-syn", 3, 0), ("multilabel-121", 2, 0), ("multilabel-41", 3, 2097152)])
def test_ranks_return_the_same_exact_totals(tmp_path, name, world, flags):
    """logical ranks on GPU 0 (host-callback transport): every rank returns the same totals, and they equal numpy on the union
    of the SAME world's own predictions (a partition reassociates sums: another world may move an argmax)"""
    from cuda_gcn_amd.model import HipGCNModel
    ml = name.startswith("multilabel-")
    ds = datagen.planted_multilabel(classes=int(name.split("-")[1])) if ml else datagen.make_dataset(name)
    one = HipGCNModel(ds, seed=4, hidden_dim=16, dropout=0.5, multilabel=ds["multilabel"] if ml else None)
    for _ in range(5):
        one.train_epoch()
    wpath, out = str(tmp_path / "w.gcnw"), str(tmp_path / "mr.npz")
    one.save_weights(wpath)
    one.close()
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mr_report_worker.py"), name, wpath, out, str(flags), "16"],
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
    pred, C = got["pred"], ds["output_dim"]

    def want(sel):
        if ml:
            return np_class_counts(pred[sel], ds["multilabel"][sel])
        return np_confusion(pred, ds["label"], C, sel)[0]
    cases = [("s1", np.flatnonzero(ds["split"] == 1)), ("s2", np.flatnonzero(ds["split"] == 2)), ("s3", np.flatnonzero(ds["split"] == 3)),
             ("all", np.arange(ds["num_nodes"])), ("query", got["query"])]
    for tag, sel in cases:
        w = want(sel)
        for r in range(world):
            assert np.array_equal(got[f"r{r}_{tag}"], w), (tag, r)
        if tag != "query":
            for r in range(world):
                assert got[f"r{r}_{tag}_rows"][0] == (sel.size if ml else int(w.sum()))


# ---- the command line ---------------------------------------------------------------------------------------------------

def _strip_times(lines):
    return [" ".join(t for t in l.split() if not t.startswith("time=")) for l in lines if "time=" in l or l.startswith("RUNNING")]


def _parse_report(path, C, matrix):
    lines = open(path).read().splitlines()
    per = np.array([[float(t) for t in l.split()[1::2]] for l in lines[:C]])
    assert all(l.split()[0::2] == ["class", "support", "precision", "recall", "f1"] for l in lines[:C])
    assert np.array_equal(per[:, 0], np.arange(C))
    s = lines[C].split()
    assert s[0] == "macro_f1" and s[2] == "micro_f1"
    m = None
    if matrix:
        assert lines[C + 1] == "confusion" and len(lines) == 2 * C + 2
        m = np.array([[int(t) for t in l.split()] for l in lines[C + 2:]], np.int64)
        assert m.shape == (C, C)
    else:
        assert len(lines) == C + 1
    return per, float(s[1]), float(s[3]), m


@pytest.mark.parametrize("multilabel", [False, True])
def test_cli_report(tmp_path, multilabel):
    """gcn-hip cora-syn (text data) with GCN_REPORT and GCN_SAVE_WEIGHTS: the file parses, its counts are those of the Python
    evaluate(3) of a model with the saved weights, and stdout is that of a run without the variable apart from time= fields"""
    from cuda_gcn_amd import model as M
    ds = datagen.make_dataset("cora-syn")
    root = str(tmp_path / "data")
    datagen.write_text(ds, root, "cora-syn")
    env = {}
    y = None
    if multilabel:
        y = datagen.multilabel_from_communities(ds["label"], classes=41)
        M.write_labels(str(tmp_path / "labels.txt"), y)
        env["GCN_MULTILABEL"] = str(tmp_path / "labels.txt")
    w, rep, pr = str(tmp_path / "w.gcnw"), str(tmp_path / "report.txt"), str(tmp_path / "pred.txt")
    args = ["cora-syn", "-", "-", "16", "-", "0.5", "0.05" if multilabel else "-", "-", "12"]

    def run(**extra):
        r = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=dict(os.environ, GCN_SEED="3", **env, **extra),
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        return r.stdout.strip().splitlines(), r.stderr
    a, ea = run(GCN_REPORT=rep, GCN_SAVE_WEIGHTS=w, GCN_PREDICT=pr)
    b, eb = run()
    assert "per-class report of the test split" in ea and "per-class report" not in eb
    assert len(a) == len(b) and _strip_times(a) == _strip_times(b) and len(_strip_times(a)) >= 14
    assert os.path.exists(pr)
    parsed = M.load_dataset(root, "cora-syn")                  # the text as the program read it
    C = 41 if multilabel else ds["output_dim"]
    m = M.HipGCNModel(parsed, seed=1, hidden_dim=16, dropout=0.5, multilabel=y)
    m.load_weights(w)
    r = m.evaluate(3)
    assert r["rows"] == int((ds["split"] == 3).sum())
    m.close()
    per, macro, micro, mat = _parse_report(rep, C, matrix=not multilabel)
    if multilabel:
        print("test split: tp", int(r["tp"].sum()), "fp", int(r["fp"].sum()), "fn", int(r["fn"].sum()))
        assert np.array_equal(r["tp"] + r["fn"], y[ds["split"] == 3].sum(axis=0)) and r["fn"].sum() > 0
    else:
        assert np.array_equal(mat, r["confusion"]) and mat.sum() == int((ds["split"] == 3).sum())
        test_acc = float(a[-1].split("test_acc=")[1].split()[0])
        assert abs(np.trace(mat) / mat.sum() - test_acc) <= 1e-5
    assert np.array_equal(per[:, 1], r["support"])
    for col, k in ((2, "precision"), (3, "recall"), (4, "f1")):
        assert np.allclose(per[:, col], r[k], rtol=0, atol=5.1e-7), k            # six decimals in the file
    assert abs(macro - r["macro_f1"]) <= 5.1e-7 and abs(micro - r["micro_f1"]) <= 5.1e-7
    # epochs 0 with the saved weights: the same report
    args[-1] = "0"
    rep2 = str(tmp_path / "report2.txt")
    run(GCN_REPORT=rep2, GCN_LOAD_WEIGHTS=w)
    assert open(rep2).read() == open(rep).read()
