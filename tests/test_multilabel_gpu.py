"""Multi-label training, evaluation and prediction on the GPU: gcnhip_bce_fwd_rows / gcnhip_bce_predict_rows against numpy
float64, the model's first epoch and its 10-epoch trace against a torch-CPU two-layer GCN with the same weights, dropout
masks and Adam, learning on the multi-label generator, HipGCNModel.predict_multilabel, two ranks, and gcn-hip with
GCN_MULTILABEL."""
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


def bce_reference(z, y, rows, count=None, scale=None):
    """(loss, dZ [n, C] (zero outside rows), TP, FP, FN, F1) in float64"""
    z = np.asarray(z, np.float64)
    zr, yr = z[rows], np.asarray(y, bool)[rows].astype(np.float64)
    n, C = zr.shape
    count = count or n
    with np.errstate(over="ignore"):
        terms = np.maximum(zr, 0) - zr * yr + np.log1p(np.exp(-np.abs(zr)))
        sig = np.where(zr >= 0, 1 / (1 + np.exp(-np.abs(zr))), np.exp(-np.abs(zr)) / (1 + np.exp(-np.abs(zr))))
    g = np.zeros_like(z)
    gr = (sig - yr) / (count * C)
    if scale is not None:
        gr = gr * np.asarray(scale, np.float64)[rows][:, None]
    g[rows] = gr
    pos, yy = zr > 0, yr > 0
    tp, fp, fn = int(np.sum(pos & yy)), int(np.sum(pos & ~yy)), int(np.sum(~pos & yy))
    f1 = 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0
    return terms.sum() / (n * C), g, tp, fp, fn, f1, np.abs(terms).sum() / (n * C)


def flag(names):
    from cuda_gcn_amd import model as M
    f = 0
    for k in names.split("|") if names else []:
        f |= getattr(M, k)
    return f


# ---- 1. the kernels ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 41, 64, 65, 121, 256])
def test_bce_kernel_against_numpy(C):
    from cuda_gcn_amd.ops import Device
    dev = Device(0)
    rng = np.random.default_rng(C)
    n = 700
    z = (rng.standard_normal((n, C)) * 4).astype(np.float32)
    special = np.array([30, -30, 100, -100, 1e30, -1e30], np.float32)
    idx = rng.integers(0, n * C, 60)
    z.reshape(-1)[idx] = special[np.arange(60) % 6]
    y = rng.random((n, C)) < 0.3
    scale = (rng.random(n) + 0.5).astype(np.float32)
    for rows in (np.arange(n, dtype=np.int32), np.sort(rng.choice(n, 333, replace=False)).astype(np.int32), np.array([n // 2], np.int32)):
        for sc in (None, scale):
            got = dev.bce_fwd_rows(z, y, rows=rows, training=True, grad_row_scale=sc, ld=(C + 3) // 4 * 4)
            loss, g, tp, fp, fn, f1, mag = bce_reference(z, y, rows, scale=sc)
            assert (got["tp"], got["fp"], got["fn"], got["rows"]) == (tp, fp, fn, rows.size)
            assert got["denom"] == np.float32(rows.size * C)
            assert abs(got["loss"] - loss) <= 1e-6 * max(1.0, mag) * 4, (got["loss"], loss)
            assert abs(got["f1"] - f1) <= 1e-6
            gg = got["grad"]
            assert np.all(np.isfinite(gg[rows]))
            outside = np.setdiff1d(np.arange(n), rows)
            assert np.all(np.isnan(gg[outside])), "rows outside the list were written"
            assert np.allclose(gg[rows], g[rows], rtol=1e-5, atol=1e-12 / (rows.size * C))
            again = dev.bce_fwd_rows(z, y, rows=rows, training=True, grad_row_scale=sc, ld=(C + 3) // 4 * 4)
            assert np.float32(again["loss_sum"]).tobytes() == np.float32(got["loss_sum"]).tobytes()
            assert np.array_equal(again["grad"][rows].view(np.uint32), gg[rows].view(np.uint32))
    # evaluation: no gradient; predicted sets and sigmoid
    got = dev.bce_fwd_rows(z, y, training=False)
    assert got["grad"] is None and got["rows"] == n
    q = np.array([5, 0, n - 1, 5], np.int32)
    sets, prob = dev.bce_predict_rows(z, rows=q, ld=(C + 3) // 4 * 4)
    assert np.array_equal(sets, z[q] > 0)
    zz = z[q].astype(np.float64)
    with np.errstate(over="ignore"):
        want = np.where(zz >= 0, 1 / (1 + np.exp(-np.abs(zz))), np.exp(-np.abs(zz)) / (1 + np.exp(-np.abs(zz))))
    assert np.allclose(prob, want, rtol=1e-6, atol=1e-7)
    dev.close()


def test_bce_kernel_refuses_out_of_range_classes():
    from cuda_gcn_amd.ops import Device, GcnHipError
    dev = Device(0)
    with pytest.raises(GcnHipError):
        dev.bce_fwd_rows(np.zeros((4, 257), np.float32), np.zeros((4, 257), bool))
    dev.close()


# ---- 2. / 3. the model against numpy and a torch-CPU reference -------------------------------------------------------------

def small(classes, seed=0):
    return datagen.planted_multilabel(n_comm=16, size=128, deg=12, feats=24, classes=classes, seed=datagen.DEFAULT_SEED + seed)


@pytest.mark.parametrize("flags", ["HOST_MASKS", "HOST_MASKS|MODULAR"])
def test_first_epoch_loss_f1_and_gradient(flags):
    from cuda_gcn_amd.model import HipGCNModel
    ds = small(41)
    y = ds["multilabel"]
    m = HipGCNModel(ds, seed=5, flags=flag(flags), hidden_dim=16, dropout=0.5, multilabel=y)
    w1 = m.var(2)
    loss, f1 = m.train_epoch()
    z, dz = m.var_reference(6), m.var_reference(6, grad=True)
    rows = np.flatnonzero(ds["split"] == 1)
    rl, g, tp, fp, fn, rf1, _ = bce_reference(z, y, rows)
    l2 = 5e-4 * float(np.sum(w1.astype(np.float64) ** 2)) / 2
    assert abs(loss - (rl + l2)) <= 2e-6, (loss, rl, l2)
    assert abs(f1 - rf1) <= 1e-6
    assert np.allclose(dz[rows], g[rows], rtol=2e-5, atol=1e-11)
    vl, vf = m.eval(2)
    v = np.flatnonzero(ds["split"] == 2)
    rl, _, _, _, _, rf1, _ = bce_reference(m.var_reference(6), y, v)
    assert abs(vl - (rl + 5e-4 * float(np.sum(m.var(2).astype(np.float64) ** 2)) / 2)) <= 2e-6 and abs(vf - rf1) <= 1e-6
    m.close()


def torch_trace(ds, y, seed, hidden, epochs, dropout=0.5, lr=0.01, wd=5e-4):
    """the reference's two-layer GCN in torch (float64 activations), the model's glorot weights and host dropout masks, BCE
    loss, the reference's Adam (W1 decayed): [(train_loss, train_f1, val_loss, val_f1)] per epoch"""
    import torch
    from cuda_gcn_amd import model as M
    N, F, C = ds["num_nodes"], ds["input_dim"], y.shape[1]
    gp, gi = ds["g_indptr"].astype(np.int64), ds["g_indices"].astype(np.int64)
    deg = np.diff(gp).astype(np.float64)
    r = np.repeat(np.arange(N), np.diff(gp))
    A = torch.sparse_coo_tensor(np.vstack([r, gi]), 1 / np.sqrt(deg[r] * deg[gi]), (N, N)).coalesce()
    fp_, fi = ds["f_indptr"].astype(np.int64), ds["f_indices"].astype(np.int64)
    fr = np.repeat(np.arange(N), np.diff(fp_))
    fv = torch.tensor(ds["f_val"], dtype=torch.float64)
    nnz = fv.numel()
    w = [M.glorot(F * hidden, F, hidden, seed).reshape(F, hidden), M.glorot(hidden * C, hidden, C, seed, F * hidden).reshape(hidden, C)]
    mom = [np.zeros_like(x) for x in w]
    vel = [np.zeros_like(x) for x in w]
    Y = torch.tensor(y, dtype=torch.float64)
    split = ds["split"]
    draws = F * hidden + hidden * C

    def forward(W1, W2, k0=None, k1=None):
        v = fv if k0 is None else fv * torch.tensor(k0, dtype=torch.float64) / (1 - dropout)
        X = torch.sparse_coo_tensor(np.vstack([fr, fi]), v, (N, F))
        H = torch.relu(torch.sparse.mm(A, torch.sparse.mm(X, W1)))
        if k1 is not None:
            H = H * torch.tensor(k1.reshape(N, hidden), dtype=torch.float64) / (1 - dropout)
        return torch.sparse.mm(A, H @ W2)

    def metrics(Z, s):
        rows = np.flatnonzero(split == s)
        zr, yr = Z[rows], Y[rows]
        loss = torch.nn.functional.binary_cross_entropy_with_logits(zr, yr, reduction="mean")
        pos, yy = (zr > 0).numpy(), yr.numpy() > 0
        tp, fpp, fn = np.sum(pos & yy), np.sum(pos & ~yy), np.sum(~pos & yy)
        return loss, (2 * tp / (2 * tp + fpp + fn) if 2 * tp + fpp + fn else 0.0)

    out = []
    for e in range(epochs):
        k0 = M.host_masks(nnz, dropout, seed, draws)
        k1 = M.host_masks(N * hidden, dropout, seed, draws + nnz)
        draws += nnz + N * hidden
        W1 = torch.tensor(w[0], dtype=torch.float64, requires_grad=True)
        W2 = torch.tensor(w[1], dtype=torch.float64, requires_grad=True)
        loss, f1 = metrics(forward(W1, W2, k0, k1), 1)
        loss.backward()
        l2 = wd * float(np.sum(w[0].astype(np.float64) ** 2)) / 2
        tl = float(loss) + l2
        grads = [W1.grad.numpy().astype(np.float32), W2.grad.numpy().astype(np.float32)]
        step = np.float32(lr * np.sqrt(1 - 0.999 ** (e + 1)) / (1 - 0.9 ** (e + 1)))
        for i in range(2):
            g = grads[i] + (np.float32(wd) * w[i] if i == 0 else 0)
            mom[i] = (0.9 * mom[i].astype(np.float64) + 0.1 * g).astype(np.float32)
            vel[i] = (0.999 * vel[i].astype(np.float64) + 0.001 * g.astype(np.float64) ** 2).astype(np.float32)
            w[i] = (w[i] - step * mom[i] / (np.sqrt(vel[i]) + np.float32(1e-8))).astype(np.float32)
        with torch.no_grad():
            vl, vf = metrics(forward(torch.tensor(w[0], dtype=torch.float64), torch.tensor(w[1], dtype=torch.float64)), 2)
        out.append((tl, f1, float(vl) + wd * float(np.sum(w[0].astype(np.float64) ** 2)) / 2, vf))
    return np.array(out)


@pytest.mark.parametrize("C,flags", [(41, "HOST_MASKS"), (41, "HOST_MASKS|MODULAR"), (121, "HOST_MASKS"), (121, "HOST_MASKS|MODULAR")])
def test_training_trace_matches_torch_cpu(C, flags):
    """10 epochs: loss within 2e-4 (f32 GPU sums against float64), micro-F1 within 2e-3 (a logit near 0 may fall either side)"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = small(C, seed=C)
    y = ds["multilabel"]
    m = HipGCNModel(ds, seed=7, flags=flag(flags), hidden_dim=16, dropout=0.5, multilabel=y)
    got = np.array([m.train_epoch() + m.eval(2) for _ in range(10)])
    m.close()
    want = torch_trace(ds, y, 7, 16, 10)
    assert np.abs(got[:, [0, 2]] - want[:, [0, 2]]).max() <= 2e-4, (got, want)
    assert np.abs(got[:, [1, 3]] - want[:, [1, 3]]).max() <= 2e-3, (got, want)


# ---- 4. learning -----------------------------------------------------------------------------------------------------------

def best_constant_f1(y):
    """micro-F1 of the best constant predicted set: the k most frequent classes, best k"""
    freq = np.sort(y.sum(0))[::-1].astype(np.float64)
    P, n = y.sum(), y.shape[0]
    k = np.arange(1, freq.size + 1)
    tp = np.cumsum(freq)
    return float(np.max(2 * tp / (2 * tp + (k * n - tp) + (P - tp))))


@pytest.mark.parametrize("C", [41, 121])
def test_learns_the_multilabel_generator(C):
    """validation micro-F1 after 100 epochs (learning rate 0.05: a sigmoid loss over classes that are ~3 % positive leaves
    every logit negative for the first tens of epochs at the reference's 0.01) is at least the best constant predictor's + 0.25"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.planted_multilabel(n_comm=32, size=256, classes=C)
    y = ds["multilabel"]
    m = HipGCNModel(ds, seed=1, hidden_dim=64, dropout=0.5, learning_rate=0.05, multilabel=y)
    tr = m.run_epochs(100)
    base = best_constant_f1(y[ds["split"] == 2])
    assert tr[-1, 3] >= base + 0.25, (tr[-1], base)
    assert np.all(np.isfinite(tr))
    m.close()


# ---- 5. predict_multilabel -------------------------------------------------------------------------------------------------

def cpu_logits(ds, w1, w2):
    N = ds["num_nodes"]
    gp, gi = ds["g_indptr"].astype(np.int64), ds["g_indices"].astype(np.int64)
    deg = np.diff(gp).astype(np.float64)
    r = np.repeat(np.arange(N), np.diff(gp))
    coef = 1 / np.sqrt(deg[r] * deg[gi])

    def agg(x):
        out = np.zeros_like(x)
        np.add.at(out, r, coef[:, None] * x[gi])
        return out
    X = ds["f_val"].reshape(N, -1).astype(np.float64)
    return agg(np.maximum(agg(X @ w1.astype(np.float64)), 0) @ w2.astype(np.float64))


@pytest.mark.parametrize("C,flags", [(41, ""), (121, ""), (41, "MODULAR"), (41, "BF16_TABLES"), (121, "ALL_ROWS")])
def test_predict_multilabel(tmp_path, C, flags):
    from cuda_gcn_amd.model import HipGCNModel
    ds = small(C)
    y = ds["multilabel"]
    kw = dict(seed=3, flags=flag(flags), hidden_dim=16, dropout=0.5, multilabel=y)
    m = HipGCNModel(ds, **kw)
    for _ in range(5):
        m.train_epoch()
    sets, prob = m.predict_multilabel(prob=True)
    N = ds["num_nodes"]
    assert sets.shape == (N, C) and sets.dtype == bool and prob.shape == (N, C)
    z = cpu_logits(ds, m.var(2), m.var(5))
    tol = (2e-2 if "BF16" in flags else 1e-4) * max(1.0, float(np.abs(z).max()))
    clear = np.abs(z) > tol
    assert clear.mean() > (0.8 if "BF16" in flags else 0.95)        # (bf16 tables: logits within ~2 % of the f32 ones)
    assert np.array_equal(sets[clear], (z > 0)[clear])
    assert np.allclose(prob, 1 / (1 + np.exp(-z)), rtol=0, atol=(2e-2 if "BF16" in flags else 1e-4))
    # a node subset = those rows of the full prediction, repeats allowed
    q = np.random.default_rng(0).choice(N, 77)
    qs, qp = m.predict_multilabel(nodes=q, prob=True)
    assert np.array_equal(qs, sets[q]) and np.array_equal(qp.view(np.uint32), prob[q].view(np.uint32))
    # a single-label call is refused
    from cuda_gcn_amd.model import GcnHostError
    with pytest.raises(GcnHostError, match="multi-label"):
        m.predict()
    # save, load, predict: the same sets
    w = str(tmp_path / "w.gcnw")
    m.save_weights(w)
    m2 = HipGCNModel(ds, **kw)
    m2.load_weights(w)
    assert np.array_equal(m2.predict_multilabel(), sets)
    m2.close()
    m.close()


@pytest.mark.parametrize("flags", ["HOST_MASKS", "HOST_MASKS|MODULAR", "", "NO_EVAL_LANE|NO_GRAPH"])
def test_predict_multilabel_between_epochs_changes_nothing(flags):
    from cuda_gcn_amd.model import HipGCNModel
    ds = small(41)
    y = ds["multilabel"]
    runs = []
    for with_predict in (False, True):
        m = HipGCNModel(ds, seed=9, flags=flag(flags), hidden_dim=16, dropout=0.5, multilabel=y)
        tr = [m.train_epoch() + m.eval(2) for _ in range(2)]
        if with_predict:
            m.predict_multilabel(prob=True)
            m.predict_multilabel(nodes=[3, 1, 4])
        tr += [m.train_epoch() + m.eval(2) for _ in range(2)]
        runs.append((np.array(tr, np.float32), m.var(2), m.var(5)))
        m.close()
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_single_label_model_refuses_predict_multilabel():
    from cuda_gcn_amd.model import HipGCNModel, GcnHostError
    m = HipGCNModel(datagen.make_dataset("cora-syn"), seed=1, hidden_dim=16)
    with pytest.raises(GcnHostError, match="single-label"):
        m.predict_multilabel()
    m.close()


# ---- 6. two ranks -----------------------------------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("flags", [0, 2097152, 4194304])
def test_two_ranks_match_one_rank(tmp_path, flags):
    """world 2 (host-callback transport, both ranks on GPU 0), ids kept or renumbered by structure: the 5-epoch trace matches
    one rank within f32 reassociation (dropout 0: device dropout decisions follow the row order, which renumbering changes), and
    the union of the ranks' predicted sets (by node id) equals one rank's"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.planted_multilabel(classes=121)
    one = HipGCNModel(ds, seed=11, hidden_dim=16, dropout=0.0, multilabel=ds["multilabel"])
    w0 = str(tmp_path / "w0.gcnw")
    one.save_weights(w0)
    trace = np.array([one.train_epoch() + one.eval(2) for _ in range(5)], np.float32)
    w = str(tmp_path / "w.gcnw")
    one.save_weights(w)
    sets, prob = one.predict_multilabel(prob=True)
    one.close()
    out = str(tmp_path / "mr.npz")
    port, world = _free_port(), 2
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mr_multilabel_worker.py"), w0, w, out, str(flags)],
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
    assert np.abs(got["trace"][:, [0, 2]] - trace[:, [0, 2]]).max() <= 1e-4
    assert np.abs(got["trace"][:, [1, 3]] - trace[:, [1, 3]]).max() <= 2e-3
    clear = np.abs(prob - 0.5) > 1e-4
    assert np.array_equal(got["sets"][clear], sets[clear])
    assert np.allclose(got["prob"], prob, rtol=0, atol=1e-5)


# ---- 7. the command line ---------------------------------------------------------------------------------------------------

def test_cli_multilabel(tmp_path):
    """GCN_MULTILABEL: _f1 fields, a test line and a predictions file of `node c1,c2,...` lines whose sets score the printed
    test_f1 on split 3; without the variable the lines keep the _acc fields"""
    from cuda_gcn_amd.model import write_labels
    ds = datagen.planted_multilabel(classes=41)
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "planted.gcnbin"))
    lab, pred = str(tmp_path / "labels.txt"), str(tmp_path / "pred.txt")
    write_labels(lab, ds["multilabel"])
    base = ["planted", "-", "-", "32", "-", "0.5", "-", "-", "20"]

    def run(**env):
        r = subprocess.run(["timeout", "-k", "10", "60", HIP] + base, cwd=str(tmp_path), env=dict(os.environ, GCN_SEED="3", **env),
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        return r.stdout.strip().splitlines()
    a = run(GCN_MULTILABEL=lab, GCN_PREDICT=pred)
    ep = [l for l in a if l.startswith("epoch=")]
    assert len(ep) == 20 and all(" train_f1=" in l and " val_f1=" in l and "_acc" not in l for l in ep)
    assert a[-1].startswith("test_loss=") and " test_f1=" in a[-1]
    test_f1 = float(a[-1].split("test_f1=")[1].split()[0])
    N, C = ds["num_nodes"], 41
    sets = np.zeros((N, C), bool)
    lines = open(pred).read().splitlines()
    assert len(lines) == N
    for i, line in enumerate(lines):
        parts = line.split(" ")
        assert int(parts[0]) == i and len(parts) <= 2
        if len(parts) == 2:
            sets[i, [int(c) for c in parts[1].split(",")]] = True
    t = ds["split"] == 3
    yy, pp = ds["multilabel"][t], sets[t]
    tp, fp, fn = np.sum(pp & yy), np.sum(pp & ~yy), np.sum(~pp & yy)
    assert abs(2 * tp / (2 * tp + fp + fn) - test_f1) <= 1e-5
    b = run()
    assert all(" train_acc=" in l for l in b if l.startswith("epoch=")) and " test_acc=" in b[-1]
