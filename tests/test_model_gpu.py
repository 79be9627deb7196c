"""GPU parity of the whole training path (HipGCN behind libgcnhost.so) against
the CPU oracle and the reference-generated golden traces.

Tolerance (stated in SURVEY §8d, f32 path): with identical initial weights and
identical dropout decisions (dropout = 0, or HOST_MASKS replaying the
reference's RNG stream) the per-epoch trace must satisfy
    |d loss| <= 2e-4 for epochs 1..10 and <= 2e-3 through epoch 100,
    |d acc|  <= 2 / (labelled rows of the split)  (two borderline rows)
— the only differences are f32 summation order / FMA contraction.
"""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from cuda_gcn_amd import datagen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def check_trace(got, want, ds, early=10):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    n = got.shape[0]
    assert want.shape[0] >= n
    want = want[:n]
    dl = np.abs(got[:, [0, 2]] - want[:, [0, 2]])
    assert dl[:early].max() <= 2e-4, f"early loss diff {dl[:early].max():.2e}"
    assert dl.max() <= 2e-3, f"loss diff {dl.max():.2e}"
    n_train = int((ds["split"] == 1).sum())
    n_val = int((ds["split"] == 2).sum())
    assert np.abs(got[:, 1] - want[:, 1]).max() <= 2.0 / n_train + 1e-6
    assert np.abs(got[:, 3] - want[:, 3]).max() <= 2.0 / n_val + 1e-6


def oracle_trace(oracle, ds, seed, epochs, **hyper):
    m = oracle.model(ds, seed_time=seed, **hyper)
    tr = np.zeros((epochs, 4), np.float32)
    for e in range(epochs):
        tr[e, 0], tr[e, 1] = m.train_epoch()
        tr[e, 2], tr[e, 3] = m.eval(2)
    test = m.eval(3)
    return tr, test, m


@pytest.mark.parametrize("name,hidden", [("tiny-syn", 16), ("cora-syn", 16), ("tiny-syn", 128)])
@pytest.mark.parametrize("mode", ["fused", "modular"])
def test_trace_dropout0_vs_oracle(oracle, name, hidden, mode):
    from cuda_gcn_amd.model import HipGCNModel, MODULAR
    ds = datagen.make_dataset(name)
    epochs = 100 if name == "tiny-syn" else 40
    want, want_test, om = oracle_trace(oracle, ds, 5, epochs, hidden_dim=hidden, dropout=0.0)
    m = HipGCNModel(ds, seed=5, flags=MODULAR if mode == "modular" else 0, hidden_dim=hidden, dropout=0.0, epochs=epochs)
    got = np.array([m.train_epoch() + m.eval(2) for _ in range(epochs)], np.float32)
    check_trace(got, want, ds)
    tl, ta = m.eval(3)
    assert abs(tl - want_test[0]) <= 2e-3 and abs(ta - want_test[1]) <= 2.0 / int((ds["split"] == 3).sum()) + 1e-6
    # final weights close to the CPU path's
    for k in (2, 5):
        w = m.var(k).reshape(-1)
        assert np.abs(w - om.var(k)).max() <= 5e-3
    m.close(); om.close()


@pytest.mark.parametrize("name,hidden", [("tiny-syn", 16), ("cora-syn", 16),
                                         ("tiny-syn", 40), ("tiny-syn", 6),    # 40 -> ld 48, 6 -> ld 8: padded rows (ld != cols)
                                         ("cora-syn", 128), ("pubmed-syn", 128)])  # hidden 128 on >= 2048 rows: the class layer's bf16x3 kernels at 7 and 3 classes (one k-step)
@pytest.mark.parametrize("mode", ["fused", "modular"])
def test_trace_dropout_host_masks_vs_oracle(oracle, name, hidden, mode):
    """dropout 0.5 with the reference's own RNG decisions replayed on the host"""
    from cuda_gcn_amd.model import HipGCNModel, MODULAR, HOST_MASKS
    ds = datagen.make_dataset(name)
    epochs = 60 if name == "tiny-syn" else (30 if hidden < 128 else 12)
    want, _, om = oracle_trace(oracle, ds, 3, epochs, hidden_dim=hidden, dropout=0.5)
    m = HipGCNModel(ds, seed=3, flags=HOST_MASKS | (MODULAR if mode == "modular" else 0), hidden_dim=hidden, dropout=0.5, epochs=epochs)
    got = np.array([m.train_epoch() + m.eval(2) for _ in range(epochs)], np.float32)
    check_trace(got, want, ds)
    m.close(); om.close()


def test_rmat_shaped_model_trace_vs_oracle(oracle):
    """BASELINE configs[4]'s model shape (R-MAT graph, dense 256 features -> 128 -> 41) at a scale whose largest
    degree product (9705^2 at scale 16) is still below 2^31, so the reference's int arithmetic (module.cpp:91-93)
    is defined and the oracle is a valid checker: 6 epochs with the reference's dropout decisions replayed"""
    from cuda_gcn_amd.model import HipGCNModel, HOST_MASKS
    ds = datagen.make_dataset("rmat-16-256")
    assert int(np.diff(ds["g_indptr"]).max()) ** 2 < 2 ** 31
    om = oracle.model(ds, seed_time=2, hidden_dim=128, dropout=0.5)
    m = HipGCNModel(ds, seed=2, flags=HOST_MASKS, hidden_dim=128, dropout=0.5, epochs=6)
    assert m.schedule().startswith("dealt") or m.schedule() == "degree"
    for e in range(6):
        got = m.train_epoch() + m.eval(2)
        want = om.train_epoch() + om.eval(2)
        assert abs(got[0] - want[0]) <= 2e-4 and abs(got[2] - want[2]) <= 2e-4, (e, got, want)
        assert abs(got[1] - want[1]) <= 2.0 / int((ds["split"] == 1).sum()) and abs(got[3] - want[3]) <= 2.0 / int((ds["split"] == 2).sum())
    gt, wt = m.eval(3), om.eval(3)
    assert abs(gt[0] - wt[0]) <= 2e-4
    m.close(); om.close()


def test_rmat_model_trace_vs_wide_oracle(oracle):
    """BASELINE configs[4]'s family WITH a hub whose int degree product overflows: R-MAT scale 20 (1 048 576 nodes, 32.5 M
    stored edges; the top hub has degree 64 619 > 46 340, so module.cpp:92's int product of its own self loop is undefined —
    the reference's arithmetic wraps it negative and the hub's row becomes NaN).  The HIP path forms the product in 64 bits
    (SURVEY App. C); the oracle's wide-degree variant does the same and is pinned bit-for-bit to the reference wherever the
    int product is defined (tests/test_oracle_pin.py).  Model 32 -> 64 -> 41 (the aggregation is what the hubs exercise —
    64 columns are one XCD-sliced launch of the hidden-width kernel; the narrow widths keep the CPU side of the test at
    ~20 s per epoch), 2 epochs + the test split with the reference's dropout decisions replayed.

    What is compared.  Accuracies and the validation / test losses (10 K rows): the oracle's own numbers, at the usual
    tolerances.  The TRAINING loss is a mean over 1.03 M rows, which the reference accumulates sequentially in one float
    (module.cpp:144,154): at this count that sum carries ~1e-3 of rounding of its own (measured: +9e-4 at scale 19, +3.7e-3
    at scale 20 against the float64 mean of the SAME logits; the HIP path adds block partials and stays at 1e-6).  So the
    training loss is checked against the float64 mean of the ORACLE's logits (+ the L2 term of the weights the forward
    used), and the training logits themselves element by element."""
    from cuda_gcn_amd.model import HipGCNModel, HOST_MASKS
    scale = int(os.environ.get("RMAT_WIDE_SCALE", "20"))
    ds = datagen.make_dataset(f"rmat-{scale}-32")
    gp, gi, N = ds["g_indptr"], ds["g_indices"], ds["num_nodes"]
    assert int(np.diff(gp).max()) > 46340 and oracle.overflowing_edges(gp, gi) >= 1, "no overflowing degree product: the wide variant would not be exercised"
    truth = np.where(ds["split"] == 1, ds["label"], -1)
    rows = np.nonzero(truth >= 0)[0]

    def f64_mean_loss(Z):
        Zr = Z[rows].astype(np.float64)
        Zr -= Zr.max(1, keepdims=True)
        return float((np.log(np.exp(Zr).sum(1)) - Zr[np.arange(rows.size), truth[rows]]).mean())
    oracle.set_wide_degree(True)
    try:
        om = oracle.model(ds, seed_time=4, hidden_dim=64, dropout=0.5)
        m = HipGCNModel(ds, seed=4, flags=HOST_MASKS, hidden_dim=64, dropout=0.5, epochs=2)
        n_tr, n_va = int((ds["split"] == 1).sum()), int((ds["split"] == 2).sum())
        for e in range(2):
            l2 = 5e-4 * float((om.var(2).astype(np.float64) ** 2).sum()) / 2        # gcn.cpp:98-105, the weights this forward uses
            got_t, want_t = m.train_epoch(), om.train_epoch()
            Zg, Zo = m.var_reference(6), om.var(6).reshape(N, -1)
            want_loss = f64_mean_loss(Zo) + l2
            assert np.isfinite(want_t).all() and np.isfinite(got_t).all(), (e, got_t, want_t)
            assert abs(got_t[0] - want_loss) <= 2e-4, (e, got_t, want_loss, want_t)
            assert abs(want_t[0] - want_loss) <= 2e-2, (e, want_t, want_loss)           # the reference's own float accumulation: loose
            assert abs(got_t[1] - want_t[1]) <= 2.0 / n_tr, (e, got_t, want_t)
            Zg_s, Zo_s = Zg[rows] - Zg[rows].max(1, keepdims=True), Zo[rows] - Zo[rows].max(1, keepdims=True)
            assert np.abs(Zg_s - Zo_s).max() <= 1e-3 * max(1.0, float(np.abs(Zo_s).max())), (e, float(np.abs(Zg_s - Zo_s).max()))
            got_v, want_v = m.eval(2), om.eval(2)
            assert abs(got_v[0] - want_v[0]) <= 2e-4 and abs(got_v[1] - want_v[1]) <= 2.0 / n_va, (e, got_v, want_v)
        gt, wt = m.eval(3), om.eval(3)
        assert abs(gt[0] - wt[0]) <= 2e-4, (gt, wt)
        m.close(); om.close()
    finally:
        oracle.set_wide_degree(False)


@pytest.mark.parametrize("name,seed,dropout", [("cora-syn", 1, 0.0), ("cora-syn", 2, 0.5), ("citeseer-syn", 1, 0.0),
                                               ("pubmed-syn", 1, 0.5), ("tiny-syn", 3, 0.5)])
def test_trace_vs_reference_golden(name, seed, dropout):
    """against the traces the REFERENCE's own objects produced (tests/golden/traces.npz)"""
    from cuda_gcn_amd.model import HipGCNModel, HOST_MASKS
    g = np.load(os.path.join(GOLD, "traces.npz"))
    want = g[f"{name}_s{seed}_d{dropout}_trace"]
    ds = datagen.make_dataset(name)
    epochs = min(want.shape[0], 40)
    m = HipGCNModel(ds, seed=seed, flags=HOST_MASKS if dropout > 0 else 0, hidden_dim=16, dropout=dropout, epochs=epochs)
    got = np.array([m.train_epoch() + m.eval(2) for _ in range(epochs)], np.float32)
    check_trace(got, want, ds)
    m.close()


@pytest.mark.parametrize("edge_coef", [False, True])
@pytest.mark.parametrize("all_rows", [True, False])
def test_first_epoch_tensors_vs_oracle(oracle, all_rows, edge_coef):
    """every intermediate of one training epoch (H0, H1, Z0, Z and their gradients).  By default the last
    aggregation computes only the rows of the scored split (all that the loss reads, module.cpp:131-133):
    then Z is compared on those rows; with ALL_ROWS on every row.  Default: the factored aggregation (the gathered matrices
    are stored pre-multiplied by dinv of their row: var_reference divides that back); EDGE_COEF: the reference's per-edge
    coefficients, every variable stored as the reference stores it."""
    from cuda_gcn_amd.model import HipGCNModel, HOST_MASKS, ALL_ROWS, EDGE_COEF
    ds = datagen.make_dataset("cora-syn")
    N, H, C = ds["num_nodes"], 16, ds["output_dim"]
    om = oracle.model(ds, seed_time=9, hidden_dim=H, dropout=0.5)
    m = HipGCNModel(ds, seed=9, flags=HOST_MASKS | (ALL_ROWS if all_rows else 0) | (EDGE_COEF if edge_coef else 0), hidden_dim=H, dropout=0.5)
    dinv, factored = m.row_scale()
    assert factored == (not edge_coef)
    assert np.allclose(dinv, 1.0 / np.sqrt(np.diff(ds["g_indptr"])), rtol=1e-7)
    if edge_coef:
        assert np.array_equal(m.var(3), m.var_reference(3))
    assert np.array_equal(m.var(2).reshape(-1), om.var(2))          # same Glorot init as gcn-seq
    assert np.array_equal(m.var(5).reshape(-1), om.var(5))
    a, b = m.train_epoch(), om.train_epoch()
    assert abs(a[0] - b[0]) <= 2e-5 and abs(a[1] - b[1]) <= 1e-6
    shapes = {1: (N, H), 3: (N, H), 4: (N, C), 6: (N, C)}
    for k, shp in shapes.items():
        want = om.var(k).reshape(shp)
        if k == 6:
            want = want - 0          # oracle's Z is max-shifted in place; fused path leaves Z unshifted
            got = m.var_reference(k)
            got = got - got.max(axis=1, keepdims=True) * (ds["split"] == 1)[:, None]
            if not all_rows:
                assert np.all(got[ds["split"] != 1] == 0)      # never computed: still the allocation's zeros
                got, want = got[ds["split"] == 1], want[ds["split"] == 1]
        else:
            got = m.var_reference(k)
        assert np.allclose(got, want, rtol=2e-5, atol=2e-6), k
        gw = om.var(k, True).reshape(shp)
        assert np.allclose(m.var_reference(k, True), gw, rtol=2e-4, atol=1e-7), ("grad", k)
    # weight gradients are consumed by Adam: compare the updated weights instead
    for k in (2, 5):
        assert np.allclose(m.var(k).reshape(-1), om.var(k), rtol=1e-5, atol=1e-6)
    m.close(); om.close()


def test_async_epochs_are_deterministic():
    """run_epochs (no host sync between epochs) == stepwise calls, and two runs are bit-identical
    (no float atomics anywhere on the path: the determinism check doubles as the race detector)"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.make_dataset("cora-syn")
    traces = []
    for _ in range(2):
        m = HipGCNModel(ds, seed=11, hidden_dim=16, dropout=0.5, epochs=25)
        traces.append(m.run_epochs(25))
        w = m.var(2)
        m.close()
    assert np.array_equal(traces[0].view(np.uint32), traces[1].view(np.uint32))
    m = HipGCNModel(ds, seed=11, hidden_dim=16, dropout=0.5, epochs=25)
    step = np.array([m.train_epoch() + m.eval(2) for _ in range(25)], np.float32)
    assert np.array_equal(step.view(np.uint32), traces[0].view(np.uint32))
    assert np.array_equal(m.var(2), w)
    m.close()


def test_device_rng_dropout_learns(oracle):
    """with the GPU's own counter-based dropout stream the run is statistically equivalent:
    final validation accuracy within 0.03 of the CPU path's mean over seeds"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.make_dataset("pubmed-syn")
    accs_o, accs_g = [], []
    for seed in (1, 2, 3):
        tr, _, om = oracle_trace(oracle, ds, seed, 20, hidden_dim=16, dropout=0.5)
        accs_o.append(tr[-1, 3]); om.close()
        m = HipGCNModel(ds, seed=seed, hidden_dim=16, dropout=0.5, epochs=20)
        g = m.run_epochs(20)
        accs_g.append(g[-1, 3])
        assert g[-1, 0] < g[0, 0]                 # training loss goes down
        m.close()
    assert abs(np.mean(accs_o) - np.mean(accs_g)) <= 0.03, (accs_o, accs_g)


def test_reddit_shape_dense_path_small(oracle):
    """a 1/50-scale Reddit shape: dense 602-column X (MFMA path), hidden 128, 41 classes, hub rows"""
    from cuda_gcn_amd.model import HipGCNModel, HOST_MASKS
    rng = np.random.default_rng(4)
    N, F, C = 4000, 602, 41
    w = np.arange(1, N + 1, dtype=np.float64) ** (-1 / 1.3)
    lo, hi = datagen._sample_edges(rng, N, 60000, w)
    gp, gi = datagen.csr_with_self_loops(lo, hi, N)
    assert np.diff(gp).max() > 1024               # exercises the split-row path
    label = rng.integers(0, C, N).astype(np.int32); label[:C] = np.arange(C)
    x = rng.standard_normal((N, F)).astype(np.float32)
    x[np.arange(N), label] += 1.5
    split = rng.integers(1, 4, N).astype(np.int32)
    ds = dict(num_nodes=N, input_dim=F, output_dim=C, g_indptr=gp, g_indices=gi,
              f_indptr=(np.arange(N + 1) * F).astype(np.int32), f_indices=np.tile(np.arange(F, dtype=np.int32), N),
              f_val=x.reshape(-1), split=split, label=label)
    want, _, om = oracle_trace(oracle, ds, 2, 6, hidden_dim=128, dropout=0.5)
    m = HipGCNModel(ds, seed=2, flags=HOST_MASKS, hidden_dim=128, dropout=0.5, epochs=6)
    got = np.array([m.train_epoch() + m.eval(2) for _ in range(6)], np.float32)
    check_trace(got, want, ds)
    m.close(); om.close()


def test_cli_gcn_hip_matches_gcn_seq():
    """`gcn-hip <dataset>` beside `gcn-seq <dataset>`: same command line, same output lines"""
    ds = datagen.make_dataset("tiny-syn")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "gcn-seq"], check=True)
    with tempfile.TemporaryDirectory() as td:
        datagen.write_text(ds, os.path.join(td, "data"), "tiny-syn")
        env = dict(os.environ, GCN_SEED="7")
        args = ["tiny-syn", "-", "-", "16", "-", "0", "-", "-", "30"]      # dropout 0, 30 epochs
        a = subprocess.run([os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")] + args, cwd=td, env=env, capture_output=True, text=True)
        b = subprocess.run([os.path.join(ROOT, "oracle", "gcn-seq")] + args, cwd=td, env=env, capture_output=True, text=True)
    assert a.returncode == 0, a.stderr
    assert b.returncode == 0, b.stderr
    la, lb = a.stdout.strip().splitlines(), b.stdout.strip().splitlines()
    assert "RUNNING ON GPU" in la and "RUNNING ON CPU" in lb
    ea = [l for l in la if l.startswith("epoch=")]
    eb = [l for l in lb if l.startswith("epoch=")]
    assert len(ea) == len(eb) == 30

    def fields(line):
        return {k: float(v) for k, v in (t.split("=") for t in line.split())}
    for x, y in zip(ea, eb):
        fx, fy = fields(x), fields(y)
        assert fx["epoch"] == fy["epoch"]
        assert abs(fx["train_loss"] - fy["train_loss"]) <= 2e-3 and abs(fx["val_loss"] - fy["val_loss"]) <= 2e-3
    assert any(l.startswith("total training time=") for l in la)
    assert any(l.startswith("test_loss=") for l in la)
    # a missing dataset fails the same way (src/main.cpp:33-36)
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip"), "nothing"], cwd=td, capture_output=True, text=True)
    assert r.returncode != 0 and "Cannot read input: nothing" in r.stderr


def test_rccl_selftest():
    """the RCCL the process loaded initialises and runs one-rank collectives on this GPU
    (the N > 1 bench relies on the same calls)"""
    from cuda_gcn_amd import _lib
    lib = _lib.gcnhost()
    rc = lib.gcnhost_rccl_selftest(0)
    assert rc == 0, lib.gcnhost_last_error()


def test_eval_lane_is_bit_identical():
    """validation on a second stream, overlapped with the next training epoch: same numbers as the
    sequential schedule (the lane only reorders independent work), eager and via run()"""
    from cuda_gcn_amd.model import HipGCNModel, EVAL_LANE, NO_GRAPH
    ds = datagen.make_dataset("pubmed-syn")
    a = HipGCNModel(ds, seed=6, flags=NO_GRAPH, hidden_dim=16, dropout=0.5, epochs=30)
    b = HipGCNModel(ds, seed=6, flags=EVAL_LANE, hidden_dim=16, dropout=0.5, epochs=30)
    ta, tb = a.run_epochs(12), b.run_epochs(12)
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32))
    # stepwise calls in between (train only, then a direct eval), then the zipped schedule again: the lane's
    # ring row must follow the epoch it evaluates, not its own call count
    for m in (a, b):
        for _ in range(3):
            m.train_epoch()
    assert a.eval(2) == b.eval(2)
    ta, tb = a.run_epochs(15), b.run_epochs(15)
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32))
    ta, tb = a.run_epochs(1), b.run_epochs(1)
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32))
    assert a.eval(3) == b.eval(3)
    assert np.array_equal(a.var(2), b.var(2))
    a.close(); b.close()


@pytest.mark.parametrize("name,hidden", [("cora-syn", 16), ("reddit-mini", 128)])
def test_scored_rows_only_is_bit_identical_to_all_rows(name, hidden):
    """skipping the rows of the logits that no split reads changes no reported number and no weight"""
    from cuda_gcn_amd.model import HipGCNModel, ALL_ROWS
    ds = datagen.make_dataset(name)
    a = HipGCNModel(ds, seed=8, flags=ALL_ROWS, hidden_dim=hidden, dropout=0.5, epochs=12)
    b = HipGCNModel(ds, seed=8, hidden_dim=hidden, dropout=0.5, epochs=12)
    ta, tb = a.run_epochs(10), b.run_epochs(10)
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32))
    assert a.train_epoch() == b.train_epoch()
    for s in (2, 3, 1):
        assert a.eval(s) == b.eval(s)
    assert np.array_equal(a.var(2), b.var(2)) and np.array_equal(a.var(5), b.var(5))
    za, zb = a.var(6), b.var(6)                              # after eval(1): rows of the training split
    assert np.array_equal(za[ds["split"] == 1], zb[ds["split"] == 1])
    a.close(); b.close()


@pytest.mark.parametrize("name,hidden", [("reddit-mini", 128), ("rmat-10-32", 16)])
def test_aggregate_first_eval_matches_reference_order(name, hidden):
    """dense X: evaluation forwards run ReLU((A^.X).W1) with A^.X built once; the reference's order
    ReLU(A^.(X.W1)) (NO_AGG_FIRST_EVAL) gives the same losses to rounding and the same training (training never
    uses the aggregated features)"""
    from cuda_gcn_amd.model import HipGCNModel, NO_AGG_FIRST_EVAL
    ds = datagen.make_dataset(name)
    a = HipGCNModel(ds, seed=8, flags=NO_AGG_FIRST_EVAL, hidden_dim=hidden, dropout=0.5, epochs=12)
    b = HipGCNModel(ds, seed=8, hidden_dim=hidden, dropout=0.5, epochs=12)
    ta, tb = a.run_epochs(10), b.run_epochs(10)
    assert np.array_equal(ta[:, :2].view(np.uint32), tb[:, :2].view(np.uint32))       # training: bit-identical
    assert np.abs(ta[:, 2] - tb[:, 2]).max() <= 2e-5                                   # validation loss
    for s in (1, 2, 3):
        n_s = int((ds["split"] == s).sum())
        la, lb = a.eval(s), b.eval(s)
        assert abs(la[0] - lb[0]) <= 2e-5 and abs(la[1] - lb[1]) <= 1.0 / n_s + 1e-7, (s, la, lb)
    ha, hb = a.var(3), b.var(3)                                                        # H1 of the last evaluation
    assert np.allclose(ha, hb, rtol=1e-4, atol=1e-5 * max(1.0, float(np.abs(ha).max())))
    assert np.array_equal(a.var(2), b.var(2))
    a.close(); b.close()


@pytest.mark.parametrize("name,hidden", [("reddit-mini", 128), ("cora-syn", 16)])
def test_restricted_backward_operator_matches_masked_launch(name, hidden):
    """the output layer's backward through the operator that has lost the edges pointing outside the training split
    (default) against masking those rows at every launch (MASKED_BWD): the same sums up to the order of their terms"""
    from cuda_gcn_amd.model import HipGCNModel, MASKED_BWD
    ds = datagen.make_dataset(name)
    a = HipGCNModel(ds, seed=8, hidden_dim=hidden, dropout=0.5, epochs=12)
    b = HipGCNModel(ds, seed=8, flags=MASKED_BWD, hidden_dim=hidden, dropout=0.5, epochs=12)
    la, lb = a.train_epoch(), b.train_epoch()
    assert la == lb                                            # the first forward does not depend on it
    ga, gb = a.var(4, True), b.var(4, True)                    # dZ0 = A^ . dZ after one backward
    assert np.allclose(ga, gb, rtol=1e-4, atol=1e-5 * float(np.abs(gb).max()))
    ta, tb = a.run_epochs(10), b.run_epochs(10)
    assert np.allclose(ta, tb, rtol=2e-4, atol=2e-5)
    a.close(); b.close()


@pytest.mark.parametrize("name,hidden,flags", [("cora-syn", 16, 0), ("pubmed-syn", 16, 0), ("reddit-mini", 128, 0), ("reddit-mini", 128, 16),
                                               ("reddit-mini", 128, 8192 | 4096), ("rmat-12-32", 16, 0)])
def test_factored_aggregation_matches_per_edge_coefficients(name, hidden, flags):
    """the default factored operator dinv[r] * sum(dinv[c] * x[c]) against the reference's per-edge coefficients (EDGE_COEF):
    same real numbers, two more f32 roundings per term — traces to 2e-5, every variable (scaled back) and the weights after 10
    epochs to the summation-order tolerance; with the validation lane (16), in the reference's evaluation order on all rows"""
    from cuda_gcn_amd.model import HipGCNModel, EDGE_COEF
    ds = datagen.make_dataset(name)
    a = HipGCNModel(ds, seed=8, flags=flags | EDGE_COEF, hidden_dim=hidden, dropout=0.5, epochs=12)
    b = HipGCNModel(ds, seed=8, flags=flags, hidden_dim=hidden, dropout=0.5, epochs=12)
    assert b.row_scale()[1] and not a.row_scale()[1]
    la, lb = a.train_epoch(), b.train_epoch()
    assert abs(la[0] - lb[0]) <= 2e-6 and la[1] == lb[1]
    for k in (1, 3, 4):
        x, y = a.var(k), b.var_reference(k)
        assert np.allclose(x, y, rtol=2e-5, atol=2e-6 * max(1.0, float(np.abs(x).max()))), k
        gx, gy = a.var(k, True), b.var_reference(k, True)
        assert np.allclose(gx, gy, rtol=2e-4, atol=2e-6 * max(1e-6, float(np.abs(gx).max()))), ("grad", k)
    ta, tb = a.run_epochs(10), b.run_epochs(10)
    assert np.abs(ta[:, [0, 2]] - tb[:, [0, 2]]).max() <= 2e-5, np.abs(ta - tb).max(axis=0)
    assert np.abs(ta[:, [1, 3]] - tb[:, [1, 3]]).max() <= 2.0 / max(1, int((ds["split"] == 2).sum())) + 1e-6
    for s in (2, 3):
        ea, eb = a.eval(s), b.eval(s)
        assert abs(ea[0] - eb[0]) <= 2e-5
    assert np.allclose(a.var(2), b.var(2), rtol=0, atol=2e-3) and np.allclose(a.var(5), b.var(5), rtol=0, atol=2e-3)
    a.close(); b.close()


def test_structure_groups_schedule_is_bit_identical():
    """labels withheld (NO_LABEL_HINT): the row groups come from the graph (modularity local moving) — another order of the
    task list, the same bits"""
    from cuda_gcn_amd.model import HipGCNModel, NO_LABEL_HINT
    ds = datagen.make_dataset("reddit-mini")
    a = HipGCNModel(ds, seed=6, flags=NO_LABEL_HINT, hidden_dim=32, dropout=0.5, epochs=4)
    b = HipGCNModel(ds, seed=6, hidden_dim=32, dropout=0.5, epochs=4)
    assert a.schedule() in ("degree", "dealt-256") or a.schedule().startswith("structure-major")
    assert b.schedule() != a.schedule() or b.schedule() in ("degree", "dealt-256")
    ta, tb = a.run_epochs(4), b.run_epochs(4)
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32))
    assert np.array_equal(a.var(2), b.var(2)) and np.array_equal(a.var(6), b.var(6))
    a.close(); b.close()


@pytest.mark.parametrize("name", ["reddit-mini-h0", "reddit-mini-h03", "reddit-mini-zipf"])
def test_structure_variants_trace_vs_oracle(oracle, name):
    """the Reddit shape WITHOUT the planted structure the headline graph has (datagen.REDDIT_VARIANTS: no label homophily,
    weak homophily, Zipf class sizes): the schedule and the slice width HipGCN picks differ from the headline's, the
    numbers do not — trace against the oracle with the reference's dropout stream replayed, in the narrow-slice form the
    rule picks and in the headline's 64-float form (8 instead of 4 partial sums per row: another summation order)"""
    from cuda_gcn_amd.model import HipGCNModel, HOST_MASKS
    ds = datagen.make_dataset(name)
    want, _, om = oracle_trace(oracle, ds, 5, 4, hidden_dim=128, dropout=0.5)
    om.close()
    m = HipGCNModel(ds, seed=5, flags=HOST_MASKS, hidden_dim=128, dropout=0.5, epochs=4)
    assert m.slice_floats() in (32, 64)
    if name.endswith("-h0"):
        assert m.slice_floats() == 32 and not m.schedule().startswith("label")
    got = np.array([m.train_epoch() + m.eval(2) for _ in range(4)], np.float32)
    check_trace(got, want, ds)
    w = m.var(2).copy()
    m.close()
    os.environ["HIPGCN_NO_SLICE_TUNING"] = "1"
    try:
        b = HipGCNModel(ds, seed=5, flags=HOST_MASKS, hidden_dim=128, dropout=0.5, epochs=4)
    finally:
        del os.environ["HIPGCN_NO_SLICE_TUNING"]
    assert b.slice_floats() == 64
    gb = np.array([b.train_epoch() + b.eval(2) for _ in range(4)], np.float32)
    check_trace(gb, want, ds)
    assert np.allclose(b.var(2), w, rtol=0, atol=1e-4)
    b.close()


@pytest.mark.parametrize("name,hidden,lane", [("reddit-mini", 128, False), ("reddit-mini", 128, True), ("cora-syn", 16, False)])
def test_loss_epilogue_is_bit_identical_to_the_loss_kernel(name, hidden, lane):
    """the loss riding in the epilogue of the class-width aggregation (default) against the loss kernel reading the stored
    logits (HIPGCN_NO_LOSS_EPILOGUE): every reported number and every weight, bit for bit"""
    from cuda_gcn_amd.model import HipGCNModel, EVAL_LANE, NO_EVAL_LANE
    ds = datagen.make_dataset(name)
    fl = EVAL_LANE if lane else NO_EVAL_LANE
    a = HipGCNModel(ds, seed=9, flags=fl, hidden_dim=hidden, dropout=0.5, epochs=8)
    os.environ["HIPGCN_NO_LOSS_EPILOGUE"] = "1"
    try:
        b = HipGCNModel(ds, seed=9, flags=fl, hidden_dim=hidden, dropout=0.5, epochs=8)
    finally:
        del os.environ["HIPGCN_NO_LOSS_EPILOGUE"]
    ta, tb = a.run_epochs(6), b.run_epochs(6)
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32))
    assert a.train_epoch() == b.train_epoch()
    for s in (2, 3, 1):
        assert a.eval(s) == b.eval(s)
    assert np.array_equal(a.var(2), b.var(2)) and np.array_equal(a.var(5), b.var(5))
    a.close(); b.close()


def test_f32_mfma_products_stay_selectable():
    """HIPGCN_GEMM=f32 (HipGCNOptions::gemm -> context option gemm_bf16x3 = 0 on the training and the lane context): the first-layer
    and class-layer products on the exact-f32 MFMA kernels of rounds 1-4.  Same real numbers as the bf16x3 default, another
    rounding: traces within 2e-5, weights within Adam's amplification of it — and not the same bits (the switch took effect)"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.make_dataset("reddit-mini")
    a = HipGCNModel(ds, seed=4, hidden_dim=128, dropout=0.5, epochs=8)
    os.environ["HIPGCN_GEMM"] = "f32"
    try:
        b = HipGCNModel(ds, seed=4, hidden_dim=128, dropout=0.5, epochs=8)
    finally:
        del os.environ["HIPGCN_GEMM"]
    ta, tb = a.run_epochs(6), b.run_epochs(6)
    assert np.abs(ta[:, [0, 2]] - tb[:, [0, 2]]).max() <= 2e-5
    assert np.abs(ta[:, [1, 3]] - tb[:, [1, 3]]).max() <= 2.0 / int((ds["split"] == 2).sum())
    assert not np.array_equal(a.var(2), b.var(2))
    # (Adam's step is lr * m / (sqrt(v) + eps): where a gradient element is ~1e-7 its rounding decides the sign of a step of ~lr,
    #  so a handful of the 77 K + 5 K weights may sit a few steps apart after eight epochs; the bulk must agree)
    for v in (2, 5):
        dw = np.abs(a.var(v).astype(np.float64) - b.var(v))
        assert np.median(dw) <= 1e-5 and np.mean(dw > 2e-3) <= 2e-3, (v, float(np.median(dw)), float(np.mean(dw > 2e-3)), float(dw.max()))
    a.close(); b.close()


@pytest.mark.parametrize("lane", [False, True])
def test_both_products_of_an_evaluation_in_one_launch(lane):
    """evaluation forwards compute Z0 = ReLU((A^.X).W1).W2 in one launch, the hidden matrix staying in accumulators (default), against
    the two launches with H1 stored (HIPGCN_NO_EVAL_FUSION): training untouched (bit-identical), evaluation losses within the
    two-roundings tolerance, accuracies within one row; and get_var(3) after a fused evaluation still returns that evaluation's
    hidden matrix (rebuilt on demand by the stored form: the bits of the unfused model)"""
    from cuda_gcn_amd.model import HipGCNModel, EVAL_LANE, NO_EVAL_LANE
    ds = datagen.make_dataset("reddit-mini")
    fl = EVAL_LANE if lane else NO_EVAL_LANE
    a = HipGCNModel(ds, seed=9, flags=fl, hidden_dim=128, dropout=0.5, epochs=8)
    os.environ["HIPGCN_NO_EVAL_FUSION"] = "1"
    try:
        b = HipGCNModel(ds, seed=9, flags=fl, hidden_dim=128, dropout=0.5, epochs=8)
    finally:
        del os.environ["HIPGCN_NO_EVAL_FUSION"]
    ta, tb = a.run_epochs(6), b.run_epochs(6)
    assert np.array_equal(ta[:, :2].view(np.uint32), tb[:, :2].view(np.uint32))
    assert np.abs(ta[:, 2] - tb[:, 2]).max() <= 2e-5     # (the same plane products in both forms: usually the same float, never far)
    for s in (2, 3, 1):
        n_s = int((ds["split"] == s).sum())
        la, lb = a.eval(s), b.eval(s)
        assert abs(la[0] - lb[0]) <= 2e-5 and abs(la[1] - lb[1]) <= 1.0 / n_s + 1e-7, (s, la, lb)
    if not lane:
        assert np.array_equal(a.var(3), b.var(3))               # H1 of eval(1), rebuilt for a; stored for b
        assert np.array_equal(a.var(3), b.var(3))               # (and again: the rebuilt matrix stays)
    assert a.train_epoch() == b.train_epoch()
    assert np.array_equal(a.var(2), b.var(2)) and np.array_equal(a.var(5), b.var(5))
    a.close(); b.close()


def test_row_groups_are_bit_identical():
    """scheduling the aggregation label by label (the default when the labels are assortative on the
    graph, as on reddit-*) changes no number"""
    from cuda_gcn_amd.model import HipGCNModel, NO_ROW_GROUPS
    ds = datagen.make_dataset("reddit-mini")
    a = HipGCNModel(ds, seed=6, flags=NO_ROW_GROUPS, hidden_dim=32, dropout=0.5, epochs=4)
    b = HipGCNModel(ds, seed=6, hidden_dim=32, dropout=0.5, epochs=4)
    ta, tb = a.run_epochs(4), b.run_epochs(4)
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32))
    assert np.array_equal(a.var(2), b.var(2)) and np.array_equal(a.var(6), b.var(6))
    a.close(); b.close()


@pytest.mark.parametrize("name,hidden,epochs", [("cora-syn", 16, 40), ("reddit-mini", 128, 10)])
def test_bf16_tables_track_the_f32_trace(oracle, name, hidden, epochs):
    """opt-in storage format (beyond the reference): GraphSum gathers bfloat16 copies of H0, Z0, dZ, dH1
    and sums in f32.  Not the parity path — the stated envelope is |dloss| <= 5e-3 and |dacc| <= 0.03
    against the f32 oracle with the same dropout decisions (measured: 1.2e-3 / 0.021 over 100 epochs)"""
    from cuda_gcn_amd.model import HipGCNModel, HOST_MASKS, BF16_TABLES
    ds = datagen.make_dataset(name)
    want, want_test, om = oracle_trace(oracle, ds, 5, epochs, hidden_dim=hidden, dropout=0.5)
    m = HipGCNModel(ds, seed=5, flags=HOST_MASKS | BF16_TABLES, hidden_dim=hidden, dropout=0.5, epochs=epochs)
    got = np.array([m.train_epoch() + m.eval(2) for _ in range(epochs)], np.float64)
    assert np.abs(got[:, [0, 2]] - want[:, [0, 2]]).max() <= 5e-3
    assert np.abs(got[:, [1, 3]] - want[:, [1, 3]]).max() <= 0.03
    t = m.eval(3)
    assert abs(t[0] - want_test[0]) <= 5e-3 and abs(t[1] - want_test[1]) <= 0.03
    assert np.abs(got - want).max() > 0          # it IS a different arithmetic: must not silently be the f32 path
    m.close(); om.close()


def _run_cli(binary, td, args, env):
    r = subprocess.run([binary] + args, cwd=td, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    ep = [dict((k, float(v)) for k, v in (t.split("=") for t in l.split())) for l in lines if l.startswith("epoch=")]
    return lines, ep


def test_cli_early_stopping_and_host_masks():
    """early stopping (gcn.cpp:141-150) and GCN_HOST_MASKS=1 (the CPU path's own dropout decisions) through
    the command line, beside gcn-seq"""
    ds = datagen.make_dataset("tiny-syn")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "gcn-seq"], check=True)
    hip = os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")
    seq = os.path.join(ROOT, "oracle", "gcn-seq")
    with tempfile.TemporaryDirectory() as td:
        datagen.write_text(ds, os.path.join(td, "data"), "tiny-syn")
        # dropout 0.5 with replayed masks: the two traces stay together
        env = dict(os.environ, GCN_SEED="11", GCN_HOST_MASKS="1")
        args = ["tiny-syn", "-", "-", "16", "-", "0.5", "-", "-", "40"]
        _, ea = _run_cli(hip, td, args, env)
        _, eb = _run_cli(seq, td, args, env)
        assert len(ea) == len(eb) == 40
        for x, y in zip(ea, eb):
            assert abs(x["train_loss"] - y["train_loss"]) <= 2e-3 and abs(x["val_loss"] - y["val_loss"]) <= 2e-3
            assert abs(x["train_acc"] - y["train_acc"]) <= 2 / 30 + 1e-6
        # early stopping window 5, dropout 0: both stop, within two epochs of each other
        env = dict(os.environ, GCN_SEED="11")
        args = ["tiny-syn", "-", "-", "16", "-", "0", "0.05", "-", "300", "5"]
        la, ea = _run_cli(hip, td, args, env)
        lb, eb = _run_cli(seq, td, args, env)
        assert any("Early stopping..." in l for l in la) and any("Early stopping..." in l for l in lb)
        assert abs(len(ea) - len(eb)) <= 2 and len(ea) < 300


def test_full_size_reddit_two_epochs_vs_oracle(oracle):
    """BASELINE configs[2] at full size (232 965 nodes, 23.4 M stored edges, 602 -> 128 -> 41): two
    training epochs + validation against the CPU oracle with the reference's dropout decisions replayed
    (about a minute: the oracle needs ~13 s per epoch)"""
    from cuda_gcn_amd.model import HipGCNModel, HOST_MASKS
    ds = datagen.make_dataset("reddit-syn")
    om = oracle.model(ds, seed_time=3, hidden_dim=128, dropout=0.5)
    m = HipGCNModel(ds, seed=3, flags=HOST_MASKS, hidden_dim=128, dropout=0.5, epochs=2)
    # a validation forward with the (identical) initial weights: every element of H1 and Z
    a, b = m.eval(2), om.eval(2)
    assert abs(a[0] - b[0]) <= 2e-5 and abs(a[1] - b[1]) <= 1e-4
    h = m.var_reference(3)
    assert np.allclose(h, om.var(3).reshape(h.shape), rtol=1e-4, atol=2e-6)
    z, zo = m.var(6), om.var(6).reshape(-1, ds["output_dim"])
    lab = ds["split"] == 2                                   # the oracle max-shifts the rows it scored, in place
    z = z - np.where(lab[:, None], z.max(axis=1, keepdims=True), 0)
    # only the scored rows of Z are computed (nobody reads the others); all rows of the aggregation at full
    # size are covered by test_graphsum_reddit_size_properties and the masked-vs-unmasked op test
    assert np.allclose(z[lab], zo[lab], rtol=1e-4, atol=5e-6)
    for e in range(2):
        got = m.train_epoch() + m.eval(2)
        want = om.train_epoch() + om.eval(2)
        assert abs(got[0] - want[0]) <= 2e-4 and abs(got[2] - want[2]) <= 2e-4, (e, got, want)
        assert abs(got[1] - want[1]) <= 2e-5 and abs(got[3] - want[3]) <= 1e-4, (e, got, want)
    # after Adam steps single weights whose gradient is ~0 may have moved by +-lr in opposite directions
    # (the first Adam step is lr * sign(g)); activations are therefore compared in bulk only
    d = np.abs(m.var_reference(3) - om.var(3).reshape(h.shape))
    assert np.median(d) <= 1e-6 and d.max() <= 5e-3, (np.median(d), d.max())
    m.close(); om.close()


def test_full_size_reddit_headline_schedule_repeats_itself():
    """The headline configuration as bench.py runs it (device dropout stream, validation lane on its own stream, every default):
    30 asynchronous epochs at full size, twice — every reported number and both weight matrices bit for bit.  No float atomics
    are on the path, so a difference is a race; the hand-counted asm loads of the bf16x3 kernels misbehaved
    ONLY at this size with the lane co-running, never on the small graphs of the other repeatability tests."""
    from cuda_gcn_amd.model import HipGCNModel, EVAL_LANE
    ds = datagen.make_dataset("reddit-syn")
    runs = []
    for _ in range(2):
        m = HipGCNModel(ds, seed=5, flags=EVAL_LANE, hidden_dim=128, dropout=0.5, epochs=30)
        tr = m.run_epochs(30)
        runs.append((tr, m.var(2), m.var(5), m.eval(3)))
        m.close()
    (ta, w1a, w2a, ea), (tb, w1b, w2b, eb) = runs
    assert np.isfinite(ta).all() and ta[-1, 0] < ta[0, 0]
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32))
    assert np.array_equal(w1a, w1b) and np.array_equal(w2a, w2b) and ea == eb

