"""Label propagation and Correct & Smooth on the GPU: the blend aggregation (gcnhip_graphsum_blend) and the two row-local
kernels of smooth.hip against the float64 reference of tests/smooth_ref.py, the model's propagate / label_propagation /
correct_and_smooth against the reference recurrence within its propagated bound, their usefulness on a planted graph, no
side effects on training, refusals, and the command line (GCN_SMOOTH)."""
import os
import re
import subprocess

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import smooth_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")
SENTINEL = -7.5


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


# ---- gcnhip_graphsum_blend ----------------------------------------------------------------------------------------------

def irregular_graph(n=400):
    """400 rows: row 0 empty, row 1 one edge, row 2 64 edges, row 3 65 edges, row 4 repeated neighbours, row 5 a hub of 300
    (three segments of the split length 128: the finalize kernel), the rest 2 .. 12 random neighbours.  Nothing points at the
    empty row (its degree 0 has no coefficient)."""
    rng = np.random.default_rng(11)
    rows = [np.zeros(0, np.int64), np.array([7]), 1 + rng.permutation(n - 1)[:64], 1 + rng.permutation(n - 1)[:65],
            np.array([7, 7, 7, 9, 9, 4]), 1 + rng.permutation(n - 1)[:300]]
    for _ in range(6, n):
        rows.append(1 + rng.permutation(n - 1)[:rng.integers(2, 13)])
    indptr = np.cumsum([0] + [r.size for r in rows]).astype(np.int32)
    return indptr, np.concatenate(rows).astype(np.int32)


@pytest.fixture(scope="module")
def blend_setup():
    from cuda_gcn_amd.ops import Device
    dev = Device(0)
    indptr, indices = irregular_graph()
    g = dev.graph(indptr, indices)
    csr = g.csr()
    deg = np.diff(csr[0])
    assert np.array_equal(csr[0], indptr) and deg[0] == 0 and deg[1] == 1 and deg[2] == 64 and deg[3] == 65 and deg[5] == 300
    assert np.all(np.isfinite(csr[2])) and np.array_equal(csr[2], R.edge_coef(csr[0], csr[1]))
    yield dev, g, csr
    g.free()
    dev.close()


@pytest.mark.parametrize("dim", [1, 3, 7, 16, 29, 41, 64])
def test_blend_matches_the_one_step_reference(blend_setup, dim):
    """every lane-group width, ragged tails and the 64-column launch; three (alpha, beta, lo, hi); entrywise within
    8 eps (|alpha| sum |coef . in| + |beta . base|); padding untouched; pred = numpy.argmax of the returned rows; base == in is
    the same as a copy; two launches give the same bits"""
    dev, g, csr = blend_setup
    n = g.n_rows
    rng = np.random.default_rng(dim)
    x = (rng.standard_normal((n, dim)) * 2).astype(np.float32)
    base = (rng.standard_normal((n, dim)) * 2).astype(np.float32)
    ld = (dim + 3) // 4 * 4 + (4 if dim == 7 else 0)             # one case with a whole spare quad of padding
    for alpha, beta, lo, hi in ((0.8, 0.2, 0.0, 1.0), (1.0, 0.0, -1.0, 1.0), (0.5, 0.5, -np.inf, np.inf)):
        a32, b32 = float(np.float32(alpha)), float(np.float32(beta))
        want, bound = R.blend_step(csr, x, base, a32, b32, lo, hi)
        free, _ = R.blend_step(csr, x, base, a32, b32)
        if np.isfinite(lo):
            clamped = (free < lo) | (free > hi)
            assert clamped.any() and not clamped.all()            # some entries clamp and some do not
        out, pred = dev.graphsum_blend(g, x, base, alpha, beta, lo, hi, ld=ld, argmax=True, fill=SENTINEL)
        err = np.abs(out[:, :dim].astype(np.float64) - want)
        assert np.all(err <= bound), (dim, alpha, float((err - bound).max()))
        assert np.all(out[:, dim:] == SENTINEL)
        assert np.array_equal(pred, np.argmax(out[:, :dim], axis=1))
        again, pred2 = dev.graphsum_blend(g, x, base, alpha, beta, lo, hi, ld=ld, argmax=True, fill=SENTINEL)
        assert same_bits(out, again) and np.array_equal(pred, pred2)
        assert same_bits(out, dev.graphsum_blend(g, x, base, alpha, beta, lo, hi, ld=ld, fill=SENTINEL))     # without pred
        # the gathered table as its own base: the same device buffer, and a copy of it
        own = dev.graphsum_blend(g, x, None, alpha, beta, lo, hi, ld=ld, fill=SENTINEL)
        assert same_bits(own, dev.graphsum_blend(g, x, x.copy(), alpha, beta, lo, hi, ld=ld, fill=SENTINEL))
        want_own, bound_own = R.blend_step(csr, x, x, a32, b32, lo, hi)
        assert np.all(np.abs(own[:, :dim].astype(np.float64) - want_own) <= bound_own)
    # every row constant (clamped to one value, the empty row included): one tie of all classes, the lowest class wins
    tie, pred = dev.graphsum_blend(g, x, base, 0.8, 0.2, 0.5, 0.5, ld=ld, argmax=True)
    assert np.all(tie[:, :dim] == 0.5) and np.all(pred == 0)


def test_blend_refusals(blend_setup):
    from cuda_gcn_amd.ops import GcnHipError
    dev, g, _ = blend_setup
    x = np.zeros((g.n_rows, 8), np.float32)
    with pytest.raises(GcnHipError, match="out must not be in"):
        dev.graphsum_blend(g, x, None, 0.5, 0.5, alias_out=True)
    with pytest.raises(GcnHipError, match="dim <= 64"):
        dev.graphsum_blend(g, np.zeros((g.n_rows, 65), np.float32), None, 0.5, 0.5)
    with pytest.raises(GcnHipError, match="16-byte aligned"):
        dev.graphsum_blend(g, np.zeros((g.n_rows, 7), np.float32), None, 0.5, 0.5, ld=7)


@pytest.mark.parametrize("split_edges", [0, 16, 32])
def test_blend_and_predict_gathers_are_the_aggregation_bit_for_bit(split_edges):
    """The blend and prediction kernels gather as the plain aggregation does, so with an epilogue that changes nothing they
    give its bits.  split_edges 0: the hub is 3 segments of 128; 16: the 64-, 65- and 300-edge rows are 4, 5 and 19 segments;
    32: they are 2, 3 and 10 — the segment sum's four-wide batch runs 0 to 4 times and is followed by tails of 0, 1, 2 and 3.
    The blend with base = 0, alpha = 1, beta = 0 and no clamp is exact: 1 . s is s, 0 . 0 is +0, and s is never -0 because the
    running sum starts at +0."""
    from cuda_gcn_amd.ops import Device
    dev = Device(0)
    dev.set_option("split_edges", split_edges)
    g = dev.graph(*irregular_graph())
    n = g.n_rows
    for dim in (1, 3, 7, 16, 29, 41, 64):
        x = (np.random.default_rng(100 + dim).standard_normal((n, dim)) * 2).astype(np.float32)
        agg = {s: dev.graphsum_ex(g, x, scaling=s) for s in (0, 1)}
        blend = dev.graphsum_blend(g, x, base=np.zeros_like(x), alpha=1.0, beta=0.0, lo=-np.inf, hi=np.inf)
        assert same_bits(blend[:, :dim], agg[0]), ("blend", dim)
        for s in (0, 1):
            assert same_bits(dev.graphsum_predict(g, x=x, scaling=s)["logits"], agg[s]), ("predict", dim, s)
        t = dev.to_bf16(x)
        want = dev.graphsum_bf16(g, t, dim, ld_out=(dim + 3) // 4 * 4)
        assert same_bits(dev.graphsum_predict(g, table_bf16=t, dim=dim)["logits"], want), ("predict bf16", dim)
    g.free()
    dev.close()


# ---- smooth.hip ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [3, 41, 64])
def test_error_and_correct_rows_match_the_reference(c):
    """E_0 and sigma, then G_0, from the same inputs as the reference: exp entries within EXP_ATOL, zeros and one-hot rows exact,
    sigma within the sum bound; truth -1 or >= C contributes nothing; a zero row of E^ and a row that would scale by more than
    1000 take s = 1; two launches give the same bits"""
    from cuda_gcn_amd.ops import Device
    dev = Device(0)
    n = 301
    rng = np.random.default_rng(c)
    z = rng.standard_normal((n, c)) * 2
    logp = (z - z.max(axis=1, keepdims=True) - np.log(np.exp(z - z.max(axis=1, keepdims=True)).sum(axis=1, keepdims=True))).astype(np.float32)
    truth = rng.integers(-1, c, n).astype(np.int32)
    truth[:4] = [c, c + 5, -1, 0]
    for rows in (None, rng.permutation(n)[:120].astype(np.int32)):
        want, sigma = R.error_rows(logp, truth, rows)
        e, got = dev.cs_error_rows(logp, truth, rows, ld_e=(c + 3) // 4 * 4 + 4)
        counted = np.abs(want).sum(axis=1) > 0
        assert counted.sum() == sigma[1] and not counted[:3].any() and 0 < sigma[1] < (n if rows is None else rows.size)
        assert np.all(e[~counted] == 0) and np.all(e[:, c:] == 0)                     # the launch zeroed the NaN-filled table
        assert np.all(np.abs(e[counted][:, :c].astype(np.float64) - want[counted]) <= R.EXP_ATOL)
        assert got[1] == sigma[1]
        assert abs(float(got[0]) - sigma[0]) <= 8 * R.EPS * sigma[0] + sigma[1] * c * R.EXP_ATOL
        e2, got2 = dev.cs_error_rows(logp, truth, rows, ld_e=(c + 3) // 4 * 4 + 4)
        assert same_bits(e, e2) and same_bits(got, got2)
    # G_0 from a residual table with a zero row (s = inf) and a tiny row (s > 1000) among the unknown rows
    ld_e = (c + 3) // 4 * 4
    e_hat = np.zeros((n, ld_e), np.float32)
    e_hat[:, :c] = rng.standard_normal((n, c)) * 0.05
    unknown = np.flatnonzero((truth < 0) | (truth >= c))
    e_hat[unknown[0]] = 0
    e_hat[unknown[1], :c] *= 1e-6
    sigma = np.array([37.5, 50.0], np.float32)
    s = R.autoscale(e_hat[:, :c], sigma)
    assert s[unknown[0]] == 1 and s[unknown[1]] == 1 and np.all((s[unknown[2:]] > 0.05) & (s[unknown[2:]] < 500))          # nobody near the guard
    want = R.correct_rows(logp, e_hat[:, :c], truth, sigma)
    g0 = dev.cs_correct_rows(logp, e_hat, truth, sigma, ld_g=ld_e + 4, fill=SENTINEL)
    known = (truth >= 0) & (truth < c)
    assert np.array_equal(g0[known][:, :c], R.onehot_rows(truth, c)[known].astype(np.float32))
    assert np.all(g0[:, c:] == SENTINEL)
    tol = R.EXP_ATOL + 16 * R.EPS * s[:, None] * np.abs(e_hat[:, :c]) + 4 * R.EPS * np.abs(want)    # norm (8), two divisions, the product
    assert np.all(np.abs(g0[:, :c].astype(np.float64) - want) <= tol)
    assert same_bits(g0, dev.cs_correct_rows(logp, e_hat, truth, sigma, ld_g=ld_e + 4, fill=SENTINEL))
    # no known row at all: sigma = 0 / 0, every row takes s = 1
    none = np.full(n, -1, np.int32)
    _, s0 = dev.cs_error_rows(logp, none)
    assert s0.tolist() == [0.0, 0.0]
    g1 = dev.cs_correct_rows(logp, e_hat, none, s0)
    assert np.all(np.abs(g1[:, :c].astype(np.float64) - (np.exp(logp.astype(np.float64)) + e_hat[:, :c])) <= R.EXP_ATOL + 4 * R.EPS)
    dev.close()


# ---- the model ----------------------------------------------------------------------------------------------------------

def dataset_csr(ds):
    return ds["g_indptr"], ds["g_indices"], R.edge_coef(ds["g_indptr"], ds["g_indices"])


@pytest.mark.parametrize("name,width", [("cora-syn", 5), ("tiny-syn", 3)])
def test_model_schemes_match_the_reference_recurrence(name, width):
    """propagate (a width that is not the model's class count), label_propagation and correct_and_smooth against the float64
    recurrence within its propagated bound B_K, in dataset node order; K launches = K calls of one; pred = the reference's
    argmax on every row whose top-two margin exceeds twice its bound, and those rows are more than 0.9 of all.  The float64
    reference alone reaches (oracle-trained weights, 10 epochs): cora-syn 0.9996 (Correct & Smooth) and 0.982 (label
    propagation), tiny-syn 1.0 and 0.990."""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.make_dataset(name)
    n, c = ds["num_nodes"], ds["output_dim"]
    csr = dataset_csr(ds)
    m = HipGCNModel(ds, seed=5, hidden_dim=16, dropout=0.5)
    for _ in range(10):
        m.train_epoch()
    # the primitive
    y0 = np.random.default_rng(3).standard_normal((n, width)).astype(np.float32)
    a = float(np.float32(0.8))
    yk, pred = m.propagate(y0, 0.8, 6, clamp=(-0.5, 0.5), argmax=True)
    want, bound = R.propagate(csr, y0, a, 6, -0.5, 0.5)
    assert np.all(np.abs(yk.astype(np.float64) - want) <= bound)
    assert (np.abs(want) == 0.5).any() and (np.abs(want) < 0.5).any()
    assert np.array_equal(pred, np.argmax(yk, axis=1))
    assert same_bits(m.propagate(y0, 0.8, 0), y0)
    assert same_bits(m.propagate(y0, 0.0, 3), y0)                                     # alpha = 0: 0 . sum + 1 . y0
    free, fb = R.propagate(csr, y0, a, 3)
    assert np.all(np.abs(m.propagate(y0, 0.8, 3).astype(np.float64) - free) <= fb)  # no clamp
    # label propagation from the training split
    truth = np.where(ds["split"] == 1, ds["label"], -1)
    lp_pred, lp_y = m.label_propagation(alpha=0.9, iters=50)
    rp, ry, rb = R.label_propagation(csr, truth, c, float(np.float32(0.9)), 50)
    assert np.all(np.abs(lp_y.astype(np.float64) - ry) <= rb)
    ok = R.clear_rows(ry, rb)
    assert ok.mean() > 0.9, ok.mean()
    assert np.array_equal(lp_pred[ok], rp[ok]) and np.array_equal(lp_pred, np.argmax(lp_y, axis=1))
    both, _ = m.label_propagation(alpha=0.9, iters=50, splits=(1, 2))                  # two splits known: a merged truth
    rp2, ry2, rb2 = R.label_propagation(csr, np.where(np.isin(ds["split"], (1, 2)), ds["label"], -1), c, float(np.float32(0.9)), 50)
    ok2 = R.clear_rows(ry2, rb2)
    assert np.array_equal(both[ok2], rp2[ok2])
    # Correct & Smooth from the model's own log-softmax rows
    _, _, logp = m.predict(logp=True)
    cs_pred, g = m.correct_and_smooth()
    ref = R.correct_and_smooth(csr, logp, truth, a, 50, a, 50)
    assert np.all(np.abs(g.astype(np.float64) - ref["G"]) <= ref["B_G"]), float((np.abs(g - ref["G"]) - ref["B_G"]).max())
    ok = R.clear_rows(ref["G"], ref["B_G"])
    assert ok.mean() > 0.9, ok.mean()
    assert np.array_equal(cs_pred[ok], ref["pred"][ok]) and np.array_equal(cs_pred, np.argmax(g, axis=1))
    lean, none = m.correct_and_smooth(scores=False)
    assert none is None and np.array_equal(lean, cs_pred)
    short, gs = m.correct_and_smooth(iters_correct=2, iters_smooth=0)                  # no smoothing launch: pred from G_0
    ref0 = R.correct_and_smooth(csr, logp, truth, a, 2, a, 0)
    assert np.all(np.abs(gs.astype(np.float64) - ref0["G"]) <= ref0["B_G"]) and np.array_equal(short, np.argmax(gs, axis=1))
    m.close()


def test_k_iterations_are_k_launches():
    """propagate(y0, alpha, K) has the bits of K calls with iters = 1 chained through the host.  A call's base is ITS y0, so the
    chain is the K-step recurrence exactly when the base drops out: alpha = 1 (the launch adds 0 . y0 to the same sums)"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.make_dataset("tiny-syn")
    m = HipGCNModel(ds, seed=1, hidden_dim=16, dropout=0.5)
    y0 = np.abs(np.random.default_rng(0).standard_normal((ds["num_nodes"], 41))).astype(np.float32)
    y = y0
    for _ in range(4):
        y = m.propagate(y, 1.0, 1, clamp=(0.0, 1.0))
    assert same_bits(m.propagate(y0, 1.0, 4, clamp=(0.0, 1.0)), y)
    assert same_bits(m.propagate(y0, 0.7, 5), m.propagate(y0, 0.7, 5))
    m.close()


def test_correct_and_smooth_is_useful_on_a_planted_graph():
    """8 planted communities of 128 nodes, the model trained for 4 epochs only: in the float64 reference, run from the model's own
    log-softmax rows, Correct & Smooth lifts the test-split accuracy, and the GPU's two accuracies are within 2 / rows of the
    reference's.  Chosen with the CPU oracle's training path (same data, seed 5): 0.238 before, 1.000 after (214 test rows: a gain
    of 163 rows against a tolerance of 2)."""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.planted_communities(n_comm=8, size=128)
    m = HipGCNModel(ds, seed=5, hidden_dim=16, dropout=0.5)
    for _ in range(4):
        m.train_epoch()
    test = ds["split"] == 3
    rows = int(test.sum())
    label = ds["label"][test]
    pred, _, logp = m.predict(logp=True)
    cs_pred, _ = m.correct_and_smooth(scores=False)
    ref = R.correct_and_smooth(dataset_csr(ds), logp, np.where(ds["split"] == 1, ds["label"], -1), float(np.float32(0.8)), 50, float(np.float32(0.8)), 50)
    before_ref = float(np.mean(np.argmax(logp, axis=1)[test] == label))
    after_ref = float(np.mean(ref["pred"][test] == label))
    before, after = float(np.mean(pred[test] == label)), float(np.mean(cs_pred[test] == label))
    print(f"planted: reference {before_ref:.4f} -> {after_ref:.4f}, GPU {before:.4f} -> {after:.4f}, {rows} test rows")
    assert after_ref - before_ref > 20.0 / rows, (before_ref, after_ref)
    assert abs(before - before_ref) <= 2.0 / rows and abs(after - after_ref) <= 2.0 / rows
    m.close()


@pytest.mark.parametrize("flags", ["0", "EVAL_LANE", "NO_GRAPH"])
def test_smoothing_between_epochs_changes_nothing(flags):
    """two models with the same seed train in lockstep, one calling correct_and_smooth, label_propagation and propagate between
    epochs: traces, weights, test metrics and the logits of the last forward are bit-identical"""
    from cuda_gcn_amd import model as M
    f = getattr(M, flags) if flags != "0" else 0
    ds = datagen.make_dataset("cora-syn")
    a = M.HipGCNModel(ds, seed=6, flags=f, hidden_dim=16, dropout=0.5)
    b = M.HipGCNModel(ds, seed=6, flags=f, hidden_dim=16, dropout=0.5)
    ta, tb = [], []
    y0 = np.ones((ds["num_nodes"], 9), np.float32)
    for e in range(4):
        ta.append(a.run_epochs(1))
        tb.append(b.run_epochs(1))
        b.correct_and_smooth(iters_correct=3, iters_smooth=3)
        b.label_propagation(iters=3)
        b.propagate(y0, 0.5, 2)
    ta.append(np.array([a.train_epoch() + a.eval(2)], np.float32))
    tb.append(np.array([b.train_epoch() + b.eval(2)], np.float32))
    ta, tb = np.concatenate(ta), np.concatenate(tb)
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32)), (ta, tb)
    for k in (2, 5):
        assert same_bits(a.var(k), b.var(k)), k
    assert a.eval(3) == b.eval(3)
    assert same_bits(a.var(6), b.var(6))
    a.close()
    b.close()


def test_refusals():
    """a multi-label model, 65 classes, a bad alpha, negative iterations, a y0 of the wrong shape: ValueError from the Python
    front end, and GcnHostError with the driver's message when the C entry point is called directly"""
    from cuda_gcn_amd.model import HipGCNModel, GcnHostError, _ck
    ds = datagen.make_dataset("tiny-syn")
    n = ds["num_nodes"]
    y = np.random.default_rng(0).random((n, ds["output_dim"])) < 0.3
    ml = HipGCNModel(ds, seed=1, hidden_dim=16, multilabel=y)
    pred = np.zeros(n, np.int32)
    for what in (ml.correct_and_smooth, ml.label_propagation):
        with pytest.raises(ValueError, match="multi-label model"):
            what()
    with pytest.raises(GcnHostError, match="correct_and_smooth: this is a multi-label model"):
        _ck(ml.lib, ml.lib.gcnhost_model_correct_and_smooth(ml.h, 0.8, 1, 0.8, 1, 2, pred.ctypes.data, None), "correct_and_smooth")
    with pytest.raises(GcnHostError, match="label_propagation: this is a multi-label model"):
        _ck(ml.lib, ml.lib.gcnhost_model_label_propagation(ml.h, 0.9, 1, 2, pred.ctypes.data, None), "label_propagation")
    assert ml.propagate(np.ones((n, 2), np.float32), 0.5, 1).shape == (n, 2)           # the primitive needs no labels
    ml.close()
    wide = dict(ds, output_dim=65, label=(np.arange(n) % 65).astype(np.int32))
    m65 = HipGCNModel(wide, seed=1, hidden_dim=16)
    with pytest.raises(ValueError, match="at most 64 classes"):
        m65.correct_and_smooth()
    for call, msg in ((lambda: m65.lib.gcnhost_model_correct_and_smooth(m65.h, 0.8, 1, 0.8, 1, 2, pred.ctypes.data, None), "correct_and_smooth: at most 64 classes"),
                      (lambda: m65.lib.gcnhost_model_label_propagation(m65.h, 0.9, 1, 2, pred.ctypes.data, None), "label_propagation: at most 64 classes")):
        with pytest.raises(GcnHostError, match=msg):
            _ck(m65.lib, call(), "call")
    m65.close()
    m = HipGCNModel(ds, seed=1, hidden_dim=16)
    y0 = np.zeros((n, 3), np.float32)
    out = np.zeros_like(y0)
    with pytest.raises(ValueError, match="alpha must be in"):
        m.propagate(y0, 1.5, 1)
    with pytest.raises(ValueError, match="y0 must be"):
        m.propagate(np.zeros((n + 1, 3), np.float32), 0.5, 1)
    for alpha, iters, dim, msg in ((1.5, 1, 3, r"alpha must be in \[0, 1\]"), (float("nan"), 1, 3, r"alpha must be in \[0, 1\]"),
                                   (0.5, -1, 3, "iters must be >= 0"), (0.5, 1, 65, "1 to 64 columns"), (0.5, 1, 0, "1 to 64 columns")):
        with pytest.raises(GcnHostError, match=msg):
            _ck(m.lib, m.lib.gcnhost_model_propagate(m.h, y0.ctypes.data, dim, alpha, iters, 0.0, 1.0, out.ctypes.data, None), "propagate")
    with pytest.raises(GcnHostError, match="splits are 1"):
        _ck(m.lib, m.lib.gcnhost_model_label_propagation(m.h, 0.9, 1, 0, pred.ctypes.data, None), "label_propagation")
    m.train_epoch()                                                                     # the model is still usable
    m.close()


# ---- the command line ---------------------------------------------------------------------------------------------------

def test_cli_smooth(tmp_path):
    """gcn-hip cora-syn with GCN_SMOOTH=cs: one more line, smoothed_test_acc=, after the test line — the accuracy of the classes
    GCN_PREDICT then holds — and every other line (times aside) as in a run without the variable; lp likewise; a bad value is
    refused before the GPU is touched"""
    ds = datagen.make_dataset("cora-syn")
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "cora-syn.gcnbin"))
    args = ["cora-syn", "-", "-", "16", "-", "0.5", "-", "-", "4"]

    def run(**env):
        r = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=dict(os.environ, GCN_SEED="3", **env),
                           capture_output=True, text=True)
        lines = r.stdout.strip().splitlines()
        return r, [re.sub(r"time=\S+", "time=", l) for l in lines[lines.index("RUNNING ON GPU"):]] if "RUNNING ON GPU" in lines else []
    plain, a = run()
    assert plain.returncode == 0, plain.stderr[-2000:]
    assert a[-1].startswith("test_loss=") and not any("smoothed" in l for l in a)
    test = ds["split"] == 3
    for mode in ("cs", "lp"):
        p = str(tmp_path / f"{mode}.txt")
        r, b = run(GCN_SMOOTH=mode, GCN_PREDICT=p)
        assert r.returncode == 0, r.stderr[-2000:]
        assert b[:-1] == a and re.fullmatch(r"smoothed_test_acc=\d\.\d{5}", b[-1]), b[-3:]
        rows = np.loadtxt(p, ndmin=2)
        assert rows.shape == (ds["num_nodes"], 2) and np.array_equal(rows[:, 0], np.arange(ds["num_nodes"]))
        acc = float(np.mean(rows[test, 1].astype(np.int64) == ds["label"][test]))
        assert b[-1] == f"smoothed_test_acc={acc:.5f}"
    bad, _ = run(GCN_SMOOTH="yes")
    assert bad.returncode != 0 and "GCN_SMOOTH is cs" in bad.stderr
