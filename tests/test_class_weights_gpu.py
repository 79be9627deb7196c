"""Class-weighted training on the GPU: gcnhip_wxent_fwd_rows / gcnhip_wbce_fwd_rows against numpy float64 and, with unit
weights, against the unweighted kernels bit for bit; a weighted model's first epoch against the same reference and its
10-epoch trace against a torch-CPU float64 GCN (cross_entropy(weight=), binary_cross_entropy_with_logits(pos_weight=)); the
new constructor without weights against the old one; evaluate / predict between epochs, the captured graph and the validation
lane; two ranks; what the weights are for (macro-recall on an imbalanced graph); gcn-hip with GCN_CLASS_WEIGHTS."""
import ctypes as C
import faulthandler
import os
import signal
import socket
import subprocess
import sys

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import class_weights_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")
TEST_LIMIT_S = 180


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


def flag(names):
    from cuda_gcn_amd import model as M
    f = 0
    for k in names.split("|") if names else []:
        f |= getattr(M, k)
    return f


def special_logits(rng, n, c):
    z = (rng.standard_normal((n, c)) * 4).astype(np.float32)
    special = np.array([30, -30, 100, -100, 1e30, -1e30], np.float32)
    idx = rng.integers(0, n * c, 60)
    z.reshape(-1)[idx] = special[np.arange(60) % 6]
    return z


def row_lists(rng, n):
    return (np.arange(n, dtype=np.int32), np.sort(rng.choice(n, n // 3, replace=False)).astype(np.int32), np.array([n // 2], np.int32))


def draw_weights(rng, c):
    w = rng.uniform(0.1, 10, c).astype(np.float32)
    w[int(rng.integers(0, c))] = 0.0
    return w


def wxent_grad_close(got, want, rows, truth, w, weight_sum, scale, rtol, atol):
    """|got - want| <= rtol |want| + atol everywhere, plus, on the true class's entry of a row, 4 ulp(1) . w[t] / weight_sum
    [. scale]: that entry is w (p_t - 1) / weight_sum, and the float32 p_t = exp(z_t - max) / sum carries a few ulp of ITS OWN
    size (expf and the division), which the exact subtraction p_t - 1 leaves as an absolute error of up to ~3 x 2^-24 however
    small 1 - p_t is — the unweighted kernel's form, kept because unit weights must reproduce its bits."""
    t = np.asarray(truth)[rows]
    extra = np.zeros_like(want[rows])
    e = 4 * 2.0 ** -24 * np.asarray(w, np.float64)[t] / weight_sum
    if scale is not None:
        e = e * np.asarray(scale, np.float64)[rows]
    extra[np.arange(rows.size), t] = e
    err = np.abs(got[rows].astype(np.float64) - want[rows])
    bound = rtol * np.abs(want[rows]) + atol + extra
    print(f"   gradient: worst |err| / bound {float(np.max(err / np.maximum(bound, 1e-300))):.3g}, "
          f"worst without the true-entry term {float(np.max(err / np.maximum(bound - extra, 1e-300))):.3g}")
    return bool(np.all(err <= bound))


# ---- 1. the kernels against numpy ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cn", [1, 7, 41, 64, 65, 121, 256])
def test_wxent_kernel_against_numpy(Cn):
    from cuda_gcn_amd.ops import Device
    dev = Device(0)
    rng = np.random.default_rng(Cn)
    n = 700
    z = special_logits(rng, n, Cn)
    truth = rng.integers(0, Cn, n).astype(np.int32)
    w = draw_weights(rng, Cn)
    if Cn == 1:
        w[0] = 2.5                                 # the only class cannot have weight 0: the weighted mean would be 0 / 0
    zero = int(np.flatnonzero(w == 0)[0]) if Cn > 1 else -1
    scale = (rng.random(n) + 0.5).astype(np.float32)
    ld = (Cn + 3) // 4 * 4
    for rows in row_lists(rng, n):
        if not w[truth[rows]].sum() > 0:
            continue                               # (the single row may carry the zero class: no weighted mean to form)
        for sc in (None, scale):
            got = dev.wxent_fwd_rows(z, truth, w, rows=rows, grad_row_scale=sc, ld=ld)
            ls, ws, g, correct, total, mag = R.wxent_reference(z, truth, w, rows, scale=sc)
            print(f"C={Cn} rows={rows.size} scale={sc is not None}: loss_sum {got['loss_sum']!r} ref {ls!r} |terms| {mag!r} wsum {got['weight_sum']!r} ref {ws!r}")
            assert (got["correct"], got["total"]) == (correct, total)
            assert got["result"][2] == correct and got["result"][3] == total
            assert np.isfinite(got["loss_sum"])
            assert abs(got["loss_sum"] - ls) <= 4e-6 * max(1.0, mag), (got["loss_sum"], ls)
            assert abs(got["weight_sum"] - ws) <= 4e-6 * max(1.0, ws)
            gg = got["grad"]
            assert np.all(np.isfinite(gg[rows]))
            outside = np.setdiff1d(np.arange(n), rows)
            assert np.all(np.isnan(gg[outside])), "rows outside the list were written"
            assert wxent_grad_close(gg, g, rows, truth, w, ws, sc, rtol=1e-5, atol=1e-12 / rows.size)
            if zero >= 0:
                zr = rows[truth[rows] == zero]
                assert np.all(gg[zr] == 0.0), "a class of weight 0 left a gradient"
            again = dev.wxent_fwd_rows(z, truth, w, rows=rows, grad_row_scale=sc, ld=ld)
            assert again["result"].tobytes() == got["result"].tobytes() and again["result_i"].tobytes() == got["result_i"].tobytes()
            assert np.array_equal(again["grad"][rows].view(np.uint32), gg[rows].view(np.uint32))
    got = dev.wxent_fwd_rows(z, truth, w, training=False, ld=ld)
    assert got["grad"] is None and got["total"] == n
    dev.close()


@pytest.mark.parametrize("Cn", [1, 7, 41, 64, 65, 121, 256])
def test_wbce_kernel_against_numpy(Cn):
    from cuda_gcn_amd.ops import Device
    dev = Device(0)
    rng = np.random.default_rng(1000 + Cn)
    n = 700
    z = special_logits(rng, n, Cn)
    y = rng.random((n, Cn)) < 0.3
    pw = draw_weights(rng, Cn)
    zero = int(np.flatnonzero(pw == 0)[0])
    scale = (rng.random(n) + 0.5).astype(np.float32)
    ld = (Cn + 3) // 4 * 4
    for rows in row_lists(rng, n):
        for sc in (None, scale):
            got = dev.wbce_fwd_rows(z, y, pw, rows=rows, grad_row_scale=sc, ld=ld)
            loss, g, tp, fp, fn, f1, mag = R.wbce_reference(z, y, pw, rows, scale=sc)
            k = rows.size * Cn
            print(f"C={Cn} rows={rows.size} scale={sc is not None}: loss_sum {got['loss_sum']!r} ref {loss * k!r} |terms| {mag * k!r}")
            assert (got["tp"], got["fp"], got["fn"], got["rows"]) == (tp, fp, fn, rows.size)
            assert got["denom"] == np.float32(k)
            assert np.isfinite(got["loss_sum"])
            assert abs(got["loss_sum"] - loss * k) <= 4e-6 * max(1.0, mag * k), (got["loss_sum"], loss * k)
            gg = got["grad"]
            assert np.all(np.isfinite(gg[rows]))
            outside = np.setdiff1d(np.arange(n), rows)
            assert np.all(np.isnan(gg[outside])), "rows outside the list were written"
            assert np.allclose(gg[rows], g[rows], rtol=1e-5, atol=1e-12 / k)
            assert np.all(gg[rows][:, zero][y[rows][:, zero]] == 0.0), "a positive of weight 0 left a gradient"
            again = dev.wbce_fwd_rows(z, y, pw, rows=rows, grad_row_scale=sc, ld=ld)
            assert np.float32(again["loss_sum"]).tobytes() == np.float32(got["loss_sum"]).tobytes()
            assert np.array_equal(again["grad"][rows].view(np.uint32), gg[rows].view(np.uint32))
    dev.close()


def test_kernels_refuse_more_than_256_classes():
    from cuda_gcn_amd.ops import Device, GcnHipError
    dev = Device(0)
    with pytest.raises(GcnHipError):
        dev.wxent_fwd_rows(np.zeros((4, 257), np.float32), np.zeros(4, np.int32), np.ones(257, np.float32))
    with pytest.raises(GcnHipError):
        dev.wbce_fwd_rows(np.zeros((4, 257), np.float32), np.zeros((4, 257), bool), np.ones(257, np.float32))
    dev.close()


# ---- 2. unit weights ---------------------------------------------------------------------------------------------------------

def xent_rows_scaled(dev, z, truth, rows, scale, ld, shift=False):
    """gcnhip_xent_fwd_rows_scaled on a NaN-filled gradient: (result f32 [4], result_i int32 [2], grad, logits)"""
    n, c = z.shape
    lb = dev.padded(z, ld)
    gb = dev.buf(np.full((n, ld), np.nan, np.float32))
    tb, rb = dev.buf(np.ascontiguousarray(truth, np.int32)), dev.buf(rows)
    sb = dev.buf(np.ascontiguousarray(scale, np.float32)) if scale is not None else None
    res, resi = dev.buf(np.zeros(4, np.float32)), dev.buf(np.zeros(2, np.int32))
    rc = dev.lib.gcnhip_xent_fwd_rows_scaled(dev.ctx, lb.ptr, ld, gb.ptr, ld, tb.ptr, rb.ptr, int(rows.size), c, 1, int(rows.size), int(shift),
                                             res.ptr, resi.ptr, sb.ptr if sb else None)
    assert rc == 0
    return res.download(), resi.download(), gb.download()[:, :c], lb.download()[:, :c]


@pytest.mark.parametrize("Cn,ld", [(7, 8), (41, 44), (64, 64), (121, 124), (41, 41), (7, 7)])
def test_unit_weights_have_the_bits_of_the_unweighted_kernel(Cn, ld):
    """every weight 1.0f: d_result, d_result_i and the gradient rows of gcnhip_wxent_fwd_rows are those of
    gcnhip_xent_fwd_rows_scaled on the same inputs, bit for bit (the lane-per-row form for aligned rows of at most 64 classes,
    the wave-per-row form otherwise; several blocks of partials)"""
    from cuda_gcn_amd.ops import Device
    dev = Device(0)
    rng = np.random.default_rng(Cn * 100 + ld)
    n = 5000
    z = (rng.standard_normal((n, Cn)) * 3).astype(np.float32)
    truth = rng.integers(0, Cn, n).astype(np.int32)
    scale = (rng.random(n) + 0.5).astype(np.float32)
    ones = np.ones(Cn, np.float32)
    for rows in row_lists(rng, n):
        for sc in (None, scale):
            for shift in (False, True):
                res, resi, g, lg = xent_rows_scaled(dev, z, truth, rows, sc, ld, shift)
                got = dev.wxent_fwd_rows(z, truth, ones, rows=rows, weight_sum=float(rows.size), grad_row_scale=sc, ld=ld, shift_in_place=shift)
                assert got["result"].tobytes() == res.tobytes(), (got["result"], res)
                assert got["result_i"].tobytes() == resi.tobytes()
                assert np.array_equal(got["grad"][rows].view(np.uint32), g[rows].view(np.uint32))
                assert np.array_equal(got["logits"].view(np.uint32), lg.view(np.uint32))
    dev.close()


@pytest.mark.parametrize("Cn", [7, 41, 64, 121])
def test_unit_pos_weight_agrees_with_the_unweighted_bce_kernel(Cn):
    from cuda_gcn_amd.ops import Device
    dev = Device(0)
    rng = np.random.default_rng(Cn)
    n = 700
    z = special_logits(rng, n, Cn)
    y = rng.random((n, Cn)) < 0.3
    ld = (Cn + 3) // 4 * 4
    for rows in row_lists(rng, n):
        a = dev.bce_fwd_rows(z, y, rows=rows, ld=ld)
        b = dev.wbce_fwd_rows(z, y, np.ones(Cn, np.float32), rows=rows, ld=ld)
        assert (a["tp"], a["fp"], a["fn"], a["rows"], a["denom"]) == (b["tp"], b["fp"], b["fn"], b["rows"], b["denom"])
        mag = R.wbce_reference(z, y, np.ones(Cn), rows)[6] * rows.size * Cn
        assert abs(a["loss_sum"] - b["loss_sum"]) <= 2 * 4e-6 * max(1.0, mag)          # each within 4e-6 of the float64 sum
        assert np.allclose(a["grad"][rows], b["grad"][rows], rtol=2e-5, atol=1e-12 / (rows.size * Cn))
    dev.close()


# ---- 3. the first epoch of a model ------------------------------------------------------------------------------------------

def small_ml(classes, seed=0):
    return datagen.planted_multilabel(n_comm=16, size=128, deg=12, feats=24, classes=classes, seed=datagen.DEFAULT_SEED + seed)


def small_sl(classes=8, seed=0):
    return datagen.planted_communities(n_comm=16, size=128, deg=12, feats=24, classes=classes, seed=datagen.DEFAULT_SEED + seed)


def l2_of(m):
    return 5e-4 * float(np.sum(m.var(2).astype(np.float64) ** 2)) / 2


@pytest.mark.parametrize("flags", ["HOST_MASKS", "HOST_MASKS|MODULAR"])
def test_first_epoch_single_label(flags):
    from cuda_gcn_amd.model import HipGCNModel
    ds = small_sl()
    rng = np.random.default_rng(3)
    w = rng.uniform(0.1, 10, 8).astype(np.float32)
    m = HipGCNModel(ds, seed=5, flags=flag(flags), hidden_dim=16, dropout=0.5, class_weights=w)
    l2 = l2_of(m)
    loss, acc = m.train_epoch()
    z, dz = m.var_reference(6), m.var_reference(6, grad=True)
    # (the modular loss shifts the stored logits in place, row - max: every quantity below is unchanged by it)
    rows = np.flatnonzero(ds["split"] == 1)
    ls, ws, g, correct, total, _ = R.wxent_reference(z, ds["label"], w, rows)
    print(f"{flags}: train loss {loss!r} ref {ls / ws + l2!r} acc {acc!r} ref {correct / total!r}")
    assert abs(loss - (ls / ws + l2)) <= 2e-6, (loss, ls / ws, l2)
    assert abs(acc - correct / total) <= 1e-6
    assert wxent_grad_close(dz, g, rows, ds["label"], w, ws, None, rtol=2e-5, atol=1e-11)
    l2 = l2_of(m)
    vl, va = m.eval(2)
    v = np.flatnonzero(ds["split"] == 2)
    ls, ws, _, correct, total, _ = R.wxent_reference(m.var_reference(6), ds["label"], w, v)      # the validation split's own weight_sum
    print(f"{flags}: val loss {vl!r} ref {ls / ws + l2!r}")
    assert abs(vl - (ls / ws + l2)) <= 2e-6 and abs(va - correct / total) <= 1e-6
    m.close()


@pytest.mark.parametrize("flags", ["HOST_MASKS", "HOST_MASKS|MODULAR"])
def test_first_epoch_multilabel(flags):
    from cuda_gcn_amd.model import HipGCNModel
    ds = small_ml(41)
    y = ds["multilabel"]
    pw = np.random.default_rng(4).uniform(0.1, 10, 41).astype(np.float32)
    m = HipGCNModel(ds, seed=5, flags=flag(flags), hidden_dim=16, dropout=0.5, multilabel=y, class_weights=pw)
    l2 = l2_of(m)
    loss, f1 = m.train_epoch()
    z, dz = m.var_reference(6), m.var_reference(6, grad=True)
    rows = np.flatnonzero(ds["split"] == 1)
    rl, g, tp, fp, fn, rf1, _ = R.wbce_reference(z, y, pw, rows)
    print(f"{flags}: train loss {loss!r} ref {rl + l2!r} f1 {f1!r} ref {rf1!r}")
    assert abs(loss - (rl + l2)) <= 2e-6, (loss, rl, l2)
    assert abs(f1 - rf1) <= 1e-6
    assert np.allclose(dz[rows], g[rows], rtol=2e-5, atol=1e-11)
    l2 = l2_of(m)
    vl, vf = m.eval(2)
    v = np.flatnonzero(ds["split"] == 2)
    rl, _, _, _, _, rf1, _ = R.wbce_reference(m.var_reference(6), y, pw, v)
    assert abs(vl - (rl + l2)) <= 2e-6 and abs(vf - rf1) <= 1e-6
    m.close()


# ---- 4. ten epochs against torch on the CPU -------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", ["HOST_MASKS", "HOST_MASKS|MODULAR"])
def test_trace_single_label_matches_torch_cpu(flags):
    from cuda_gcn_amd.model import HipGCNModel
    ds = small_sl(seed=1)
    w = np.random.default_rng(7).uniform(0.1, 10, 8).astype(np.float32)
    m = HipGCNModel(ds, seed=7, flags=flag(flags), hidden_dim=16, dropout=0.5, class_weights=w)
    got = np.array([m.train_epoch() + m.eval(2) for _ in range(10)])
    m.close()
    want = R.torch_trace(ds, 7, 16, 10, weight=w)
    print("loss diff", np.abs(got[:, [0, 2]] - want[:, [0, 2]]).max(), "acc diff", np.abs(got[:, [1, 3]] - want[:, [1, 3]]).max())
    assert np.abs(got[:, [0, 2]] - want[:, [0, 2]]).max() <= 2e-4, (got, want)
    n_tr, n_va = np.sum(ds["split"] == 1), np.sum(ds["split"] == 2)
    assert np.abs(got[:, 1] - want[:, 1]).max() <= 2 / n_tr and np.abs(got[:, 3] - want[:, 3]).max() <= 2 / n_va, (got, want)


@pytest.mark.parametrize("Cn,flags", [(41, "HOST_MASKS"), (121, "HOST_MASKS|MODULAR")])
def test_trace_multilabel_matches_torch_cpu(Cn, flags):
    from cuda_gcn_amd.model import HipGCNModel
    ds = small_ml(Cn, seed=Cn)
    y = ds["multilabel"]
    pw = np.random.default_rng(Cn).uniform(0.1, 10, Cn).astype(np.float32)
    m = HipGCNModel(ds, seed=7, flags=flag(flags), hidden_dim=16, dropout=0.5, multilabel=y, class_weights=pw)
    got = np.array([m.train_epoch() + m.eval(2) for _ in range(10)])
    m.close()
    want = R.torch_trace(ds, 7, 16, 10, weight=pw, multilabel=y)
    print("loss diff", np.abs(got[:, [0, 2]] - want[:, [0, 2]]).max(), "f1 diff", np.abs(got[:, [1, 3]] - want[:, [1, 3]]).max())
    assert np.abs(got[:, [0, 2]] - want[:, [0, 2]]).max() <= 2e-4, (got, want)
    assert np.abs(got[:, [1, 3]] - want[:, [1, 3]]).max() <= 2e-3, (got, want)


# ---- 5. unweighted stays unweighted ------------------------------------------------------------------------------------------

class _NewConstructorWithoutWeights:
    """HipGCNModel built through gcnhost_model_create_weighted with class_weights = NULL"""

    def __new__(cls, ds, seed, multilabel=None, **hyper):
        from cuda_gcn_amd import _lib, model as M
        from cuda_gcn_amd.ops import pack_multihot
        m = M.HipGCNModel.__new__(M.HipGCNModel)
        m.lib = lib = _lib.gcnhost()
        words = pack_multihot(np.asarray(multilabel) != 0) if multilabel is not None else None
        out_dim = multilabel.shape[1] if multilabel is not None else ds["output_dim"]
        m.multilabel, m.class_weights = words is not None, None
        p = M.default_params(num_nodes=ds["num_nodes"], input_dim=ds["input_dim"], output_dim=out_dim, **hyper)
        m.params = p
        i32 = lambda a: np.ascontiguousarray(a, np.int32)
        k = [i32(ds["g_indptr"]), i32(ds["g_indices"]), i32(ds["f_indptr"]), i32(ds["f_indices"]),
             np.ascontiguousarray(ds["f_val"], np.float32), i32(ds["split"]), i32(ds["label"])]
        m._ag, m._ar = C.cast(None, _lib.ALLGATHER_FN), C.cast(None, _lib.ALLREDUCE_FN)
        h = C.c_void_p()
        rc = lib.gcnhost_model_create_weighted(C.byref(h), C.byref(p), *[a.ctypes.data for a in k],
                                               words.ctypes.data if words is not None else None, None,
                                               int(seed), 0, 0, 0, 1, None, m._ag, m._ar, None)
        assert rc == 0, lib.gcnhost_last_error()
        m.h = h
        return m


@pytest.mark.parametrize("multilabel", [False, True])
def test_new_constructor_without_weights_is_the_old_model(multilabel):
    """default flags (single-label: the loss epilogue path): 5 epochs of run_epochs, bit for bit"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = small_ml(41) if multilabel else small_sl()
    y = ds["multilabel"] if multilabel else None
    old = HipGCNModel(ds, seed=9, hidden_dim=16, dropout=0.5, multilabel=y)
    a = old.run_epochs(5)
    wa = old.var(2)
    old.close()
    new = _NewConstructorWithoutWeights(ds, 9, multilabel=y, hidden_dim=16, dropout=0.5)
    b = new.run_epochs(5)
    wb = new.var(2)
    new.close()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(wa.view(np.uint32), wb.view(np.uint32))


def test_unit_weights_train_like_the_unweighted_model(monkeypatch):
    """a model with every weight 1 against the unweighted model on its loss-kernel path (HIPGCN_NO_LOSS_EPILOGUE: the same row
    lists, the same factored gradient): the same trace bit for bit — the weighted mean of ones is the plain mean"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = small_sl()
    tr = []
    for w in (None, np.ones(8, np.float32)):
        if w is None:
            monkeypatch.setenv("HIPGCN_NO_LOSS_EPILOGUE", "1")
        else:
            monkeypatch.delenv("HIPGCN_NO_LOSS_EPILOGUE")
        m = HipGCNModel(ds, seed=9, flags=flag("HOST_MASKS"), hidden_dim=16, dropout=0.5, class_weights=w)
        tr.append(np.array([m.train_epoch() + m.eval(2) for _ in range(4)], np.float32))
        m.close()
    assert np.array_equal(tr[0].view(np.uint32), tr[1].view(np.uint32)), tr


# ---- 6. state -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags,multilabel", [("HOST_MASKS", False), ("", False), ("NO_EVAL_LANE|NO_GRAPH", False), ("", True), ("HOST_MASKS|MODULAR", True)])
def test_evaluate_and_predict_between_epochs_change_nothing(flags, multilabel):
    from cuda_gcn_amd.model import HipGCNModel
    ds = small_ml(41) if multilabel else small_sl()
    y = ds["multilabel"] if multilabel else None
    runs = []
    for with_calls in (False, True):
        m = HipGCNModel(ds, seed=9, flags=flag(flags), hidden_dim=16, dropout=0.5, multilabel=y, class_weights="balanced")
        tr = [m.train_epoch() + m.eval(2) for _ in range(2)]
        if with_calls:
            rep = m.evaluate(2)
            assert rep["rows"] == int(np.sum(ds["split"] == 2))
            m.evaluate(nodes=[3, 1, 4])
            (m.predict_multilabel if multilabel else m.predict)(nodes=[5, 9])
        tr += [m.train_epoch() + m.eval(2) for _ in range(2)]
        runs.append((np.array(tr, np.float32), m.var(2), m.var(5)))
        m.close()
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("multilabel", [False, True])
def test_captured_graph_and_validation_lane_are_bit_identical(multilabel):
    """run_epochs (the captured epoch graph) = train_epoch + eval(2) one by one; EVAL_LANE on = off"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = small_ml(41) if multilabel else small_sl()
    y = ds["multilabel"] if multilabel else None
    kw = dict(seed=4, hidden_dim=16, dropout=0.5, multilabel=y, class_weights="balanced")
    m = HipGCNModel(ds, flags=flag("NO_EVAL_LANE"), **kw)
    a = m.run_epochs(6)
    m.close()
    m = HipGCNModel(ds, flags=flag("NO_EVAL_LANE"), **kw)
    b = np.array([m.train_epoch() + m.eval(2) for _ in range(6)], np.float32)
    m.close()
    m = HipGCNModel(ds, flags=flag("EVAL_LANE"), **kw)
    c = m.run_epochs(6)
    m.close()
    assert np.all(np.isfinite(a))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (a, b)
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32)), (a, c)


def test_save_load_and_predict_on_a_weighted_model(tmp_path):
    from cuda_gcn_amd.model import HipGCNModel
    ds = small_sl()
    kw = dict(seed=3, hidden_dim=16, dropout=0.5, class_weights="balanced")
    m = HipGCNModel(ds, **kw)
    m.run_epochs(5)
    pred, prob = m.predict()
    rep = m.evaluate(3)
    t = ds["split"] == 3
    assert np.array_equal(rep["confusion"], np.bincount(ds["label"][t] * 8 + pred[t], minlength=64).reshape(8, 8))
    w = str(tmp_path / "w.gcnw")
    m.save_weights(w)
    m2 = HipGCNModel(ds, **kw)
    m2.load_weights(w)
    assert np.array_equal(m2.predict()[0], pred)
    assert np.float32(m2.eval(3)[0]).tobytes() == np.float32(m.eval(3)[0]).tobytes()
    m.close()
    m2.close()


# ---- 7. two ranks ------------------------------------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("multilabel", [0, 1])
def test_two_ranks_match_one_rank(tmp_path, multilabel):
    """world 2 (host-callback transport, both ranks on GPU 0, ids kept): the 5-epoch trace within 2e-4 of one rank.  Single-label:
    every node of class 7 lies in the second half of the ids, so rank 0 owns no row of the class with the largest weight — a
    per-rank weight_sum would change the loss scale."""
    from cuda_gcn_amd.model import HipGCNModel
    from tests.mr_class_weights_worker import dataset_and_weights
    ds, y, w = dataset_and_weights(multilabel)
    one = HipGCNModel(ds, seed=11, hidden_dim=16, dropout=0.0, multilabel=y, class_weights=w)
    w0 = str(tmp_path / "w0.gcnw")
    one.save_weights(w0)
    trace = np.array([one.train_epoch() + one.eval(2) for _ in range(5)], np.float32)
    one.close()
    out = str(tmp_path / "mr.npz")
    port, world = _free_port(), 2
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mr_class_weights_worker.py"), w0, out, str(multilabel)],
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
    if not multilabel:
        assert int(got["rank0_rare_rows"]) == 0
    print("trace diff", np.abs(got["trace"] - trace).max(axis=0))
    assert np.abs(got["trace"][:, [0, 2]] - trace[:, [0, 2]]).max() <= 2e-4, (got["trace"], trace)
    assert np.abs(got["trace"][:, [1, 3]] - trace[:, [1, 3]]).max() <= 2e-3


# ---- 8. it does what it is for ------------------------------------------------------------------------------------------------

def test_balanced_weights_raise_the_macro_recall_of_an_imbalanced_graph():
    """The training split of classes 3 .. 7 of a planted graph is thinned to a twentieth (class_weights_ref.IMBALANCED).  The same
    seed is trained twice, unweighted and "balanced", and the validation macro-recall of evaluate(2) compared.  The torch-CPU
    float64 model on this dataset (40 epochs, seed 5): 0.3705 unweighted, 0.9456 balanced, a gain of 0.5751 — the GPU model's
    gain must be at least half of the gain torch shows in this very run."""
    from cuda_gcn_amd.model import HipGCNModel, balanced_class_weights
    cfg = R.IMBALANCED
    ds = R.imbalanced_planted(**cfg)
    Cn = cfg["classes"]
    w = balanced_class_weights(ds["label"], ds["split"], Cn)
    torch_rec, gpu_rec = [], []
    for weight in (None, w):
        _, pred, truth = R.torch_trace(ds, cfg["model_seed"], cfg["hidden"], cfg["epochs"], weight=weight, want_val_pred=True)
        torch_rec.append(R.macro_recall(pred, truth, Cn))
    for weight in (None, "balanced"):
        m = HipGCNModel(ds, seed=cfg["model_seed"], flags=flag("HOST_MASKS"), hidden_dim=cfg["hidden"], dropout=0.5, class_weights=weight)
        for _ in range(cfg["epochs"]):
            m.train_epoch()
        rep = m.evaluate(2)
        assert np.all(rep["support"] > 0)
        gpu_rec.append(float(np.mean(rep["recall"])))
        m.close()
    print(f"macro-recall torch unweighted {torch_rec[0]:.4f} balanced {torch_rec[1]:.4f}; gpu unweighted {gpu_rec[0]:.4f} balanced {gpu_rec[1]:.4f}")
    torch_gain, gpu_gain = torch_rec[1] - torch_rec[0], gpu_rec[1] - gpu_rec[0]
    assert torch_gain >= 0.3, torch_rec
    assert gpu_gain >= 0.5 * torch_gain, (gpu_rec, torch_rec)


# ---- 9. the command line -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("multilabel", [False, True])
def test_cli_class_weights(tmp_path, multilabel):
    """GCN_CLASS_WEIGHTS=balanced and =<file> (the same weights written out) print the same lines, in the usual format, with the
    Python model's test loss for the same seed and weights; GCN_REPORT / GCN_PREDICT / GCN_SAVE_WEIGHTS still work; a malformed
    file exits non-zero naming the line"""
    from cuda_gcn_amd.model import HipGCNModel, balanced_class_weights, write_labels
    ds = datagen.planted_multilabel(classes=41) if multilabel else R.imbalanced_planted(**R.IMBALANCED)
    Cn = ds["output_dim"]
    y = ds["multilabel"] if multilabel else None
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "planted.gcnbin"))
    extra = {}
    if multilabel:
        write_labels(str(tmp_path / "labels.txt"), y)
        extra["GCN_MULTILABEL"] = str(tmp_path / "labels.txt")
    w = balanced_class_weights(y if multilabel else ds["label"], ds["split"], Cn)
    wfile = tmp_path / "w.txt"
    wfile.write_text("".join(f"{float(x)!r}\n" for x in w.astype(np.float64)))       # float64 repr of a float32: strtof gives it back
    base = ["planted", "-", "-", "16", "-", "0.5", "-", "-", "10"]
    key = "f1" if multilabel else "acc"

    def run(ok=True, **env):
        r = subprocess.run(["timeout", "-k", "10", "90", HIP] + base, cwd=str(tmp_path),
                           env=dict(os.environ, GCN_SEED="3", GCN_HOST_MASKS="1", GCN_EVAL_LANE="0", **extra, **env), capture_output=True, text=True)
        assert (r.returncode == 0) == ok, r.stderr[-3000:]
        return r.stdout.strip().splitlines(), r.stderr

    def strip(lines):
        return [" ".join(t for t in l.split() if not t.startswith("time=")) for l in lines if l.startswith(("epoch=", "test_loss="))]
    a, _ = run(GCN_CLASS_WEIGHTS="balanced", GCN_REPORT=str(tmp_path / "rep.txt"), GCN_PREDICT=str(tmp_path / "pred.txt"),
               GCN_SAVE_WEIGHTS=str(tmp_path / "w.gcnw"))
    b, _ = run(GCN_CLASS_WEIGHTS=str(wfile))
    plain, _ = run()
    ep = [l for l in a if l.startswith("epoch=")]
    assert len(ep) == 10 and all(f" train_{key}=" in l and f" val_{key}=" in l for l in ep)
    assert a[-1].startswith("test_loss=") and f" test_{key}=" in a[-1]
    assert strip(a) == strip(b)
    assert strip(a) != strip(plain)
    for f in ("rep.txt", "pred.txt", "w.gcnw"):
        assert (tmp_path / f).stat().st_size > 0
    assert len((tmp_path / "pred.txt").read_text().splitlines()) == ds["num_nodes"]
    m = HipGCNModel(ds, seed=3, flags=flag("HOST_MASKS|NO_EVAL_LANE"), hidden_dim=16, dropout=0.5, multilabel=y, class_weights=w)
    for _ in range(10):
        m.train_epoch()
        m.eval(2)
    tl, ta = m.eval(3)
    m.close()
    cli_loss = float(a[-1].split("test_loss=")[1].split()[0])
    print("cli test_loss", cli_loss, "python", tl)
    assert abs(cli_loss - tl) <= 1e-5
    bad = tmp_path / "bad.txt"
    bad.write_text("".join("1\n" if i != 2 else "oops\n" for i in range(Cn)))
    _, err = run(ok=False, GCN_CLASS_WEIGHTS=str(bad))
    assert "line 3" in err
