"""Split conformal prediction on the GPU: the three kernels of csrc/conformal.hip against the float64 reference of
tests/conformal_ref.py within its carried bounds, the diffusion of the scores through gcnhip_graphsum_blend, the model's
conformal_fit / predict_sets / coverage against the reference on the model's own log-softmax rows, the exact identities of the
device's own threshold, no side effects on training or on predict, refusals, and the command line (GCN_CONFORMAL)."""
import math
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import calib_ref
from tests import conformal_ref as R
from tests import smooth_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")
SENTINEL = -7.5
BETAS = (0.25, 1.0, 4.0)
METHODS = {"lac": (R.LAC, 0.0, 0), "aps": (R.APS, 0.0, 0), "raps": (R.APS, 0.01, 2)}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def dev():
    from cuda_gcn_amd.ops import Device
    d = Device(0)
    yield d
    d.close()


def check_scores(dev, logp, rows, ld, beta, name):
    """the scores launch against the reference: within E, unlisted rows and padding untouched, the same bits twice, the last
    rank exactly 1 (+ its penalty); returns (S_gpu [n, C], S_ref, E)"""
    method, lam, k_reg = METHODS[name]
    n, c = logp.shape
    want, e, rank = R.scores(logp, beta, method, lam, k_reg)
    got = dev.conformal_scores(logp, beta, method, lam, k_reg, rows, ld, ld_out=c + 3, fill=SENTINEL)
    idx, inside = R.listed(n, rows)
    done = np.zeros(n, bool)
    done[idx[inside]] = True
    assert np.all(got[~done] == SENTINEL) and np.all(got[:, c:] == SENTINEL)
    err = np.abs(got[done][:, :c].astype(np.float64) - want[done])
    assert np.all(err <= e[done]), (name, beta, float((err - e[done]).max()))
    assert same_bits(got, dev.conformal_scores(logp, beta, method, lam, k_reg, rows, ld, ld_out=c + 3, fill=SENTINEL))
    if method == R.APS:
        last = np.float32(1.0) + np.float32(lam) * np.float32(max(0, c - k_reg))
        assert np.all(got[done][:, :c][rank[done] == c - 1] == last)
    return got[:, :c], want, e


def check_sets(dev, table, want, e, truth, rows, ld, thresh, exact, st=None):
    """the sets launch on the device's own table against the reference's sets at the same threshold.  exact: every entry, size
    and count must match (the caller has shown that no entry can go either way); else entries that are not ambiguous match
    and a count differs by at most the number of rows with an ambiguous entry"""
    n, c = table.shape
    st = st or R.sets(want, e, thresh, truth, rows)
    th = np.broadcast_to(np.asarray(thresh, np.float32), (c,)).copy()
    member, size, counts = dev.conformal_sets_rows(table, th, truth, rows, ld)
    if exact:
        assert np.array_equal(member, st["member"]) and np.array_equal(size, st["size"]) and np.array_equal(counts, st["counts"])
    else:
        clear = ~st["ambiguous"]
        assert np.array_equal(member[clear], st["member"][clear])
        assert np.all(np.abs(size.astype(np.int64) - st["size"]) <= st["ambiguous"].sum(axis=1))
        assert np.all(np.abs(counts - st["counts"]) <= st["amb_rows"]), (counts, st["counts"], st["amb_rows"])
    # what the launch says about itself, whatever the rounding
    idx, inside = R.listed(n, rows)
    assert np.all(size[~inside] == -1) and not member[~inside].any() and np.array_equal(size[inside], member[inside].sum(axis=1))
    assert counts[0] == inside.sum() and counts[3] == (size == 0).sum()
    assert np.array_equal(counts[4:4 + c + 1], np.bincount(size[inside], minlength=c + 1))
    assert counts[4 + c + 1:4 + 2 * c + 1].sum() == counts[1] and counts[4 + 2 * c + 1:].sum() == counts[2]
    again = dev.conformal_sets_rows(table, th, truth, rows, ld)
    assert all(same_bits(x, y) for x, y in zip((member, size, counts), again))
    only = dev.conformal_sets_rows(table, th, truth, rows, ld, bits=False, size=False)
    assert only[0] is None and only[1] is None and same_bits(only[2], counts)
    return st


def check_small(dev, logp, truth, rows, ld):
    n, c = logp.shape
    for beta in BETAS:
        for name in METHODS:
            got, want, e = check_scores(dev, logp, rows, ld, beta, name)
            ts = dev.conformal_true_scores(got, truth, rows, ld=c + 2, fill=SENTINEL)
            ref, bound = R.true_scores(want, e, truth, rows)
            idx, inside = R.listed(n, rows)
            t = np.where(inside, truth[np.clip(idx, 0, max(n - 1, 0))] if n else -1, -1)
            ok = inside & (t >= 0) & (t < c)
            assert np.all(ts[~ok] == -1.0) and same_bits(ts[ok], got[idx[ok], t[ok]])
            assert np.all(np.abs(ts.astype(np.float64) - ref) <= bound)
            for th in (0.5, 0.9):
                # No entry is ambiguous at these thresholds, except where the score IS the threshold: two classes tied for the
                # maximum have p = 1 / 2 on both sides without any rounding (expf(0) = 1, Z = 2), so 1 - p and the first
                # cumulated sum are exactly 0.5 here and there.  Everything is compared exactly.
                st = R.sets(want, e, th, truth, rows)
                amb = st["ambiguous"]
                r = np.broadcast_to(idx[:, None], amb.shape)[amb]
                assert np.all(want[r, np.nonzero(amb)[1]] == th) and (c == 2 or not amb.any()), (c, n, beta, name, th)
                assert np.all(got[r, np.nonzero(amb)[1]] == np.float32(th))
                check_sets(dev, got, want, e, truth, rows, ld, th, exact=True, st=st)


@pytest.mark.parametrize("c", [2, 41, 64])
def test_kernels_match_the_reference_on_small_shapes(dev, c):
    """n in {0, 1, 5, 17}, ld == C and C + 5, beta in {0.25, 1, 4}, lac / aps / aps with lam = 0.01, k_reg = 2; a column at -1e4, a
    tie for the maximum, truth -1 and >= C, the truth otherwise drawn from the row's softmax; a row list that is repeated,
    unsorted and outside the table; an empty list.  Sets at the fixed thresholds 0.5 and 0.9: bits, sizes and counts exact."""
    for n in (0, 1, 5, 17):
        logp, truth = R.make_case(n, c, 100 * c + n)
        for ld in (None, c + 5):
            check_small(dev, logp, truth, None, ld)
    logp, truth = R.make_case(17, c, 7)
    check_small(dev, logp, truth, [16, 3, 3, -1, 17, 0, 4, 99, 2, 1, 3], c + 1)
    check_small(dev, logp, truth, np.zeros(0, np.int32), None)
    # the tie of row 4 ranks the lower class first: class 0 is alone in its cumulated sum, class C - 1 carries the others
    got = dev.conformal_scores(logp, 1.0, R.APS)
    tied = np.flatnonzero(logp[4] == logp[4].max())
    assert tied[0] == 0 and tied[-1] == c - 1 and np.all(np.diff(got[4, tied]) > 0)
    p0 = math.exp(float(logp[4, 0])) / np.exp(logp[4].astype(np.float64)).sum()
    assert abs(float(got[4, 0]) - p0) <= 1e-5 and got[4, 0] < got[4, c - 1]
    # +inf as a threshold: the full set on every row
    member, size, counts = dev.conformal_sets_rows(got, np.full(c, np.inf, np.float32), truth)
    assert member.all() and np.all(size == c) and counts[4 + c] == 17 and counts[2] == counts[1] == 15


@pytest.mark.parametrize("rows,c,seed", [(20011, 41, 3), (4001, 64, 5), (4001, 2, 6)])
def test_kernels_past_the_block_cap(dev, rows, c, seed):
    """more rows than one pass of the grid, so the cap and the grid-stride loop both run.  (20011, 41) and (4001, 64): beta in
    {0.25, 1} x alpha in {0.1, 0.3} x all three methods; (4001, 2): lac at both alphas, aps only at 0.3; beta = 4 only with lac
    at alpha = 0.3 (peaked rows with aps and two-class aps at 0.1 put the threshold on the full-set score).  The threshold the
    sets are built with is the REFERENCE's quantile rounded to f32, so the condition — ambiguous entries are at most 1 % — is one
    on the reference alone; the device's own quantile lies within the largest bound of the scores it was taken from."""
    from cuda_gcn_amd.model import conformal_quantile
    logp, truth = R.make_case(rows, c, seed)
    alphas = {(b, m): (0.1, 0.3) for b in (0.25, 1.0) for m in METHODS}
    if c == 2:
        alphas.update({(b, m): (0.3,) for b in (0.25, 1.0) for m in ("aps", "raps")})
    alphas[4.0, "lac"] = (0.3,)
    listed = np.random.default_rng(seed).integers(-5, rows + 9, rows - 1000)
    for i, ((beta, name), some) in enumerate(alphas.items()):
        ld, sub = ((c + 7, None) if i % 2 else (None, listed))    # alternately: a stride, every row / a list with strangers
        got, want, e = check_scores(dev, logp, None, ld, beta, name)
        ts = dev.conformal_true_scores(got, truth, sub)
        ref, bound = R.true_scores(want, e, truth, sub)
        assert np.array_equal(ts < 0, ref < 0) and np.all(np.abs(ts.astype(np.float64) - ref) <= bound)
        for alpha in some:
            q_ref, k, kept = R.quantile(ref, alpha)
            fit = conformal_quantile(ts, alpha)
            assert fit["k"] == k and fit["n_cal"] == kept and math.isfinite(q_ref)
            assert abs(fit["threshold"] - q_ref) <= bound.max(), (beta, alpha, name, fit["threshold"], q_ref, bound.max())
            t = float(np.float32(q_ref))
            st = R.sets(want, e, t, truth, sub)
            print(f"rows {rows} C {c} beta {beta} alpha {alpha} {name}: q {q_ref:.6f} (device {fit['threshold']:.6f}), ambiguous entries "
                  f"{int(st['ambiguous'].sum())} in {st['amb_rows']} rows, coverage {st['counts'][2] / st['counts'][1]:.4f}")
            assert st["ambiguous"].sum() <= 0.01 * st["ambiguous"].size and st["amb_rows"] <= 0.01 * rows
            check_sets(dev, got, want, e, truth, sub, None, t, exact=False, st=st)


def test_kernel_refusals(dev):
    from cuda_gcn_amd.ops import GcnHipError
    logp, truth = R.make_case(5, 3, 0)
    for beta in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(GcnHipError, match="gcnhip_conformal_scores: beta must be finite and > 0"):
            dev.conformal_scores(logp, beta, R.LAC)
    with pytest.raises(GcnHipError, match=r"gcnhip_conformal_scores: method is 0 \(lac\) or 1 \(aps\)"):
        dev.conformal_scores(logp, 1.0, 2)
    for lam in (-0.5, float("nan")):
        with pytest.raises(GcnHipError, match="gcnhip_conformal_scores: lam must be finite and >= 0"):
            dev.conformal_scores(logp, 1.0, R.APS, lam=lam)
    with pytest.raises(GcnHipError, match="gcnhip_conformal_scores: k_reg must be >= 0"):
        dev.conformal_scores(logp, 1.0, R.APS, k_reg=-1)
    with pytest.raises(GcnHipError, match="gcnhip_conformal_scores: a row stride is below num_classes"):
        dev.conformal_scores(logp, 1.0, R.LAC, ld_out=2)
    with pytest.raises(GcnHipError, match="gcnhip_conformal_scores: without a row list n is at most n_table"):
        dev.conformal_scores(logp, 1.0, R.LAC, n=6)
    wide = np.zeros((2, 65), np.float32)
    with pytest.raises(GcnHipError, match="gcnhip_conformal_scores: 1 <= num_classes <= 64"):
        dev.conformal_scores(wide, 1.0, R.LAC)
    with pytest.raises(GcnHipError, match="gcnhip_conformal_true_scores: 1 <= num_classes <= 64"):
        dev.conformal_true_scores(wide, np.zeros(2, np.int32))
    with pytest.raises(GcnHipError, match="gcnhip_conformal_sets_rows: 1 <= num_classes <= 64"):
        dev.conformal_sets_rows(wide, np.zeros(65, np.float32), np.zeros(2, np.int32))


@pytest.mark.parametrize("c", [7, 41])
def test_diffusion_of_the_scores_through_the_blend(dev, c):
    """the table after the one blend launch is within the propagated bound of d . A^ . S + (1 - d) . S — on the irregular graph of
    the smoothing tests (an empty row, a hub of 300, repeated neighbours) —, and the sets built from it match the reference's"""
    from tests.test_smooth_gpu import irregular_graph
    indptr, indices = irregular_graph()
    g = dev.graph(indptr, indices)
    csr = g.csr()
    logp, truth = R.make_case(g.n_rows, c, 21)
    for name, d in (("lac", 0.5), ("aps", 0.25), ("raps", 1.0)):
        got, want, e = check_scores(dev, logp, None, None, 1.0, name)
        d32 = calib_ref.f32(d)
        out = dev.graphsum_blend(g, got, None, d32, calib_ref.f32(np.float32(1.0) - np.float32(d32)))[:, :c]
        ref, bound = R.diffuse(csr, want, e, d)
        err = np.abs(out.astype(np.float64) - ref)
        assert np.all(err <= bound), (name, d, float((err - bound).max()))
        ts, tb = R.true_scores(ref, bound, truth)
        q = float(np.float32(R.quantile(ts, 0.2)[0]))
        st = R.sets(ref, bound, q, truth)
        assert st["amb_rows"] <= 0.01 * g.n_rows
        check_sets(dev, out, ref, bound, truth, None, None, q, exact=False, st=st)
    g.free()


# ---- the model ----------------------------------------------------------------------------------------------------------

def trained(ds, epochs=10, **kw):
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.make_dataset(ds) if isinstance(ds, str) else ds
    m = HipGCNModel(ds, seed=5, hidden_dim=16, **dict(dict(dropout=0.5), **kw))
    m.run_epochs(epochs, want_trace=False)
    return ds, m


def reference_table(ds, logp, temperature, name, d):
    method, lam, k_reg = METHODS[name]
    beta = calib_ref.f32(np.float32(1.0) / np.float32(temperature))
    s, e, _ = R.scores(logp, beta, method, lam, k_reg)
    if d > 0:
        csr = (ds["g_indptr"], ds["g_indices"], S.edge_coef(ds["g_indptr"], ds["g_indices"]))
        s, e = R.diffuse(csr, s, e, d)
    return s, e


def check_model(m, ds, logp, temperature, name, d, alpha, per_class=False):
    """conformal_fit, predict_sets and coverage against the reference on the model's own rows; returns the fit"""
    method, lam, k_reg = METHODS[name]
    n, c = logp.shape
    every = np.arange(n, dtype=np.int32)
    label = ds["label"]
    val, test = np.flatnonzero(ds["split"] == 2), np.flatnonzero(ds["split"] == 3)
    s, e = reference_table(ds, logp, temperature, name, d)
    fit = m.conformal_fit(alpha=alpha, split=2, method="lac" if name == "lac" else "aps", lam=lam, k_reg=k_reg, diffusion=d, per_class=per_class,
                          return_scores=True)
    assert fit["temperature"] == np.float32(temperature) and fit["alpha"] == alpha and fit["per_class"] == per_class
    ts, tb = R.true_scores(s, e, label, val)
    # the scores come in the split's list order: as sorted vectors they are within the largest bound (sorting is 1-Lipschitz too)
    assert fit["scores"].size == val.size and np.array_equal(np.sort(fit["scores"]) < 0, np.sort(ts) < 0)
    assert np.all(np.abs(np.sort(fit["scores"]).astype(np.float64) - np.sort(ts)) <= tb.max())
    if per_class:
        th, k, n_cal = R.quantile_per_class(ts, label[val], c, alpha)
        assert np.array_equal(fit["n_cal"], n_cal)
        for j in range(c):
            assert (fit["thresh"][j] == th[j] == math.inf) or abs(float(fit["thresh"][j]) - th[j]) <= tb[label[val] == j].max(initial=0.0)
    else:
        q, k, kept = R.quantile(ts, alpha)
        assert np.all(fit["n_cal"] == kept) and np.all(fit["thresh"] == np.float32(fit["threshold"]))
        assert (fit["threshold"] == q == math.inf) or abs(fit["threshold"] - q) <= tb.max(), (fit["threshold"], q, tb.max())
    # the sets under the device's own threshold
    thresh = fit["thresh"].astype(np.float64)
    st = R.sets(s, e, thresh, label, every)
    assert st["ambiguous"].sum() <= 0.01 * st["ambiguous"].size
    member, size = m.predict_sets(fit, nodes=every)
    clear = ~st["ambiguous"]
    assert np.array_equal(member[clear], st["member"][clear]) and np.array_equal(size, member.sum(axis=1))
    q3 = [5, 3, 3, n - 1, 0]
    mq, sq = m.predict_sets(fit, nodes=q3)
    assert np.array_equal(mq, member[q3]) and np.array_equal(sq, size[q3])
    # coverage: the counts of the test split, and of a query
    for split, rows in ((3, test), (2, val)):
        ref = R.sets(s, e, thresh, label, rows)
        cov = m.coverage(fit, split=split)
        got = np.concatenate([[cov["rows"], cov["labelled"], cov["covered"], cov["empty"]], cov["size_hist"], cov["class_support"], cov["class_covered"]])
        assert np.all(np.abs(got - ref["counts"]) <= ref["amb_rows"]), (got, ref["counts"])
        assert cov["rows"] == rows.size and cov["labelled"] == ref["counts"][1] and np.array_equal(cov["class_support"], ref["counts"][4 + c + 1:4 + 2 * c + 1])
        assert cov["mean_size"] == pytest.approx(size[rows].mean()) and cov["coverage"] == cov["covered"] / cov["labelled"]
        assert cov["covered"] == member[rows, label[rows]].sum() and np.array_equal(cov["size_hist"], np.bincount(size[rows], minlength=c + 1))
    cq = m.coverage(fit, split=None, nodes=q3)
    assert cq["rows"] == 5 and cq["covered"] == member[q3, label[q3]].sum()
    # the exact identities of the device's own threshold on its calibration rows
    cov = m.coverage(fit, split=2)
    if per_class:
        lab_of = fit["scores"] >= 0
        assert cov["labelled"] == lab_of.sum()
        for j in range(c):
            kj = R.quantile_k(int(fit["n_cal"][j]), alpha)
            assert cov["class_support"][j] == fit["n_cal"][j] and (cov["class_covered"][j] >= kj or fit["n_cal"][j] < kj)
            if fit["n_cal"][j] < kj:
                assert fit["thresh"][j] == math.inf and cov["class_covered"][j] == fit["n_cal"][j]
    else:
        kept = fit["scores"][fit["scores"] >= 0]
        k = R.quantile_k(kept.size, alpha)
        assert cov["covered"] == (kept <= np.float32(fit["threshold"])).sum() and (cov["covered"] >= k or kept.size < k)
    return fit


def test_model_fit_sets_and_coverage_match_the_reference():
    """8 planted communities of 128 nodes after 10 epochs: lac, aps, aps with the RAPS penalty, each with and without diffusion, a
    per-class fit; under a set temperature the scores follow the scaled rows and a fit from another temperature is refused;
    predict() has the same bits before and after; d = 0 has the bits of the plain kernel on the model's rows"""
    from cuda_gcn_amd.model import GcnHostError
    from cuda_gcn_amd.ops import Device
    ds = datagen.planted_communities(n_comm=8, size=128, p_in=0.5, feats=8)
    ds, m = trained(ds)
    n, c = ds["num_nodes"], ds["output_dim"]
    every = np.arange(n, dtype=np.int32)
    before = m.predict(nodes=every, logp=True)
    logp = before[2]
    fits = {}
    for name, d, alpha, per_class in (("lac", 0.0, 0.1, False), ("aps", 0.0, 0.1, False), ("raps", 0.0, 0.2, False), ("lac", 0.5, 0.1, False),
                                      ("aps", 0.3, 0.2, False), ("aps", 1.0, 0.1, False), ("aps", 0.0, 0.2, True), ("lac", 0.5, 0.3, True)):
        fits[name, d, per_class] = check_model(m, ds, logp, 1.0, name, d, alpha, per_class)
    after = m.predict(nodes=every, logp=True)
    assert all(same_bits(x, y) for x, y in zip(before, after))
    # d = 0 launches no blend: the returned scores are the plain kernel's on these rows, bit for bit
    dev = Device(0)
    val = np.flatnonzero(ds["split"] == 2)
    table = dev.conformal_scores(logp, 1.0, R.APS)
    plain = dev.conformal_true_scores(table, ds["label"], val)
    dev.close()
    assert same_bits(np.sort(plain), np.sort(fits["aps", 0.0, False]["scores"]))
    # too few rows for this alpha: +inf, and the full set everywhere
    few = val[:5].tolist()
    inf = m.conformal_fit(alpha=0.1, split=None, nodes=few)
    assert inf["threshold"] == math.inf and np.all(inf["n_cal"] == 5)
    member, size = m.predict_sets(inf, nodes=every)
    assert member.all() and np.all(size == c)
    cov = m.coverage(inf, split=3)
    assert cov["covered"] == cov["labelled"] and cov["size_hist"][c] == cov["rows"] and cov["empty"] == 0
    # a temperature: the scores follow the scaled rows; a fit from another temperature is refused
    old = fits["aps", 0.0, False]
    m.set_temperature(2.0)
    for call in (lambda: m.predict_sets(old), lambda: m.coverage(old)):
        with pytest.raises(GcnHostError, match="conformal_sets: the fit was made at temperature 1.0"):
            call()
    new = check_model(m, ds, logp, 2.0, "aps", 0.0, 0.1)
    check_model(m, ds, logp, 2.0, "lac", 0.5, 0.1)
    assert new["temperature"] == 2.0 and not same_bits(new["scores"], old["scores"])
    m.set_temperature(1.0)
    with pytest.raises(GcnHostError, match="conformal_sets: the fit was made at temperature 2.0"):
        m.predict_sets(new)
    assert same_bits(m.conformal_fit(alpha=0.1, return_scores=True)["scores"], old["scores"])
    assert all(same_bits(x, y) for x, y in zip(before, m.predict(nodes=every, logp=True)))
    m.close()


@pytest.mark.parametrize("flags", ["0", "EVAL_LANE", "NO_GRAPH"])
def test_conformal_calls_between_epochs_change_nothing(flags):
    """two models with the same seed train in lockstep, one fitting, predicting sets and measuring coverage between epochs:
    traces, weights, test metrics and the logits of the last forward are bit-identical"""
    from cuda_gcn_amd import model as M
    f = getattr(M, flags) if flags != "0" else 0
    ds = datagen.make_dataset("cora-syn")
    a = M.HipGCNModel(ds, seed=6, flags=f, hidden_dim=16, dropout=0.5)
    b = M.HipGCNModel(ds, seed=6, flags=f, hidden_dim=16, dropout=0.5)
    ta, tb = [], []
    for e in range(3):
        ta.append(a.run_epochs(1))
        tb.append(b.run_epochs(1))
        fit = b.conformal_fit(alpha=0.1, diffusion=0.5 if e else 0.0, method="aps" if e < 2 else "lac")
        b.predict_sets(fit, nodes=[4, 4, 9])
        b.coverage(fit)
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
    """a multi-label model, 65 classes, two ranks, alpha outside (0, 1), an unknown method, lam < 0, k_reg < 0, diffusion outside
    [0, 1], a split without labelled rows, a NaN threshold: GcnHostError naming the call, from the Python front end and from
    the C entry points called directly"""
    import ctypes as C
    from cuda_gcn_amd.model import HipGCNModel, GcnHostError, _ConformalFit, _ck
    from tests.mr_threads import ThreadWorld
    ds = datagen.make_dataset("tiny-syn")
    n, c = ds["num_nodes"], ds["output_dim"]

    def direct_fit(m, alpha=0.1, method=1, lam=0.0, k_reg=0, d=0.0):
        s = _ConformalFit()
        return m.lib.gcnhost_model_conformal_fit(m.h, 2, None, 0, alpha, method, lam, k_reg, d, 0, C.addressof(s), None, 0, None)

    def direct_sets(m, **kw):
        s = _ConformalFit()
        s.method, s.alpha, s.temperature = 1, 0.1, 1.0
        for k, v in kw.items():
            setattr(s, k, v)
        cnt = np.zeros(4 + 3 * 64 + 1, np.int64)
        return m.lib.gcnhost_model_conformal_sets(m.h, C.addressof(s), 3, None, 0, None, None, cnt.ctypes.data)

    some = dict(method="aps", lam=0.0, k_reg=0, diffusion=0.0, temperature=1.0, alpha=0.1, per_class=False)
    y = np.random.default_rng(0).random((n, c)) < 0.3
    ml = HipGCNModel(ds, seed=1, hidden_dim=16, multilabel=y)
    wide = HipGCNModel(dict(ds, output_dim=65, label=(np.arange(n) % 65).astype(np.int32)), seed=1, hidden_dim=16)
    for m, msg in ((ml, "this is a multi-label model"), (wide, "at most 64 classes")):
        k = m.params.output_dim
        fit = dict(some, thresh=np.ones(k, np.float32), n_cal=np.ones(k, np.int64))
        with pytest.raises(GcnHostError, match=f"conformal_fit: {msg}"):
            m.conformal_fit()
        with pytest.raises(GcnHostError, match=f"conformal_fit: {msg}"):
            _ck(m.lib, direct_fit(m), "call")
        for call in (lambda: m.predict_sets(fit), lambda: m.coverage(fit)):
            with pytest.raises(GcnHostError, match=f"conformal_sets: {msg}"):
                call()
        with pytest.raises(GcnHostError, match=f"conformal_sets: {msg}"):
            _ck(m.lib, direct_sets(m), "call")
        m.close()
    m = HipGCNModel(ds, seed=1, hidden_dim=16)
    for alpha in (0.0, 1.0, -0.5, float("nan")):
        with pytest.raises(GcnHostError, match=r"conformal_fit: alpha must be in \(0, 1\)"):
            m.conformal_fit(alpha=alpha)
        with pytest.raises(GcnHostError, match=r"conformal_sets: alpha must be in \(0, 1\)"):
            _ck(m.lib, direct_sets(m, alpha=alpha), "call")
    with pytest.raises(GcnHostError, match="conformal_fit: the method is 'aps' or 'lac'"):
        m.conformal_fit(method="raps")
    with pytest.raises(GcnHostError, match=r"conformal_fit: the method is 0 \(lac\) or 1 \(aps\)"):
        _ck(m.lib, direct_fit(m, method=2), "call")
    with pytest.raises(GcnHostError, match="conformal_fit: lam must be finite and >= 0"):
        m.conformal_fit(lam=-0.1)
    with pytest.raises(GcnHostError, match="conformal_fit: k_reg must be >= 0"):
        m.conformal_fit(k_reg=-1)
    for d in (-0.1, 1.5, float("nan")):
        with pytest.raises(GcnHostError, match=r"conformal_fit: diffusion must be in \[0, 1\]"):
            m.conformal_fit(diffusion=d)
        with pytest.raises(GcnHostError, match=r"conformal_sets: diffusion must be in \[0, 1\]"):
            _ck(m.lib, direct_sets(m, diffusion=d), "call")
    with pytest.raises(GcnHostError, match="conformal_fit: give a split or a node query, not both"):
        m.conformal_fit(split=2, nodes=[1])
    with pytest.raises(GcnHostError, match="conformal_fit: split is 1"):
        m.conformal_fit(split=4)
    fit = m.conformal_fit(alpha=0.3)
    bad = dict(fit, thresh=np.where(np.arange(c) == 2, np.nan, fit["thresh"]).astype(np.float32))
    for call in (lambda: m.predict_sets(bad), lambda: m.coverage(bad)):
        with pytest.raises(GcnHostError, match="conformal_sets: the threshold of class 2 is NaN"):
            call()
    with pytest.raises(GcnHostError, match="conformal_sets: the fit holds 3 thresholds"):
        m.predict_sets(dict(fit, thresh=np.ones(3, np.float32)))
    with pytest.raises(GcnHostError, match="conformal_fit: the rows have no labelled rows"):
        m.conformal_fit(split=None, nodes=[])
    m.close()
    # a split without labelled rows
    empty = HipGCNModel(dict(ds, split=np.where(ds["split"] == 2, 3, ds["split"]).astype(np.int32)), seed=1, hidden_dim=16)
    with pytest.raises(GcnHostError, match="conformal_fit: split 2 has no labelled rows"):
        empty.conformal_fit()
    empty.close()
    # two logical ranks: refused on each
    tw = ThreadWorld(2)
    seen, errors = [None, None], []

    def body(rank):
        try:
            ag, ar = tw.callbacks(rank)
            r = HipGCNModel(ds, seed=4, device=0, rank=rank, world=2, host_allgather=ag, host_allreduce=ar, hidden_dim=16, dropout=0.5)
            msgs = []
            for call in (r.conformal_fit, lambda: r.coverage(fit), lambda: r.predict_sets(fit, nodes=[])):
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
        assert "conformal_fit: one rank only" in msgs[0] and "conformal_sets: one rank only" in msgs[1] and "conformal_sets: one rank only" in msgs[2]


# ---- the command line ---------------------------------------------------------------------------------------------------

def timeless(stdout):
    return re.sub(r"time=\S+", "time=*", stdout)


def test_cli_conformal(tmp_path):
    """gcn-hip cora-syn with GCN_CONFORMAL: one more line after the test line, which parses and agrees with the Python path
    (weights handed over through a weights file, 0 epochs); the file's sets are predict_sets' of the test nodes; stdout without
    GCN_CONFORMAL is the same bytes minus that line (the wall-clock fields `time=` masked: they differ between any two runs);
    refused with GCN_MULTILABEL before the GPU is touched"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.make_dataset("cora-syn")
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "cora-syn.gcnbin"))
    m = HipGCNModel(ds, seed=3, hidden_dim=16, dropout=0.5)
    m.run_epochs(6, want_trace=False)
    w = str(tmp_path / "w.gcnw")
    m.save_weights(w)
    test = np.flatnonzero(ds["split"] == 3)
    want = {}
    for method, d in (("aps", 0.0), ("lac", 0.5)):
        fit = m.conformal_fit(alpha=0.2, method=method, diffusion=d)
        want[method] = (fit, m.predict_sets(fit, nodes=test), m.coverage(fit, split=3))
    m.close()
    args = ["cora-syn", "-", "-", "16", "-", "0.5", "-", "-", "0"]
    base = dict(os.environ, GCN_SEED="3", GCN_LOAD_WEIGHTS=w)
    plain = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=base, capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr[-2000:]
    for method, d in (("aps", 0.0), ("lac", 0.5)):
        out = str(tmp_path / f"sets_{method}.txt")
        env = dict(base, GCN_CONFORMAL=out, GCN_CONFORMAL_ALPHA="0.2", GCN_CONFORMAL_METHOD=method, GCN_CONFORMAL_DIFFUSION=str(d))
        r = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.splitlines(keepends=True)
        assert lines[-2].startswith("test_loss=") and timeless("".join(lines[:-1])) == timeless(plain.stdout)
        got = re.fullmatch(r"conformal_alpha=(\S+) threshold=(\S+) cal_rows=(\d+) test_coverage=(\S+) test_mean_set_size=(\S+) test_empty=(\d+)\n", lines[-1])
        assert got, lines[-3:]
        fit, (member, size), cov = want[method]
        a, q, cal, coverage, mean, empty = got.groups()
        assert float(a) == 0.2 and abs(float(q) - fit["threshold"]) <= 1e-6 and int(cal) == fit["n_cal"][0]
        assert abs(float(coverage) - cov["coverage"]) <= 1e-5 and abs(float(mean) - cov["mean_size"]) <= 1e-4 and int(empty) == cov["empty"]
        text = open(out).read().splitlines()
        assert len(text) == test.size
        for i, line in enumerate(text):
            f = line.split()
            classes = [int(x) for x in f[2].split(",")] if len(f) > 2 else []
            assert int(f[0]) == test[i] and int(f[1]) == size[i] == len(classes) and classes == np.flatnonzero(member[i]).tolist(), (i, line)
    labels = tmp_path / "labels.txt"
    labels.write_text("".join(f"{int(c) % 3}\n" for c in ds["label"]))
    bad = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=dict(env, GCN_MULTILABEL=str(labels)),
                         capture_output=True, text=True)
    assert bad.returncode != 0 and "GCN_CONFORMAL builds the sets of a single-label model" in bad.stderr, bad.stderr[-500:]
    bad = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=dict(env, GCN_CONFORMAL_ALPHA="1.5"),
                         capture_output=True, text=True)
    assert bad.returncode != 0 and "GCN_CONFORMAL needs GCN_CONFORMAL_ALPHA in (0, 1)" in bad.stderr, bad.stderr[-500:]
