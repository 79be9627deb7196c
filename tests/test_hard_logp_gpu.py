"""The row kernels behind predict()'s log-softmax rows on the hard table (softmax_ref.hard_logp: control, wide, constant, tie,
underflow and spread rows, entries down to -1.9e30) at every beta of calibrate()'s bracket: gcnhip_calib_nll_rows, _bins_rows and
_scale_rows (csrc/calib.hip), gcnhip_conformal_scores, _true_scores and _sets_rows (csrc/conformal.hip) and the beta != 1 tail of
attach_finish (csrc/attach.hip), each against the float64 references of tests/calib_ref.py, tests/conformal_ref.py and
tests/softmax_ref.py within the bounds those carry.  No tolerance is new and no expected value comes from a kernel; the
conditions on the inputs (no ambiguous row with 1 and 7 bins, at most 10 % with 15) and the f32 restatements with their four
mutants are tests/test_hard_logp_cpu.py's.

Every (C, beta) of softmax_ref.CS x BETAS = (1, 2, 5, 41, 63, 64) x (0.01, 0.25, 1, 4, 100), row strides C and C + 3, the rows
all at once, the tame rows alone (no entry below -200: the sums' bounds are then 1e-3, not the 1e23 a wide row brings) and a
list with repeats and ids outside the table.

The domain of beta (include/gcnhip_driver.h): every entry point refuses beta > GCNHIP_BETA_MAX = 8e37 — the kernels round
beta . l before they take the maximum, and above FLT_MAX / ln 64 = 8.18e37 every product of a constant row is -inf, the maximum
is -inf and s - max is NaN — and HipGCNModel.set_temperature refuses the temperatures whose f32 reciprocal is larger.
test_the_largest_accepted_beta pins a constant row of C = 41 at the limit itself.

Measured on an MI355X (measurements against the references, not inputs to any bound): 130 cases in 7.2 s of wall time run alone,
of which test_model_at_the_ends_of_the_bracket takes 5.2 s (the first model of a process; under 4.5 s inside the whole suite) and
no other case more than 0.05 s.  Worst |got - want| / bound per family: nll sum 0.267, g sum 0.014, h sum 0.006, conf 0.108,
conf_sum 0.093, scaled row 0.644, scaled prob 0.101, lac 0.250, aps 0.108, raps 0.108, attach logp 0.130, attach prob 0.064,
model logp 0.358, model prob 0.031; past the caps nll sum 0.267, g sum 0.002, h sum below 0.001, conf_sum 0.066, lac 0.197,
raps 0.099, scaled row 0.644.  Nothing left a bound, no kernel was changed.

Mutants of the kernels, each built once, run against this file and discarded (the statements tests/test_hard_logp_cpu.py removes
from its restatement): without the maximum shift in row_softmax and conformal_scores_kernel 46 cases fail — nll, scaled rows and
scores at beta = 100 from C = 5 on, the scaled rows at beta = 4 too, every bins case from C = 2 on (conf = 1 / Z needs the
largest e to be 1), both cases past the caps and test_the_largest_accepted_beta; without the `p == 0` guards every
test_nll_sums_on_hard_rows case from C = 2 on (25) and both cases past the caps; without the cum clamp
test_scores_on_hard_rows[41-4.0], [63-1.0], [63-4.0] and [64-4.0] (the full-set contract: a score above 1.0f); without the last
rank forced to 1.0f 21 cases of test_scores_on_hard_rows, every C >= 2 (the bit-for-bit check).
"""
import time

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import calib_ref
from tests import conformal_ref
from tests import softmax_ref as R
from tests.calib_ref import U

pytestmark = pytest.mark.gpu

SENTINEL = -7.5
FILL = np.uint32(0xFFC5A5A5)                       # a NaN with a payload no kernel produces
METHODS = {"lac": (conformal_ref.LAC, 0.0, 0), "aps": (conformal_ref.APS, 0.0, 0), "raps": (conformal_ref.APS, 0.01, 2)}
BETA_MAX = np.float32(8e37)
WORST = {}
T0 = [None]
CASES = [(c, beta) for c in R.CS for beta in R.BETAS]


@pytest.fixture(scope="module")
def dev():
    from cuda_gcn_amd.ops import Device
    d = Device(0)
    T0[0] = time.time()
    yield d
    print("\nworst |got - want| / bound per family: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    print(f"wall time of this file's cases: {time.time() - T0[0]:.1f} s")
    d.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def within(family, got, want, bound, what=""):
    r = R.worst(got, want, bound)
    WORST[family] = max(WORST.get(family, 0.0), float(r))
    assert r <= 1.0, f"{family} {what}: |got - want| is {r:.3f} of the bound"


def tame_rows(logp):
    return np.flatnonzero(logp.min(axis=1) >= -200.0)


def row_lists(logp):
    """every row; the tame rows; repeated, unsorted ids, some outside the table"""
    n = logp.shape[0]
    return [None, tame_rows(logp).astype(np.int32), np.array([n - 1, 3, 3, -1, n, 0, 4, n + 50, 2, 1, 3, 20, 20, 9, n - 2], np.int32)]


def per_bin(b, n_bins, key="E_conf"):
    return np.bincount(b["bin"], weights=b[key], minlength=n_bins)


# ---- calib.hip ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c,beta", CASES)
def test_nll_sums_on_hard_rows(dev, c, beta):
    """sum nll, sum g, sum h inside E_S (the sum of the rows' bounds), finite, h >= 0, the counted rows exact, the same bits twice"""
    logp, t, _ = R.hard_logp(c)
    b32 = calib_ref.f32(beta)
    tt = t.copy()
    tt[[1, 9]] = -1, c                                         # a control and a wide row are not counted
    for ld in (None, c + 3):
        for rows in row_lists(logp):
            want = calib_ref.nll_g_h(logp, tt, b32, rows)
            got = dev.calib_nll_rows(logp, tt, b32, rows, ld)
            assert np.isfinite(got).all() and got[2] >= 0, got
            assert got[3] == want["S"][3]
            for k, name in enumerate(("nll", "g", "h")):
                within(name + " sum", got[k], want["S"][k], want["E_S"][k], f"C {c} beta {beta}")
            assert same_bits(got, dev.calib_nll_rows(logp, tt, b32, rows, ld))


@pytest.mark.parametrize("c,beta", CASES)
def test_bins_on_hard_rows(dev, c, beta):
    """1 and 7 bins (no row is ambiguous): count and correct exact, conf_sum inside the bin's sum of E_conf.  15 bins: count and
    correct within amb_near, and every row that is not ambiguous, launched alone, lands in the reference's bin.  The tie and
    the constant rows predict the lowest column."""
    logp, t, kinds = R.hard_logp(c)
    b32 = calib_ref.f32(beta)
    n = logp.shape[0]
    for ld in (None, c + 3):
        for rows in row_lists(logp):
            for n_bins in (1, 7, 15):
                b = calib_ref.bins(logp, t, b32, n_bins, rows)
                count, correct, conf = dev.calib_bins_rows(logp, t, b32, n_bins, rows, ld)
                assert count.sum() == b["rows"].size and np.isfinite(conf).all()
                if n_bins < 15:
                    assert not b["ambiguous"].any()
                    assert np.array_equal(count, b["count"]) and np.array_equal(correct, b["correct"]), (n_bins, count, b["count"])
                    within("conf_sum", conf, b["conf_sum"], per_bin(b, n_bins) * (1 + 1e-9), f"C {c} beta {beta} bins {n_bins}")
                else:
                    assert np.all(np.abs(count - b["count"]) <= b["amb_near"]) and np.all(np.abs(correct - b["correct"]) <= b["amb_near"])
                    assert np.all(np.abs(conf - b["conf_sum"]) <= b["amb_near"] + b["E_conf"].sum() * (1 + 1e-9))
                again = dev.calib_bins_rows(logp, t, b32, n_bins, rows, ld)
                assert all(same_bits(x, y) for x, y in zip((count, correct, conf), again))
    b = calib_ref.bins(logp, t, b32, 15)
    for r in np.flatnonzero(~b["ambiguous"]):
        count, correct, conf = dev.calib_bins_rows(logp, t, b32, 15, [r])
        assert count.tolist() == np.bincount([b["bin"][r]], minlength=15).tolist(), (r, kinds[r], count, b["bin"][r])
        assert correct.sum() == int(b["pred"][r] == t[r])
        within("conf", conf[b["bin"][r]], b["conf"][r], b["E_conf"][r], f"C {c} beta {beta} row {r}")
    # ties: the reference's pred is the lowest of the tied columns; the kernel agrees with the label on it and on no other
    for r in [i for i, k in enumerate(kinds) if k in ("tie", "constant")]:
        tied = np.flatnonzero(logp[r] == logp[r].max())
        assert b["pred"][r] == tied[0] and (tied.size >= 2 or c == 1)
        for col in tied[:3]:
            tt = t.copy()
            tt[r] = col
            assert dev.calib_bins_rows(logp, tt, b32, 1, [r])[1].tolist() == [int(col == tied[0])], (r, col)


@pytest.mark.parametrize("c,beta", CASES)
def test_scaled_rows_on_hard_rows(dev, c, beta):
    """log_softmax(beta . l) inside E_out and its largest probability inside E_prob; in place gives the bits of out of place; rows
    not listed and the padding keep their fill"""
    logp, _, _ = R.hard_logp(c)
    b32 = calib_ref.f32(beta)
    for ld in (None, c + 3):
        for rows in row_lists(logp):
            out, e_out, prob, e_prob = calib_ref.scale(logp, b32, rows)
            o, p = dev.calib_scale_rows(logp, b32, rows, ld, ld_out=c + 3, fill=SENTINEL)
            done = ~np.isnan(prob)
            assert np.all(o[~done] == SENTINEL) and np.all(o[:, c:] == SENTINEL) and np.all(p[~done] == SENTINEL)
            within("scaled row", o[done][:, :c], out[done], e_out[done], f"C {c} beta {beta}")
            within("scaled prob", p[done], prob[done], e_prob[done], f"C {c} beta {beta}")
            assert np.all(o[done][:, :c] <= 0)
            o2, p2 = dev.calib_scale_rows(logp, b32, rows, ld, ld_out=c + 3, fill=SENTINEL)
            assert same_bits(o, o2) and same_bits(p, p2)
            if rows is None or len(set(rows.tolist())) == len(rows):
                q, pq = dev.calib_scale_rows(logp, b32, rows, ld, in_place=True, fill=SENTINEL)
                assert same_bits(q[done][:, :c], o[done][:, :c]) and same_bits(pq, p)
                assert same_bits(q[~done][:, :c], logp[~done])


# ---- conformal.hip --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c,beta", CASES)
def test_scores_on_hard_rows(dev, c, beta):
    """LAC, APS and APS with the RAPS penalty inside E; the last-ranked class is 1.0f + pen bit for bit; with lam = 0 and every
    threshold 1.0f the sets launch returns the full set on every row (conformal.hip's header); the true-class scores are the
    returned table's entries"""
    logp, t, _ = R.hard_logp(c)
    n = logp.shape[0]
    tt = t.copy()
    tt[[1, 9]] = -1, c
    one = np.ones(c, np.float32)
    for ld in (None, c + 3):
        for rows in row_lists(logp):
            idx, inside = conformal_ref.listed(n, rows)
            done = np.zeros(n, bool)
            done[idx[inside]] = True
            for name, (method, lam, k_reg) in METHODS.items():
                want, e, rank = conformal_ref.scores(logp, beta, method, lam, k_reg)
                got = dev.conformal_scores(logp, beta, method, lam, k_reg, rows, ld, ld_out=c + 3, fill=SENTINEL)
                assert np.all(got[~done] == SENTINEL) and np.all(got[:, c:] == SENTINEL)
                within(name, got[done][:, :c], want[done], e[done], f"C {c} beta {beta}")
                assert same_bits(got, dev.conformal_scores(logp, beta, method, lam, k_reg, rows, ld, ld_out=c + 3, fill=SENTINEL))
                table = got[:, :c]
                if method == conformal_ref.APS:
                    last = np.float32(1.0) + np.float32(lam) * np.float32(max(0, c - k_reg))
                    assert np.all(bits(table[done][rank[done] == c - 1]) == bits(last))
                if lam == 0:
                    assert np.all(table[done] <= np.float32(1.0))
                    member, size, counts = dev.conformal_sets_rows(table, one, tt, rows, ld)
                    assert member[inside].all() and np.all(size[inside] == c) and not member[~inside].any() and np.all(size[~inside] == -1)
                    assert counts[0] == inside.sum() and counts[4 + c] == inside.sum() and counts[1] == counts[2]
                ts = dev.conformal_true_scores(table, tt, rows, ld=c + 2, fill=SENTINEL)
                label = np.where(inside, tt[np.clip(idx, 0, n - 1)], -1)
                ok = inside & (label >= 0) & (label < c)
                assert np.all(ts[~ok] == -1.0) and same_bits(ts[ok], table[idx[ok], label[ok]])


# ---- past the block caps --------------------------------------------------------------------------------------------------

TILES = 373                                       # x 44 rows = 16 412 > 256 blocks x 64 rows (calib.hip) and 16 384 (conformal.hip)


@pytest.mark.parametrize("beta", [0.01, 100.0])
def test_kernels_past_the_block_caps(dev, beta):
    """the C = 41 table 373 times over, one launch per kernel: the sums inside the sums of the per-row bounds — with every row
    labelled, and with the rows below -200 unlabelled, whose bound is not drowned by a wide row's —; with 7 bins count and
    correct are 373 times the one-tile reference, exactly; every tile of the scores has the bits of the first"""
    c = 41
    one, t1, _ = R.hard_logp(c)
    n1 = one.shape[0]
    assert n1 * TILES >= 16400
    logp, t = np.tile(one, (TILES, 1)), np.tile(t1, TILES)
    b32 = calib_ref.f32(beta)
    tame = np.zeros(n1, bool)
    tame[tame_rows(one)] = True
    for truth1 in (t1, np.where(tame, t1, -1).astype(np.int32)):
        w = calib_ref.nll_g_h(one, truth1, b32)
        got = dev.calib_nll_rows(logp, np.tile(truth1, TILES), b32, None, c + 3)
        assert np.isfinite(got).all() and got[2] >= 0 and got[3] == TILES * w["S"][3]
        for k, name in enumerate(("nll", "g", "h")):
            within(name + " sum past the cap", got[k], TILES * w["S"][k], TILES * w["E_S"][k], f"beta {beta}")
    b = calib_ref.bins(one, t1, b32, 7)
    assert not b["ambiguous"].any()
    count, correct, conf = dev.calib_bins_rows(logp, t, b32, 7)
    assert np.array_equal(count, TILES * b["count"]) and np.array_equal(correct, TILES * b["correct"])
    within("conf_sum past the cap", conf, TILES * b["conf_sum"], TILES * per_bin(b, 7) * (1 + 1e-9), f"beta {beta}")
    for name in ("lac", "raps"):
        method, lam, k_reg = METHODS[name]
        want, e, _ = conformal_ref.scores(one, beta, method, lam, k_reg)
        got = dev.conformal_scores(logp, beta, method, lam, k_reg).reshape(TILES, n1, c)
        within(name + " past the cap", got[0], want, e, f"beta {beta}")
        assert np.all(bits(got) == bits(got[0])[None])
    out, e_out, prob, e_prob = calib_ref.scale(one, b32)
    o, p = dev.calib_scale_rows(logp, b32)
    within("scaled row past the cap", o[:n1], out, e_out, f"beta {beta}")
    assert np.all(bits(o.reshape(TILES, n1, c)) == bits(o[:n1])[None]) and np.all(bits(p.reshape(TILES, n1)) == bits(p[:n1])[None])


# ---- attach_finish ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", R.CS)
def test_attach_finish_at_the_ends_of_the_bracket(dev, c):
    """gcnhip_attach_gather with the predict epilogue at beta = 0.01 and 100 on hard_rows(c) handed over exactly (one edge of
    coefficient 1 per row, and three 600-edge rows — the four-wave form — whose other columns are zero rows): pred exact, prob and
    logp inside E_sprob / E_scaled of softmax_ref.reference(z, beta); both load paths give the same bits"""
    z, _ = R.hard_rows(c)
    n = z.shape[0]
    long_of = [9, n - 1, n // 2]
    zeros = 599
    ta = np.concatenate([z, np.zeros((zeros, c), np.float32)])
    m = n + len(long_of)
    tb = np.zeros((m, c), np.float32)
    rng = np.random.default_rng(c)
    cols = [[i] for i in range(n)] + [[i] + list(n + np.arange(zeros)) for i in long_of]
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in cols])]).astype(np.int32)
    col = np.concatenate(cols).astype(np.int32)
    coef = (rng.random(col.size) + 0.5).astype(np.float32)
    coef[ptr[:-1]] = 1.0
    zz = np.concatenate([z, z[long_of]])
    pad = (c + 3) // 4 * 4
    for beta in (0.01, 100.0):
        ref = R.reference(zz, np.zeros(m, np.int32), beta=beta)
        unaligned = None
        for ld in (c, pad):
            got = dev.attach_gather(ptr, col, coef, ta, tb, epilogue="predict", beta=beta, ld_a=ld, ld_b=ld, ld_out=ld, logp=True)
            assert np.array_equal(bits(got["z"]), bits(zz)), "the gather does not return the hard rows"
            assert np.array_equal(got["pred"], ref["pred"])
            within("attach prob", got["prob"], ref["sprob"], ref["E_sprob"], f"C {c} beta {beta}")
            within("attach logp", got["logp"], ref["scaled"], ref["E_scaled"], f"C {c} beta {beta}")
            for k in ("pred", "prob", "logp"):
                assert np.array_equal(got[k].view(np.uint32)[n:], got[k].view(np.uint32)[long_of])
            if unaligned is None:
                unaligned = got
            else:
                assert all(np.array_equal(unaligned[k].view(np.uint32), got[k].view(np.uint32)) for k in ("pred", "prob", "logp"))


# ---- the domain of beta -----------------------------------------------------------------------------------------------------

def test_the_largest_accepted_beta(dev):
    """A constant row of C = 41 (l = -ln 41) at beta = GCNHIP_BETA_MAX = 8e37: s = -2.97e38 is finite on every lane, s - max is
    exactly 0, so e_j = 1, Z = 41 and p_j = 1 / 41 are the f32 values of every other beta — g, h, conf, the scaled row and the
    scores are held to the reference's bounds AT BETA = 1 (softmax(beta . l) of a constant row does not depend on beta; the bounds
    at 8e37 carry U |s| = 1.8e31 and say nothing) and nll, where logf(41) is absorbed by the maximum, to its bound at 8e37 and to
    being finite.  One step above the limit every entry point refuses, with the limit in the message."""
    from cuda_gcn_amd.ops import GcnHipError
    c = 41
    logp = np.full((3, c), np.float32(-np.log(41.0)), np.float32)
    t = np.array([0, 40, 7], np.int32)
    big = float(BETA_MAX)
    with np.errstate(over="ignore"):
        assert np.isfinite(np.float32(big) * logp[0, 0]) and not np.isfinite(np.float32(3.4e38) * logp[0, 0])
    at1, at_max = calib_ref.nll_g_h(logp, t, 1.0), calib_ref.nll_g_h(logp, t, big)
    got = dev.calib_nll_rows(logp, t, big)
    assert np.isfinite(got).all() and got[2] >= 0 and got[3] == 3
    assert abs(got[0] - at_max["S"][0]) <= at_max["E_S"][0]
    assert abs(got[1] - at1["S"][1]) <= at1["E_S"][1] and abs(got[2] - at1["S"][2]) <= at1["E_S"][2]
    b = calib_ref.bins(logp, t, 1.0, 7)
    count, correct, conf = dev.calib_bins_rows(logp, t, big, 7)
    assert not b["ambiguous"].any() and np.array_equal(count, b["count"]) and np.array_equal(correct, b["correct"]) and correct.sum() == 1
    assert np.all(np.abs(conf - b["conf_sum"]) <= per_bin(b, 7) * (1 + 1e-9))
    out, e_out, prob, e_prob = calib_ref.scale(logp, 1.0)
    o, p = dev.calib_scale_rows(logp, big)
    assert np.all(np.abs(o.astype(np.float64) - out) <= e_out) and np.all(np.abs(p.astype(np.float64) - prob) <= e_prob)
    for name, (method, lam, k_reg) in METHODS.items():
        want, e, _ = conformal_ref.scores(logp, 1.0, method, lam, k_reg)
        s = dev.conformal_scores(logp, big, method, lam, k_reg)
        assert np.all(np.abs(s.astype(np.float64) - want) <= e), name
    # attach_finish: zero logits are a constant row; its own log-softmax row is -logf(41) on every lane
    ptr, col, coef = np.arange(4, dtype=np.int32), np.arange(3, dtype=np.int32), np.ones(3, np.float32)
    ta, tb = np.zeros((3, c), np.float32), np.zeros((3, c), np.float32)
    a = dev.attach_gather(ptr, col, coef, ta, tb, epilogue="predict", beta=big, logp=True)
    assert np.all(a["pred"] == 0)
    more = (1.01 * (c - 1) - 8) * U                          # attach_finish adds left to right: the any-order bound for calib_ref's 8 U
    assert np.all(np.abs(a["logp"].astype(np.float64) - out) <= e_out + more) and np.all(np.abs(a["prob"] - prob) <= e_prob + prob * 1.01 * more)
    above = float(np.nextafter(BETA_MAX, np.float32(np.inf)))
    limit = "beta must be finite and > 0, and at most 8e37"
    for bad in (above, 3.4e38, float("inf")):
        for entry, call in (("gcnhip_calib_nll_rows", lambda: dev.calib_nll_rows(logp, t, bad)),
                            ("gcnhip_calib_bins_rows", lambda: dev.calib_bins_rows(logp, t, bad, 7)),
                            ("gcnhip_calib_scale_rows", lambda: dev.calib_scale_rows(logp, bad)),
                            ("gcnhip_conformal_scores", lambda: dev.conformal_scores(logp, bad, conformal_ref.APS))):
            with pytest.raises(GcnHipError, match=f"{entry}: {limit}"):
                call()
        with pytest.raises(Exception, match=f"gcnhip_attach_gather: {limit}"):
            dev.attach_gather(ptr, col, coef, ta, tb, epilogue="predict", beta=bad, logp=True)


# ---- the model --------------------------------------------------------------------------------------------------------------

def test_model_at_the_ends_of_the_bracket():
    """set_temperature(100) and (0.01) on a small trained model: predict(logp=True) is inside calib_ref.scale's bounds of the
    model's own T = 1 rows; conformal_fit and predict_sets answer with thresholds that are finite or +inf and sets that hold the
    top class; temperatures whose reciprocal passes GCNHIP_BETA_MAX are refused, the smallest accepted ones give no NaN"""
    from cuda_gcn_amd.model import HipGCNModel, GcnHostError
    ds = datagen.make_dataset("tiny-syn")
    m = HipGCNModel(ds, seed=5, hidden_dim=16, dropout=0.5)
    m.run_epochs(10, want_trace=False)
    c = ds["output_dim"]
    pred1, prob1, logp = m.predict(logp=True)
    assert np.isfinite(logp).all()
    for temp in (100.0, 0.01):
        m.set_temperature(temp)
        beta = calib_ref.f32(np.float32(1.0) / np.float32(temp))
        out, e_out, prob_ref, e_prob = calib_ref.scale(logp, beta)
        pred, prob, lp = m.predict(logp=True)
        assert np.array_equal(pred, pred1)
        within("model logp", lp, out, e_out, f"T {temp}")
        within("model prob", prob, prob_ref, e_prob, f"T {temp}")
        for method in ("lac", "aps"):
            fit = m.conformal_fit(alpha=0.1, method=method)
            assert not np.isnan(fit["thresh"]).any() and np.all((fit["thresh"] == np.inf) | np.isfinite(fit["thresh"]))
            member, size = m.predict_sets(fit, nodes=np.arange(ds["num_nodes"], dtype=np.int32))
            assert member.shape == (ds["num_nodes"], c) and np.array_equal(size, member.sum(axis=1))
            if fit["threshold"] == np.inf:
                assert member.all()
    for temp in (1e-38, 1.2e-38, 1e-45):
        with pytest.raises(GcnHostError, match="set_temperature: the temperature must be finite and > 0, with 1 / T at most 8e37"):
            m.set_temperature(temp)
    for temp in (1.3e-38, 3e38):
        m.set_temperature(temp)
        pred, prob, lp = m.predict(logp=True)
        assert np.array_equal(pred, pred1) and not np.isnan(prob).any() and not np.isnan(lp).any() and np.all(lp <= 0)
    m.set_temperature(1.0)
    assert all(same_bits(x, y) for x, y in zip((pred1, prob1, logp), m.predict(logp=True)))
    m.close()
