"""The hard log-softmax table (softmax_ref.hard_logp) against the kernels that read predict()'s rows, without a GPU: f32 numpy
restatements of calib_nll_kernel, calib_bins_kernel, calib_scale_kernel (csrc/calib.hip) and conformal_scores_kernel
(csrc/conformal.hip) — lane by lane on a 64-lane row, with the kernels' sum orders: the xor butterfly of wave_sum, the
Kogge-Stone scan over the ranks, the cum clamp, the last rank set to 1 — stay inside the bounds of tests/calib_ref.py and
tests/conformal_ref.py for every (C, beta) of softmax_ref.CS x BETAS, so the references are inside their own bounds on these rows
and the GPU file (tests/test_hard_logp_gpu.py) asks for nothing a faithful f32 kernel cannot give.

Two properties are contracts of conformal.hip's header, not bounds (a cum that is an ulp off 1 is inside every bound): no APS
score without a penalty exceeds 1.0f, and the last-ranked class scores f32(1) + pen bit for bit.  They are asserted with the bounds.

Four mutants of the restatement show that the table reaches the statements that keep the kernels finite and exact.  Each must
fail on the cases named here (rows by kind; the figures are those of this table, seed 0):
  no maximum shift (m = 0)       the constant rows at beta = 100, C >= 5: every s_j = -100 ln C <= -160 underflows expf, Z = 0, and
                                 nll, the scaled row and every score are non-finite (4 rows at each of C = 5, 41, 63, 64)
  no `p == 0` guard              the two wide rows with logits +-1e30 (l = -1.9e30 off the maximum), every beta, C >= 2:
                                 (l - mu)^2 overflows to +inf and 0 . inf = NaN reaches h (2 rows x 5 betas at each C)
  no cum clamp                   plain APS at beta = 4, C = 41, 63, 64 (NO_CLAMP_CASES): control rows whose f32 scan passes 1.0f
                                 before the last rank (3, 2 and 4 rows)
  last rank not forced to 1.0f   plain APS at every C >= 2 and beta <= 4 (LAST_RANK_CASES): rows whose f32 sum of all p stays
                                 below 1.0f (1 to 11 rows per case)
"""
import numpy as np
import pytest

from tests import calib_ref
from tests import conformal_ref
from tests import softmax_ref as R

W = 64
LANES = np.arange(W)
F = np.float32
METHODS = {"lac": (conformal_ref.LAC, 0.0, 0), "aps": (conformal_ref.APS, 0.0, 0), "raps": (conformal_ref.APS, 0.01, 2)}


# ---- the kernel statements, f32, one row of 64 lanes per table row -------------------------------------------------------

def lanes(logp):
    """(l f32 [R, 64] with 0 past C, live bool [64])"""
    logp = np.asarray(logp, F)
    l = np.zeros((logp.shape[0], W), F)
    l[:, :logp.shape[1]] = logp
    return l, LANES < logp.shape[1]


def wave_sum(v):
    """v += __shfl_xor(v, off) for off = 32 .. 1: every lane ends with the same f32"""
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, LANES ^ off]
    assert v.dtype == F
    return v[:, :1]


def wave_max(v):
    return np.fmax.reduce(v, axis=1, keepdims=True)           # fmaxf: exact, any order


def row_softmax(l, live, beta, shift=True):
    """row_softmax of calib.hip: (s, e, m, z)"""
    s = F(beta) * l
    m = wave_max(np.where(live, s, F(-np.inf))) if shift else np.zeros((l.shape[0], 1), F)
    e = np.where(live, np.exp(s - m), F(0))
    return s, e, m, wave_sum(e)


def nll_rows(logp, truth, beta, shift=True, guard=True):
    """calib_nll_kernel per row: (nll, g, h) f32 [R]"""
    l, live = lanes(logp)
    k = np.arange(l.shape[0])
    with np.errstate(all="ignore"):
        s, e, m, z = row_softmax(l, live, beta, shift)
        p = e / z
        lt = l[k, truth][:, None]
        nll = (np.log(z) + m) - F(beta) * lt
        mu = wave_sum(np.where(p == 0, F(0), p * l) if guard else p * l)
        d = l - mu
        h = wave_sum(np.where(p == 0, F(0), p * (d * d)) if guard else p * (d * d))
        g = mu - lt
    assert nll.dtype == F and g.dtype == F and h.dtype == F
    return nll[:, 0], g[:, 0], h[:, 0]


def bins_rows(logp, beta, n_bins, shift=True):
    """calib_bins_kernel per row: (conf f32, pred, bin)"""
    l, live = lanes(logp)
    with np.errstate(all="ignore"):
        _, _, _, z = row_softmax(l, live, beta, shift)
        conf = F(1) / z
        lmax = wave_max(np.where(live, l, F(-np.inf)))
        pred = np.argmax(live & (l == lmax), axis=1)           # __ffsll of the ballot: the lowest lane
        b = np.clip(np.nan_to_num(np.ceil(conf * F(n_bins)), nan=0.0, posinf=0.0).astype(np.int64) - 1, 0, n_bins - 1)
    assert conf.dtype == F
    return conf[:, 0], pred, b[:, 0]


def scale_rows(logp, beta, shift=True):
    """calib_scale_kernel per row: (out f32 [R, C], prob f32 [R])"""
    l, live = lanes(logp)
    with np.errstate(all="ignore"):
        s, _, m, z = row_softmax(l, live, beta, shift)
        o = (s - m) - np.log(z)
        prob = np.exp(wave_max(np.where(live, o, F(-np.inf))))
    assert o.dtype == F and prob.dtype == F
    return o[:, :logp.shape[1]], prob[:, 0]


def score_rows(logp, beta, method, lam=0.0, k_reg=0, shift=True, clamp=True, force_last=True):
    """conformal_scores_kernel per row: f32 [R, C]"""
    l, live = lanes(logp)
    n, c = logp.shape
    with np.errstate(all="ignore"):
        s, e, m, z = row_softmax(l, live, beta, shift)
        p = e / z
        if method == conformal_ref.LAC:
            score = F(1) - p
        else:
            rank = np.tile(LANES, (n, 1))                      # cf_rank: lanes past C keep their own lane
            for j in range(c):
                rank[:, j] = ((l[:, :c] > l[:, j:j + 1]) | ((l[:, :c] == l[:, j:j + 1]) & (LANES[:c] < j))).sum(axis=1)
            v = np.zeros((n, W), F)
            np.put_along_axis(v, rank, p, axis=1)              # ds_permute: lane rank <- p
            for off in (1, 2, 4, 8, 16, 32):                   # the inclusive Kogge-Stone scan
                t = np.zeros_like(v)
                t[:, off:] = v[:, :-off]
                v = np.where(LANES >= off, v + t, v)
            cum = np.take_along_axis(v, rank, axis=1)
            if clamp:
                cum = np.fmin(cum, F(1))
            if force_last:
                cum = np.where(rank == c - 1, F(1), cum)
            pen = F(lam) * np.maximum(rank + 1 - int(k_reg), 0).astype(F)
            score = cum + pen
    assert score.dtype == F
    return score[:, :c]


def last_rank_score(c, lam, k_reg):
    return F(1) + F(lam) * F(max(0, c - k_reg))


# ---- the table ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", R.CS)
def test_hard_logp_properties(C):
    logp, t, kinds = R.hard_logp(C)
    z, tz = R.hard_rows(C)
    n = z.shape[0]
    assert logp.dtype == np.float32 and t.dtype == np.int32 and logp.shape == (n + 2, C) and t.shape == (n + 2,) and len(kinds) == n + 2
    assert kinds[:n] == R.hard_kinds(C) and kinds[n:] == ["spread", "spread"] and np.array_equal(t[:n], tz)
    assert np.all(np.isfinite(logp)) and np.all((t >= 0) & (t < C))
    again = R.hard_logp(C)
    assert np.array_equal(logp.view(np.uint32), again[0].view(np.uint32)) and np.array_equal(t, again[1])
    assert np.array_equal(logp[:n], R.reference(z, tz)["logp"].astype(np.float32))
    # log-softmax rows: the largest entry is at least -ln C (to f32), every row sums to 1 within the reference's own bound
    lse = np.log(np.exp(logp.astype(np.float64)).sum(axis=1))
    assert np.all(np.abs(lse) <= 64 * 2e-6) and np.all(logp.max(axis=1) >= np.float32(-np.log(C)) - 1e-6)
    if C >= 2:
        assert logp.min() < -1.8e30                              # the wide row with logits +-1e30
        # ties and constant rows are still exact ties after the rounding: the prediction is the lowest column
        kk = np.array(kinds)
        assert np.all(logp[kk == "constant"] == logp[kk == "constant"][:, :1])
        for r in np.flatnonzero(kk == "tie"):
            assert (logp[r] == logp[r].max()).sum() == 2
        # the spread rows: distinct logits, uniform to 1e-5 C at beta = 0.01, a factor e^0.1 per class at beta = 100
        sp = logp[kk == "spread"].astype(np.float64)
        assert all(np.unique(row).size == C for row in sp) and t[n] == np.argmax(sp[0]) and t[n + 1] == np.argmin(sp[1])
        p_lo = np.exp(0.01 * sp) / np.exp(0.01 * sp).sum(axis=1, keepdims=True)
        assert np.all(np.abs(p_lo * C - 1) <= 1e-5 * C)
        top2 = np.sort(100.0 * sp, axis=1)[:, -2:]
        assert np.allclose(top2[:, 1] - top2[:, 0], 0.1, rtol=0, atol=2e-3)
    assert R.BETAS == (calib_ref.BETA_LO, 0.25, 1.0, 4.0, calib_ref.BETA_HI) and R.CS == (1, 2, 5, 41, 63, 64)


@pytest.mark.parametrize("C", R.CS)
def test_the_conditions_on_the_inputs_hold_in_the_reference(C):
    """what the GPU file takes for granted, on the reference alone: with 1 and 7 bins no row's confidence is within its bound of a
    bin edge, with 15 bins at most 10 % of the rows are; every bound is finite and positive"""
    logp, t, _ = R.hard_logp(C)
    for beta in R.BETAS:
        for n_bins, limit in ((1, 0.0), (7, 0.0), (15, 0.1)):
            amb = int(calib_ref.bins(logp, t, calib_ref.f32(beta), n_bins)["ambiguous"].sum())
            assert amb <= limit * logp.shape[0], (C, beta, n_bins, amb)
        w = calib_ref.nll_g_h(logp, t, calib_ref.f32(beta))
        for key in ("nll", "g", "h", "E_nll", "E_g", "E_h"):
            assert np.all(np.isfinite(w[key])), (C, beta, key)
        assert np.all(w["h"] >= 0) and np.all(w["E_nll"] > 0)
        for name, (method, lam, k_reg) in METHODS.items():
            s, e, _ = conformal_ref.scores(logp, beta, method, lam, k_reg)
            assert np.all(np.isfinite(s)) and np.all(np.isfinite(e)) and np.all(e > 0)


# ---- the faithful restatement is inside every bound ------------------------------------------------------------------------

def check_restatement(C, beta, shift=True, guard=True, clamp=True, force_last=True):
    """dict family -> (worst |got - want| / bound, the rows outside their bound or contract) for one (C, beta)"""
    logp, t, _ = R.hard_logp(C)
    b32 = calib_ref.f32(beta)
    out = {}

    def rows_outside(got, want, bound):
        got, want, bound = (np.asarray(a, np.float64).reshape(logp.shape[0], -1) for a in (got, want, bound))
        with np.errstate(invalid="ignore"):
            return np.flatnonzero(~(np.abs(got - want) <= bound).all(axis=1))

    def put(family, got, want, bound):
        out[family] = (R.worst(got, want, bound), rows_outside(got, want, bound))

    w = calib_ref.nll_g_h(logp, t, b32)
    nll, g, h = nll_rows(logp, t, b32, shift, guard)
    put("nll", nll, w["nll"], w["E_nll"])
    put("g", g, w["g"], w["E_g"])
    put("h", h, w["h"], w["E_h"])
    with np.errstate(invalid="ignore"):
        out["h >= 0"] = (0.0, np.flatnonzero(~(h >= 0)))
    for n_bins in (1, 7, 15):
        b = calib_ref.bins(logp, t, b32, n_bins)
        conf, pred, bb = bins_rows(logp, b32, n_bins, shift)
        put(f"conf{n_bins}", conf, b["conf"], b["E_conf"])
        clear = ~b["ambiguous"]
        out[f"bin{n_bins}"] = (0.0, np.flatnonzero(clear & ((bb != b["bin"]) | (pred != b["pred"]))))
    o, e_o, prob, e_prob = calib_ref.scale(logp, b32)
    so, sp = scale_rows(logp, b32, shift)
    put("scaled", so, o, e_o)
    put("prob", sp, prob, e_prob)
    for name, (method, lam, k_reg) in METHODS.items():
        s, e, rank = conformal_ref.scores(logp, beta, method, lam, k_reg)
        got = score_rows(logp, b32, method, lam, k_reg, shift, clamp, force_last)
        put(name, got, s, e)
        if method == conformal_ref.APS:
            last = last_rank_score(C, lam, k_reg)
            out[name + " last rank"] = (0.0, np.flatnonzero((got[rank == C - 1] != last)))
            if lam == 0:
                with np.errstate(invalid="ignore"):
                    out[name + " <= 1"] = (0.0, np.flatnonzero(~(got <= F(1)).all(axis=1)))
    return out


@pytest.mark.parametrize("C", R.CS)
def test_f32_restatement_is_inside_every_bound(C):
    worst = {}
    for beta in R.BETAS:
        for family, (ratio, rows) in check_restatement(C, beta).items():
            assert rows.size == 0 and ratio <= 1.0, (C, beta, family, ratio, rows)
            worst[family] = max(worst.get(family, 0.0), ratio)
    print(f"C {C}: worst |got - want| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items() if v))


def test_the_bounds_are_not_vacuous_on_the_tame_rows():
    """control, tie, constant and spread rows at beta in [0.25, 4]: a scaled entry or a score that is 1e-4 off is caught"""
    logp, t, kinds = R.hard_logp(41)
    tame = np.isin(np.array(kinds), ["control", "tie", "constant", "spread"])
    for beta in (0.25, 1.0, 4.0):
        w = calib_ref.nll_g_h(logp, t, beta)
        assert np.all(w["E_nll"][tame] < 1e-4) and np.all(w["E_g"][tame] < 1e-3)
        assert np.all(calib_ref.scale(logp, beta)[1][tame] < 1e-4)
        for method, lam, k_reg in METHODS.values():
            assert np.all(conformal_ref.scores(logp, beta, method, lam, k_reg)[1][tame] < 1e-4)


# ---- the domain of beta -----------------------------------------------------------------------------------------------------

def test_the_beta_limit_is_where_a_constant_row_stops_being_finite():
    """GCNHIP_BETA_MAX = 8e37 (include/gcnhip_driver.h) from FLT_MAX / ln 64 = 8.18e37: the statements round s = beta . l before
    the maximum, so once beta . (-ln C) overflows every lane of a constant row holds -inf, m = -inf and s - m = NaN.  At the
    limit a constant row of up to 64 classes gives the uniform answer; above FLT_MAX / ln C the restatement gives NaN (a reading
    of the statements in f32 numpy — the entry points refuse such a beta, so no kernel is ever launched with one)."""
    limit = F(8e37)
    fmax = np.finfo(F).max
    assert limit < fmax / F(np.log(64.0)) < F(8.2e37)
    with np.errstate(over="ignore"):
        assert np.isfinite(limit * F(-np.log(64.0)) * F(1 + 1e-3))               # 0.1 % of slack for the row's own rounding, 2 % in all
    for C in (2, 41, 64):
        logp = np.full((1, C), F(-np.log(C)), F)
        t = np.zeros(1, np.int32)
        nll, g, h = nll_rows(logp, t, limit)
        o, prob = scale_rows(logp, limit)
        assert np.isfinite(nll).all() and np.isfinite(g).all() and np.isfinite(h).all()
        assert np.all(np.abs(o - F(-np.log(C))) <= 1e-6 * np.log(C) + 1e-7) and abs(float(prob[0]) - 1.0 / C) <= 1e-6
        for method, lam, k_reg in METHODS.values():
            assert np.isfinite(score_rows(logp, limit, method, lam, k_reg)).all()
        if C > 2:                                                 # (two classes: FLT_MAX . ln 2 is finite, no accepted f32 beta overflows)
            above = F(fmax / np.log(C) * 1.01)
            with np.errstate(over="ignore"):
                assert np.isfinite(above) and not np.isfinite(above * logp[0, 0])
            assert np.isnan(nll_rows(logp, t, above)[0]).all() and np.isnan(scale_rows(logp, above)[0]).all()
            assert np.isnan(score_rows(logp, above, conformal_ref.LAC)).all()


# ---- the mutants ----------------------------------------------------------------------------------------------------------

def rows_of(C, kind):
    return np.flatnonzero(np.array(R.hard_logp(C)[2]) == kind)


@pytest.mark.parametrize("C", [5, 41, 63, 64])
def test_mutant_without_the_maximum_shift_fails_on_the_constant_rows(C):
    """s_j = -100 ln C on every lane: without the shift every expf underflows and Z = 0"""
    const = rows_of(C, "constant")
    assert const.size == len(R.CONSTANTS)
    out = check_restatement(C, 100.0, shift=False)
    for family in ("nll", "scaled", "prob", "conf7", "lac", "aps", "raps"):
        assert np.isin(const, out[family][1]).all() and out[family][0] > 1.0, (C, family, out[family])
    assert all(out[family][0] == np.inf for family in ("nll", "scaled", "prob", "conf7", "lac"))        # (fminf(NaN, 1) = 1: the APS scores are finite and wrong)


@pytest.mark.parametrize("C", [2, 5, 41, 63, 64])
def test_mutant_without_the_zero_probability_guard_fails_on_the_widest_rows(C):
    """l = -1.9e30 off the maximum: (l - mu)^2 = +inf with p = 0"""
    logp = R.hard_logp(C)[0]
    widest = np.flatnonzero(logp.min(axis=1) < -1e19)
    assert widest.size == 2 and np.isin(widest, rows_of(C, "wide")).all()
    for beta in R.BETAS:
        out = check_restatement(C, beta, guard=False)
        assert np.array_equal(out["h"][1], widest) and out["h"][0] == np.inf, (C, beta, out["h"])
        assert all(rows.size == 0 for family, (_, rows) in out.items() if family not in ("h", "h >= 0"))


# the (C, beta) at which the unclamped f32 scan exceeds 1.0f before the last rank on at least one row (control rows: about forty
# comparable probabilities whose rounded partial sums pass 1 while the last classes still hold 1e-8)
NO_CLAMP_CASES = ((41, 4.0), (63, 4.0), (64, 4.0))
# ... and at which the f32 sum of all p stays below 1.0f on at least one row (every kind but the constant rows takes part)
LAST_RANK_CASES = tuple((c, beta) for c in (2, 5, 41, 63, 64) for beta in (0.01, 0.25, 1.0, 4.0))


def test_mutant_without_the_cum_clamp_breaks_the_full_set_contract():
    """nothing else notices: a cum one ulp above 1 is inside every bound, which is why the contract is asserted on its own"""
    for C, beta in NO_CLAMP_CASES:
        out = check_restatement(C, beta, clamp=False)
        assert out["aps <= 1"][1].size >= 1, (C, beta)
        assert all(rows.size == 0 for family, (_, rows) in out.items() if not family.endswith("<= 1")), (C, beta)


def test_mutant_without_the_forced_last_rank_breaks_the_bit_contract():
    """the penalty of `raps` can round the missing ulp away, so plain APS is the family that must notice"""
    for C, beta in LAST_RANK_CASES:
        out = check_restatement(C, beta, force_last=False)
        assert out["aps last rank"][1].size >= 1, (C, beta)
        assert np.isin(out["raps last rank"][1], out["aps last rank"][1]).all()
        assert all(rows.size == 0 for family, (_, rows) in out.items() if not family.endswith("last rank")), (C, beta)
