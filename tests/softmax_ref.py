"""float64 numpy reference of the max-shifted softmax as the loss and prediction kernels form it (csrc/xent.hip, the loss and
predict epilogues of csrc/graphsum.hip, attach_finish of csrc/attach.hip), with an ERROR BOUND for every f32 output, and a table
of hard logit rows.  No GPU here.

The kernels form, per row of f32 logits z (read exactly) with label t,
    m = max_j z_j,  e_j = expf(z_j - m),  Z = sum_j e_j,  p_j = e_j / Z,
    term = logf(Z) - (z_t - m),   g_j = (p_j - [j == t]) / count  [. row factor] [. class weight],
    prob = 1 / Z,   logp_j = (z_j - m) - logf(Z),   correct = no z_j above z_t,   pred = the lowest column among the maxima.
`correct` and `pred` compare input floats: they are exact, not bounded.

Error bounds: the model and the constants of tests/calib_ref.py (U = 2^-24, EXP_ATOL for expf and logf, TINY where f32 flushes).
  argument    d_j = U (|z_j| + |m| + |z_j - m|)
  e_j         relative eps_j = EXP_ATOL + 1.01 d_j, plus TINY absolute
  Z           relative eps_Z = sum_j p_j eps_j + 1.01 (C - 1) U.  The second term is the bound of ONE f32 sum of C non-negative
              terms added in ANY order ((1 + U)^(C - 1) - 1 <= 1.01 (C - 1) U for C <= 256).  DESIGN §2's 8 U rule, which
              calib_ref uses here, is a bound for the TREE sums of this project; it does not cover xent_lane_kernel and the
              epilogues, which add left to right over up to 64 terms (and C = 256 in the wave form is 4 terms per lane and then
              a tree: the any-order bound covers it too).  The f32 restatement below (restate_f32) with 8 U in its place reaches 3.5
              of the term's bound on hard_rows(256); with (C - 1) U it stays at 0.6 (tests/test_softmax_cpu.py).
  p_j         dp_j = p_j (eps_j + eps_Z + U) + TINY                               (one division)
  term        E_term = eps_Z + (EXP_ATOL + U) |log Z| + 2 U |z_t - m| + U |term|
              (logf of a Z that is eps_Z off, logf's own error and the rounding of its result, the rounded difference
              z_t - m counted twice for its appearance beside m, the final subtraction)
  g_j         E_g = (dp_j + U |p_j - y_j|) / count + U |g_j| + 2^-149; with a row factor s the bound is multiplied by
              |s| (1 + U), with a class weight w by w (1 + U) — what the product does to the error its operand carries — and
              each of the two products rounds once itself: 1.01 U |g_j| more per factor, g_j the final entry (1.01 for the
              second-order terms).  Without that term the label's entry of a confidently wrong row, (p - 1) / count with
              p ~ 0, is allowed 2 U |g| — the rounded p - 1 and the division — while a kernel with a class weight rounds three
              times and one with a row factor as well four times.
  loss sum    sum_r E_term[r] + 8 U sum_r |term_r|: DESIGN §2, the kernels add the rows' terms in a tree
  weighted    the term w . term is one more product: E_wterm = w E_term (1 + U) + U |w term|, summed as above; the sum of the
              weights themselves is one tree sum: 8 U sum w
  prob        1 / Z: relative eps_Z + U
  logp_j      E_o = d_j + eps_Z + EXP_ATOL |log Z| + U |logp_j|                    (calib_ref's E_o)
  beta != 1   attach_finish rescales ITS OWN f32 log-softmax row l' (within E_o of the real l) as calib_scale_kernel does.
              calib_ref.scale(l, beta) gives the real result o and E_out for exact input.  The input error moves every
              argument beta . l_j by at most |beta| max_j E_o; log-softmax is 1-Lipschitz in the maximum norm in each of its
              two parts (the argument itself and the log-sum-exp), so o moves by at most 2 |beta| max_j E_o =: E_in, and the
              bounds of scale() — which are functions of |s_j|, |m| — grow by at most U . 3 E_in (absorbed by the factor
              (1 + 1e-6) below):  E_scaled = (E_out + E_in) (1 + 1e-6);  prob = exp(max o): relative EXP_ATOL + 1.01 max_j E_scaled.
No tolerance here was tuned to a GPU result."""
import numpy as np

from tests.calib_ref import U, EXP_ATOL, TINY
from tests import calib_ref

DENORM = 2.0 ** -149
LO, HI = -9e29, float(np.float32(1e30))          # every logit of hard_rows lies in [LO, HI]
WIDE_A = (20.0, 44.0, 60.0, 1e4, 1e30)
CONSTANTS = (0.0, 7.5, -5e29, 9e29)
UNDERFLOW_D = (17.0, 87.0, 87.4, 88.0, 103.0, 104.0, 120.0)


def _hard(C, seed):
    rng = np.random.default_rng([seed, C])
    rows, truth, kinds = [], [], []

    def add(z, t, kind):
        z = np.clip(np.asarray(z, np.float64), LO, HI).astype(np.float32)
        z[z == 0] = 0.0                                   # no -0.0
        rows.append(z); truth.append(int(t) % C); kinds.append(kind)

    for _ in range(8):
        add(rng.standard_normal(C) * 3, rng.integers(0, C), "control")
    for k, a in enumerate(WIDE_A):                        # (the low side of A = 1e30 is the table's lower limit, -9e29)
        hot = (5 * k + 2) % C
        for off in (0, 1):
            z = np.full(C, -a)
            z[hot] = a
            add(z, hot + off, "wide")
    for v in CONSTANTS:
        add(np.full(C, v), C - 1, "constant")
    for a, b in ((0, C - 1), (3, 4), (C // 2, C - 1)):
        if not 0 <= a < b < C:
            continue
        for t in (a, b):
            top = float(np.float32(rng.uniform(-2, 2)))
            z = top - 12 + rng.uniform(-0.25, 0.25, C)
            z[a] = z[b] = top
            add(z, t, "tie")
    for k, d in enumerate(UNDERFLOW_D):
        hot = (9 * k + 1) % C
        for off in (0, 1):
            z = 5.0 - d + rng.uniform(-0.25, 0.25, C)
            z[hot] = 5.0
            add(z, hot + off, "underflow")
    return np.stack(rows), np.asarray(truth, np.int32), kinds


def hard_rows(C, seed=0):
    """(logits f32 [R, C], truth int32 [R]): control, wide, constant, tie and underflow rows (see hard_kinds); all finite, in
    [-9e29, 1e30], no -0.0.  Tie rows whose two columns do not exist at this C are left out (C >= 5 has every kind)."""
    z, t, _ = _hard(C, seed)
    return z, t


def hard_kinds(C, seed=0):
    """the kind of every row of hard_rows(C, seed): 'control', 'wide', 'constant', 'tie', 'underflow'"""
    return _hard(C, seed)[2]


BETAS = (calib_ref.BETA_LO, 0.25, 1.0, 4.0, calib_ref.BETA_HI)      # the ends of calibrate()'s bracket and the betas of the dispatch files
CS = (1, 2, 5, 41, 63, 64)       # one lane, the smallest tie, the smallest C with every kind, the model's 41, the last lane empty, a full wave
SPREAD_STEP = 1e-3


def hard_logp(C, seed=0):
    """(logp f32 [R, C], truth int32 [R], kinds): the log-softmax rows a trained model hands to the kernels behind predict() —
    reference(hard_rows(C))["logp"] rounded to f32, row for row with that table's truth and kinds — and two rows of one further
    kind, 'spread': logits SPREAD_STEP apart (the classes in order and shuffled, the label on the largest and on the smallest),
    which beta = 0.01 makes uniform to 1e-5 . C and beta = 100 separates by 0.1 per class.  Every entry is finite (the lowest is
    -1.9e30) and the table is the same on every call."""
    z, t, kinds = _hard(C, seed)
    rng = np.random.default_rng([seed, C, 1])
    steps = np.arange(C, dtype=np.float64) * SPREAD_STEP
    shuffled = steps[rng.permutation(C)]
    z = np.concatenate([z, np.stack([steps, shuffled]).astype(np.float32)])
    t = np.concatenate([t, np.array([C - 1, int(np.argmin(shuffled))], np.int32)])
    logp = reference(z, t)["logp"].astype(np.float32)
    assert np.all(np.isfinite(logp))
    return logp, t, list(kinds) + ["spread", "spread"]


def tame_rows(z):
    """rows whose logits stay below 200 in magnitude: their loss terms are O(100), so a sum over them is not drowned by the
    1e30 of a wide row"""
    return np.abs(np.asarray(z, np.float64)).max(axis=1) <= 200.0


def reference(z, truth, count=None, row_scale=None, weight=None, beta=1.0):
    """Every row of z (f32 values, read exactly) in float64.  truth int [R]; rows with truth < 0 are not scored (term, E_term,
    grad 0).  count: the gradient's divisor (None: the number of scored rows; with `weight` the sum of weight[truth]).
    row_scale [R], weight [C]: optional factors of the gradient row (and, the weight, of the term).
    dict: term, E_term, correct (bool), grad, E_grad [R, C], pred, prob, E_prob, logp, E_logp, scored (bool), and with
    beta != 1 scaled, E_scaled, sprob, E_sprob (log_softmax(beta . logp) as calib_ref.scale forms it, see the module docstring);
    with weight also wsum and E_wsum (the sum of the scored rows' weights)."""
    z = np.asarray(z, np.float32).astype(np.float64)
    r, c = z.shape
    truth = np.asarray(truth, np.int64)
    scored = truth >= 0
    t = np.where(scored, truth, 0)
    k = np.arange(r)
    m = z.max(axis=1, keepdims=True)
    s = z - m
    e = np.exp(s)
    zsum = e.sum(axis=1, keepdims=True)
    p = e / zsum
    logz = np.log(zsum)
    d = U * (np.abs(z) + np.abs(m) + np.abs(s))
    eps = EXP_ATOL + 1.01 * d
    eps_z = (p * eps).sum(axis=1, keepdims=True) + 1.01 * (c - 1) * U
    dp = p * (eps + eps_z + U) + TINY
    zt = z[k, t]
    term = logz[:, 0] - (zt - m[:, 0])
    e_term = eps_z[:, 0] + (EXP_ATOL + U) * np.abs(logz[:, 0]) + 2 * U * np.abs(zt - m[:, 0]) + U * np.abs(term)
    correct = ~np.any(z > zt[:, None], axis=1) & scored
    pred = np.argmax(z, axis=1)
    y = np.zeros((r, c))
    y[k, t] = 1.0
    w = np.asarray(weight, np.float32).astype(np.float64)[t] if weight is not None else None
    if count is None:
        count = float(w[scored].sum()) if w is not None else float(max(int(scored.sum()), 1))
    count = float(np.float32(count))
    g = (p - y) / count
    e_g = (dp + U * np.abs(p - y)) / count + U * np.abs(g) + DENORM
    if w is not None:
        g = g * w[:, None]
        e_g = e_g * (w * (1 + U))[:, None] + 1.01 * U * np.abs(g)
        e_term = w * e_term * (1 + U) + U * np.abs(w * term)
        term = w * term
    if row_scale is not None:
        sc = np.asarray(row_scale, np.float32).astype(np.float64)[:, None]
        g = g * sc
        e_g = e_g * np.abs(sc) * (1 + U) + 1.01 * U * np.abs(g)
    term, e_term = np.where(scored, term, 0.0), np.where(scored, e_term, 0.0)
    g, e_g = np.where(scored[:, None], g, 0.0), np.where(scored[:, None], e_g, 0.0)
    logp = s - logz
    e_logp = d + eps_z + EXP_ATOL * np.abs(logz) + U * np.abs(logp)
    prob = 1.0 / zsum[:, 0]
    out = dict(term=term, E_term=e_term, correct=correct, grad=g, E_grad=e_g, pred=pred, prob=prob, E_prob=prob * (eps_z[:, 0] + U),
               logp=logp, E_logp=e_logp, scored=scored, count=count)
    if w is not None:
        out["wsum"] = float(w[scored].sum())
        out["E_wsum"] = 8 * U * out["wsum"]
    if beta != 1.0:
        o, e_o, _, _ = calib_ref.scale(logp, calib_ref.f32(beta))
        e_in = 2 * abs(calib_ref.f32(beta)) * e_logp.max(axis=1, keepdims=True)
        e_s = (e_o + e_in) * (1 + 1e-6)
        out["scaled"], out["E_scaled"] = o, e_s
        out["sprob"] = np.exp(o.max(axis=1))
        out["E_sprob"] = out["sprob"] * (EXP_ATOL + 1.01 * e_s.max(axis=1))
    return out


def loss_sum(ref, rows=None):
    """(sum of the terms, its bound) over the listed rows (None: all): sum E_term + 8 U sum |term| — the kernels add rows in a tree"""
    term, e = ref["term"], ref["E_term"]
    if rows is not None:
        term, e = term[rows], e[rows]
    return float(term.sum()), float(e.sum() + 8 * U * np.abs(term).sum())


def worst(got, want, bound):
    """max |got - want| / bound; a non-finite `got` counts as infinitely far"""
    got, want, bound = (np.asarray(a, np.float64) for a in (got, want, bound))
    if got.size == 0:
        return 0.0
    if not np.all(np.isfinite(got)):
        return float("inf")
    diff = np.abs(got - want)
    return float(np.where(diff == 0, 0.0, diff / np.where(diff == 0, 1.0, bound)).max())      # (a bound of 0 allows no difference)


def restate_f32(z, truth, count, flush=False, row_scale=None, weight=None):
    """The kernel statements of xent_lane_kernel / the epilogues in f32 numpy: max, shift, expf, the LEFT-TO-RIGHT sum, the term,
    p = e / Z, the label's (float)((double)p - 1.0), the division by count.  flush=True: subnormal exp results and quotients
    become zero (what a flushing f32 unit would return).  weight [C], row_scale [R]: the factors of the weighted kernels and of
    grad_row_scale, in the kernels' order (w . p, then / count, then . scale).  Returns (term f32 [R], grad f32 [R, C])."""
    z = np.asarray(z, np.float32)
    r, c = z.shape
    tiny = np.finfo(np.float32).tiny
    k = np.arange(r)
    with np.errstate(under="ignore", over="ignore"):
        mx = np.maximum(np.float32(-1e30), z.max(axis=1))
        v = z - mx[:, None]
        e = np.exp(v)
        if flush:
            e = np.where(e < tiny, np.float32(0), e)
        se = np.zeros(r, np.float32)
        for j in range(c):
            se = se + e[:, j]
        term = np.log(se) - (z[k, truth] - mx)
        p = e / se[:, None]
        if flush:
            p = np.where(np.abs(p) < tiny, np.float32(0), p)
        p[k, truth] = (p[k, truth].astype(np.float64) - 1.0).astype(np.float32)
        if weight is not None:
            w = np.asarray(weight, np.float32)[truth]
            term, p = w * term, w[:, None] * p
        g = p / np.float32(count)
        if row_scale is not None:
            g = g * np.asarray(row_scale, np.float32)[:, None]
        if flush:
            g = np.where(np.abs(g) < tiny, np.float32(0), g)
    assert term.dtype == np.float32 and g.dtype == np.float32
    return term, g
