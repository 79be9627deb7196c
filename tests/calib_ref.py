"""float64 numpy reference of temperature scaling and the reliability diagram as the GPU path computes them (no GPU here):
the negative log-likelihood of softmax(beta . l) with its first and second derivative in beta, the safeguarded Newton fit,
the bins, the report and the rescaled rows — each with an ERROR BOUND for the f32 kernels of csrc/calib.hip, so that no
tolerance has to be guessed.

Inputs are log-softmax rows l (f32 values, read exactly) and an f32 beta = 1 / T.  The kernels form, per row,
    s_j = beta . l_j,  m = max_j s_j,  e_j = expf(s_j - m),  Z = sum_j e_j,  p_j = e_j / Z.

Error bounds (u = 2^-24, the unit roundoff of f32; EXP_ATOL the relative tolerance of expf the prediction tests use for
prob, taken for logf too; DESIGN §2: one f32 sum of terms t_i in any order is within 8 u sum |t_i| of the real sum).
  argument    s_j and m are one rounded product each and s_j - m one rounded difference:
                  d_j = u (|s_j| + |m| + |s_j - m|)
  e_j         relative EXP_ATOL + 1.01 d_j =: eps_j (exp(d) - 1 <= 1.01 d for d < 0.01), plus TINY absolute where f32 flushes a
              value that float64 still holds (p_j < 1e-37: such an entry weighs nothing)
  Z           relative eps_Z = sum_j p_j eps_j + 8 u
  p_j         relative pi_j = eps_j + eps_Z + u (one division):   dp_j = p_j pi_j + TINY
  conf        = max_j p_j:                                         E_conf = max_j dp_j
  lse         logf(Z) + m:  E_lse = eps_Z + EXP_ATOL |log Z| + u |m| + u |lse|
  nll_r       lse - beta . l_t:  E_nll = E_lse + u |s_t| + u |nll_r|
  mu          sum_j p_j l_j:  E_mu = sum_j |l_j| (dp_j + 9 u p_j)      (each product rounds once, the sum by DESIGN §2)
  g_r         mu - l_t:  E_g = E_mu + u |g_r|
  h_r         sum_j p_j (l_j - mu)^2, the centred sum.  c_j = l_j - mu carries e_c = E_mu + u |c_j|, its square
              2 |c_j| e_c + e_c^2 + u c_j^2, and the product and the sum 9 u p_j c_j^2:
                  E_h = sum_j [dp_j c_j^2 + p_j (2 |c_j| e_c + e_c^2 + 10 u c_j^2)]
  scaled row  o_j = (s_j - m) - logf(Z):  E_o = d_j + eps_Z + EXP_ATOL |log Z| + u |o_j|;   prob = expf(max_j o_j): relative
              EXP_ATOL + 1.01 max_j E_o
Sums over rows are doubles added in a fixed order: their own rounding (2^-53 per add) is far below the first u above and is
covered by a factor (1 + 1e-9) on the summed bounds.  The summed gradient's bound is E_g_sum = sum_r E_g[r]."""
import numpy as np

U = 2.0 ** -24
EXP_ATOL = 2e-6      # f32 expf of a log-probability: the relative tolerance the prediction tests use for prob (smooth_ref.EXP_ATOL)
TINY = 1e-37
BETA_LO, BETA_HI = 0.01, 100.0


def f32(x):
    """the f32 value nearest to x, as a Python float: what a kernel argument holds"""
    return float(np.float32(x))


def _rows(logp, truth, rows):
    """the counted rows in list order (repeats counted as often as listed): ids inside the table whose truth is a class"""
    logp = np.asarray(logp, np.float64)
    n, c = logp.shape
    idx = np.arange(n) if rows is None else np.asarray(rows, np.int64).ravel()
    idx = idx[(idx >= 0) & (idx < n)]
    if truth is None:
        return logp, idx, None
    truth = np.asarray(truth, np.int64)
    idx = idx[(truth[idx] >= 0) & (truth[idx] < c)]
    return logp, idx, truth[idx]


def _softmax(l, beta):
    """per row: s, m, p, log Z and the bounds d (argument), dp (probability), eps_Z"""
    s = beta * l
    m = s.max(axis=1, keepdims=True) if s.shape[0] else np.zeros((0, 1))
    e = np.exp(s - m)
    z = e.sum(axis=1, keepdims=True)
    p = e / z
    d = U * (np.abs(s) + np.abs(m) + np.abs(s - m))
    eps = EXP_ATOL + 1.01 * d
    eps_z = (p * eps).sum(axis=1, keepdims=True) + 8 * U
    dp = p * (eps + eps_z + U) + TINY
    return s, m, p, np.log(z), d, dp, eps_z


def nll_g_h(logp, truth, beta, rows=None):
    """dict: nll, g, h (float64 per counted row), their f32 bounds E_nll, E_g, E_h, the sums S = {sum nll, sum g, sum h, rows}
    and E_S, the bounds of the three sums.  g = d nll / d beta = mu - l_t; h = d2 nll / d beta2 = sum_j p_j (l_j - mu)^2 >= 0."""
    logp, idx, t = _rows(logp, truth, rows)
    l = logp[idx]
    k = np.arange(idx.size)
    s, m, p, logz, d, dp, eps_z = _softmax(l, beta)
    lt, st = l[k, t], s[k, t]
    lse = (logz + m)[:, 0]
    nll = lse - st
    mu = (p * l).sum(axis=1)
    g = mu - lt
    c = l - mu[:, None]
    h = (p * c * c).sum(axis=1)
    e_lse = eps_z[:, 0] + EXP_ATOL * np.abs(logz[:, 0]) + U * np.abs(m[:, 0]) + U * np.abs(lse)
    e_nll = e_lse + U * np.abs(st) + U * np.abs(nll)
    e_mu = (np.abs(l) * (dp + 9 * U * p)).sum(axis=1)
    e_g = e_mu + U * np.abs(g)
    e_c = e_mu[:, None] + U * np.abs(c)
    e_h = (dp * c * c + p * (2 * np.abs(c) * e_c + e_c * e_c + 10 * U * c * c)).sum(axis=1)
    sums = np.array([nll.sum(), g.sum(), h.sum(), float(idx.size)])
    e_sums = np.array([e_nll.sum(), e_g.sum(), e_h.sum()]) * (1 + 1e-9)
    return dict(nll=nll, g=g, h=h, E_nll=e_nll, E_g=e_g, E_h=e_h, S=sums, E_S=e_sums, rows=idx)


def newton(evaluate, rel_tol=1e-6, max_steps=40, round_beta=f32):
    """The safeguarded Newton iteration of HipGCN::calibrate on a convex function of beta.  evaluate(beta) -> (sum nll, sum g,
    sum h, rows).  From beta = 1 inside the bracket [0.01, 100], which moves with the sign of g; the Newton step beta - g / h when
    h > 0 and it stays strictly inside the bracket, else the geometric midpoint (while the end the step goes to is still the outer
    limit, the step is at least a factor 2: the tail of a perfectly classified split is left behind within the 40 steps); stops
    when |delta beta| <= rel_tol . beta or after max_steps.  round_beta: what the evaluation sees (the kernels take an f32 beta; None: float64 throughout).  Returns a dict:
    beta, temperature, nll_before, nll_after (means), steps, at_bound, and the last evaluation's sums S."""
    lo, hi, beta = BETA_LO, BETA_HI, 1.0
    s = evaluate(beta)
    before = s[0] / s[3]
    steps = 0
    while steps < max_steps:
        g, h = s[1], s[2]
        if g > 0:
            hi = beta
        elif g < 0:
            lo = beta
        else:
            break
        nxt = beta - g / h if h > 0 else 0.0
        if h > 0 and g < 0 and hi == BETA_HI:                     # no minimum seen yet on that side: at least a factor 2
            nxt = max(nxt, 2 * beta)
        if h > 0 and g > 0 and lo == BETA_LO:
            nxt = min(nxt, beta / 2)
        if not h > 0 or not lo < nxt < hi:
            nxt = float(np.sqrt(lo * hi))
        if round_beta:
            nxt = round_beta(nxt)
        delta = abs(nxt - beta)
        beta = nxt
        steps += 1
        s = evaluate(beta)
        if delta <= rel_tol * beta:
            break
    flat = s[1] == 0                                              # the gradient vanished before a minimum was bracketed on that side
    at_bound = (hi == BETA_HI and (beta >= BETA_HI * (1 - 1e-4) or (flat and beta > 1))) or \
        (lo == BETA_LO and (beta <= BETA_LO * (1 + 1e-4) or (flat and beta < 1)))
    return dict(beta=beta, temperature=1.0 / beta, nll_before=before, nll_after=s[0] / s[3], steps=steps, at_bound=bool(at_bound), S=s)


def fit(logp, truth, rows=None):
    """the fit in float64, run to 1e-12: the minimiser of the NLL of softmax(beta . l) over the counted rows, inside [0.01, 100]"""
    return newton(lambda b: nll_g_h(logp, truth, b, rows)["S"], rel_tol=1e-12, max_steps=200, round_beta=None)


def bins(logp, truth, beta, n_bins, rows=None):
    """dict: conf, pred, bin per counted row, the per-bin count / correct (int64) / conf_sum (float64), the per-row bound E_conf,
    `ambiguous` (rows whose conf . bins lies within n_bins . E_conf + u . conf . n_bins of an integer: an f32 kernel may put them
    into the neighbouring bin) and amb_near [n_bins] = the ambiguous rows in or beside each bin.  Bin b holds conf in
    (b / B, (b + 1) / B]; pred is the largest l_j, the lowest column on a tie."""
    logp, idx, t = _rows(logp, truth, rows)
    l = logp[idx]
    _, _, p, _, _, dp, _ = _softmax(l, beta)
    conf = p.max(axis=1) if idx.size else np.zeros(0)
    e_conf = dp.max(axis=1) if idx.size else np.zeros(0)
    pred = np.argmax(l, axis=1) if idx.size else np.zeros(0, np.int64)
    x = conf * n_bins
    b = np.clip(np.ceil(x).astype(np.int64) - 1, 0, n_bins - 1)
    amb = (np.abs(x - np.rint(x)) <= n_bins * e_conf + U * x) & (np.rint(x) > 0) & (np.rint(x) < n_bins)   # (the clamp owns both ends)
    count = np.bincount(b, minlength=n_bins).astype(np.int64)
    correct = np.bincount(b, weights=(pred == t).astype(np.float64), minlength=n_bins).astype(np.int64)
    conf_sum = np.bincount(b, weights=conf, minlength=n_bins)
    near = np.zeros(n_bins, np.int64)
    for bb in b[amb]:
        near[max(bb - 1, 0):bb + 2] += 1
    return dict(conf=conf, pred=pred, bin=b, count=count, correct=correct, conf_sum=conf_sum, E_conf=e_conf, ambiguous=amb, amb_near=near,
                rows=idx)


def report(count, correct, conf_sum):
    """dict: accuracy, confidence per bin (0 for an empty bin), ece, mce, rows — host/calibration.h in numpy"""
    count = np.asarray(count, np.float64)
    full = count > 0
    acc = np.where(full, np.asarray(correct, np.float64) / np.where(full, count, 1), 0.0)
    conf = np.where(full, np.asarray(conf_sum, np.float64) / np.where(full, count, 1), 0.0)
    gap = np.abs(acc - conf)
    rows = count.sum()
    return dict(accuracy=acc, confidence=conf, ece=float((count / rows * gap).sum()) if rows else 0.0,
                mce=float(gap[full].max()) if full.any() else 0.0, rows=int(rows))


def ece_bound(b, n_bins):
    """how far the ECE of an f32 kernel's bins may lie from report(b): every ambiguous row may change bins — it leaves one bin's
    gap sum and joins another's, at most 2 / rows in all — and every confidence carries E_conf"""
    n = max(b["conf"].size, 1)
    return (2.0 * int(b["ambiguous"].sum()) + float(b["E_conf"].sum())) / n


def scale(logp, beta, rows=None):
    """(out, E_out [n_table, C], prob, E_prob [n_table]; NaN where a row is not listed): log_softmax(beta . l) and the probability
    of its largest entry"""
    logp, idx, _ = _rows(logp, None, rows)
    idx = np.unique(idx)
    n, c = logp.shape
    out, e_out = np.full((n, c), np.nan), np.full((n, c), np.nan)
    prob, e_prob = np.full(n, np.nan), np.full(n, np.nan)
    s, m, p, logz, d, dp, eps_z = _softmax(logp[idx], beta)
    o = (s - m) - logz
    eo = d + eps_z + EXP_ATOL * np.abs(logz) + U * np.abs(o)
    out[idx], e_out[idx] = o, eo
    if idx.size:
        prob[idx] = np.exp(o.max(axis=1))
        e_prob[idx] = prob[idx] * (EXP_ATOL + 1.01 * eo.max(axis=1))
    return out, e_out, prob, e_prob
