"""float64 numpy reference of Monte Carlo dropout as csrc/mcdropout.hip and ModelQueries::mc_dropout define it (no GPU here):
the stochastic forward with its masks drawn from tests/dropout_ref.keep — independently of the kernels — and the row-local
statistics, each with an ERROR BOUND for the kernels so that no tolerance has to be guessed.  Also the cases the CPU and the GPU
tests share (model_cases / model_weights / kernel_samples): the CPU tests check the conditions on these inputs with the reference
alone, the GPU tests run the kernels on the same inputs.

The forward (sample s, rate p, thr16 = dropout_threshold(p), sc = f32 1 / (1 - p), 64-bit seed):
    X~[jj]  = X[jj] . (keep(seed ^ KEY_INPUT_DROPOUT,  s, jj,        thr16) ? sc : 0)      jj: CSR order (dense: r . F + k)
    T       = X~ . W1
    H[r, c] = ReLU((A^ . T)[r, c]) . (keep(seed ^ KEY_HIDDEN_DROPOUT, s, r . h + c, thr16) ? sc : 0)
    Z       = A^ . (H . W2),     l_s = log_softmax(Z / temperature)
A^ comes from the stored rows: a(r, j) = 1 / sqrt(len(r) . len(j)), degree = stored row length.

Error bounds of the statistics.  The kernels read the f32 rows l_s exactly and work in float64 until one final f32 store, so a
statistic x carries (u = 2^-24, v = 2^-53)
    E(x) = u |x| + TINY + K v max(1, ln C)        K = 8 (C + S + 8)
the first term the store's rounding (TINY where f32 leaves the normal range), the last the float64 work: exp and log within
2 ulp each, a product, a 64-lane butterfly sum of C terms, S sequential adds, one division — fewer than C + S + 8 roundings,
each on a partial result no larger than max(1, ln C) (a probability, or an entropy <= ln C), with a factor 8 to spare.  The
mutual information is a difference of two such values, so its float64 part doubles.  pred and votes are integers: exact unless
`ambiguous` (below)."""
import numpy as np

from tests import dropout_ref as D

U = 2.0 ** -24
V = 2.0 ** -53
TINY = 1e-37
KEY_INPUT_DROPOUT = 0x9E3779B97F4A7C15
KEY_HIDDEN_DROPOUT = 0xD1B54A32D192ED03
KEY_MC_DROPOUT = 0xA0761D6478BD642F
M64 = (1 << 64) - 1
LOGIT_RTOL = 2e-5                                              # test_predict_gpu.py's rule for the reference's operation order


def logit_tol(z):
    return LOGIT_RTOL * max(1.0, float(np.abs(z).max()))


def log_softmax(z):
    z = np.asarray(z, np.float64)
    s = z - z.max(axis=1, keepdims=True)
    return s - np.log(np.exp(s).sum(axis=1, keepdims=True))


# ------------------------------------------------------------------------------------------------------------ the forward
def adjacency(ds):
    """(row of every stored edge, its column, a(r, j) in float64) from the stored rows, degree = stored row length"""
    gp, gi = np.asarray(ds["g_indptr"], np.int64), np.asarray(ds["g_indices"], np.int64)
    ln = np.diff(gp).astype(np.float64)
    rows = np.repeat(np.arange(gp.size - 1), np.diff(gp))
    return rows, gi, 1.0 / np.sqrt(ln[rows] * ln[gi])


def aggregate(adj, x):
    rows, cols, coef = adj
    out = np.zeros((int(rows.max()) + 1 if rows.size else 0, x.shape[1]))
    np.add.at(out, rows, coef[:, None] * x[cols])
    return out


def masked_features(ds, p, seed, s, key=KEY_INPUT_DROPOUT):
    """X~ as a dense float64 [N, F] matrix"""
    N, F = ds["num_nodes"], ds["input_dim"]
    fp = np.asarray(ds["f_indptr"], np.int64)
    v = np.asarray(ds["f_val"], np.float64).ravel()
    t = D.thr16(p)
    if t:
        k = D.keep((seed ^ key) & M64, s, np.arange(v.size, dtype=np.uint64), t)
        v = np.where(k, v * float(D.scale(p)), 0.0)
    x = np.zeros((N, F))
    fi = ds.get("f_indices")
    cols = np.tile(np.arange(F), N) if fi is None else np.asarray(fi, np.int64)
    np.add.at(x, (np.repeat(np.arange(N), np.diff(fp)), cols), v)    # (a repeated column adds, as the product does)
    return x


def sample_logits(ds, w1, w2, p, seed, s, adj=None, swap_keys=False):
    """Z of sample s in float64 [N, C]"""
    adj = adj or adjacency(ds)
    w1, w2 = np.asarray(w1, np.float64), np.asarray(w2, np.float64)
    k_in, k_hid = (KEY_HIDDEN_DROPOUT, KEY_INPUT_DROPOUT) if swap_keys else (KEY_INPUT_DROPOUT, KEY_HIDDEN_DROPOUT)
    a = aggregate(adj, masked_features(ds, p, seed, s, k_in) @ w1)
    h = np.maximum(a, 0.0)
    t = D.thr16(p)
    if t:
        k = D.keep((seed ^ k_hid) & M64, s, np.arange(h.size, dtype=np.uint64), t).reshape(h.shape)
        h = np.where(k, h * float(D.scale(p)), 0.0)
    return aggregate(adj, h @ w2)


def samples(ds, w1, w2, p, seed, first_sample, n_samples, temperature=1.0):
    """(Z [S, N, C], l [S, N, C]) of the samples first_sample .. first_sample + S - 1"""
    adj = adjacency(ds)
    z = np.stack([sample_logits(ds, w1, w2, p, seed, first_sample + s, adj) for s in range(n_samples)])
    return z, np.stack([log_softmax(zz / temperature) for zz in z])


# --------------------------------------------------------------------------------------------------------- the statistics
def statistics(logp, rows=None, tol=0.0):
    """logp [S, n_table, C]: log-softmax rows (f32 values, read exactly).  rows: the listed rows (None: all; an id outside the
    table adds nothing).  Returns a dict by list position: mean_prob [n, C], pred, confidence, entropy, expected_entropy,
    mutual_information, variation_ratio, votes [n, C], acc [n, C + 1] (the accumulators), E = the bound of every float statistic
    (one number: the largest over rows), ambiguous_samples [S, n] (the two largest entries of l_s lie within tol of each other
    without being equal columns: the vote may go either way; tol = 0: none) and ambiguous_rows [n] (the same for the two largest
    mean probabilities within 2 E, or a row with an ambiguous sample)."""
    logp = np.asarray(logp, np.float64)
    if logp.ndim == 2:
        logp = logp[None]
    S, n_table, C = logp.shape
    idx = np.arange(n_table) if rows is None else np.asarray(rows, np.int64).ravel()
    inside = (idx >= 0) & (idx < n_table)
    n = idx.size
    l = np.full((S, n, C), -np.inf)
    l[:, inside] = logp[:, idx[inside]]
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.exp(l)
        h = -np.where(p == 0.0, 0.0, p * np.where(p == 0.0, 0.0, l)).sum(axis=2)            # [S, n]
    acc = np.zeros((n, C + 1))
    votes = np.zeros((n, C), np.int64)
    amb_s = np.zeros((S, n), bool)
    for s in range(S):                                         # launch order
        acc[:, :C] += p[s]
        acc[:, C] += h[s]
        if inside.any():
            a = np.argmax(l[s][inside], axis=1)                # lowest class on a tie
            votes[np.flatnonzero(inside), a] += 1
        if tol > 0 and C > 1:
            t = np.sort(l[s], axis=1)
            amb_s[s] = inside & (t[:, -1] - t[:, -2] <= tol) & (t[:, -1] != t[:, -2])
    mp = acc[:, :C] / S
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = -np.where(mp > 0, mp * np.log(np.where(mp > 0, mp, 1.0)), 0.0).sum(axis=1)
    eent = acc[:, C] / S
    pred = np.argmax(mp, axis=1) if n else np.zeros(0, np.int64)
    k = 8.0 * (C + S + 8) * V * max(1.0, np.log(C))
    out = dict(mean_prob=mp, pred=pred, confidence=mp[np.arange(n), pred] if n else np.zeros(0), entropy=ent, expected_entropy=eent,
               mutual_information=np.maximum(0.0, ent - eent), variation_ratio=1.0 - votes.max(axis=1, initial=0) / S if n else np.zeros(0),
               votes=votes, acc=acc, ambiguous_samples=amb_s)
    big = max([float(np.abs(out[q]).max(initial=0.0)) for q in ("mean_prob", "entropy", "expected_entropy")] + [1.0])
    out["K"] = TINY + 2 * k
    out["E"] = U * big + out["K"]
    amb_r = amb_s.any(axis=0)
    if C > 1 and n:
        order = np.argsort(-mp, axis=1, kind="stable")
        top, second = order[:, 0], order[:, 1]
        r = np.arange(n)
        close = mp[r, top] - mp[r, second] <= 2 * out["E"]
        # an exact tie — the lowest class wins on both sides — is no ambiguity: equal columns in every sample, or columns of
        # zeros and ones (one-hot samples), whose sums are exact in any order
        same = np.all(l[:, r, top] == l[:, r, second], axis=0)
        whole = np.all(np.isin(p[:, r, top], (0.0, 1.0)) & np.isin(p[:, r, second], (0.0, 1.0)), axis=0)
        amb_r |= close & ~same & ~whole
    out["ambiguous_rows"] = amb_r
    return out


def bound(ref, name):
    """per-entry bound of statistic `name` of statistics()'s dict"""
    return U * np.abs(ref[name]) + ref["K"]


# ------------------------------------------------------------------------------------------------------- the shared cases
def kernel_samples(n_table, C, S, seed=0):
    """S log-softmax tables [S, n_table, C] f32 with the planted rows of the kernel tests (when the table has room): row 0 an
    exact tie for the maximum in every sample (classes 0 and C - 1, the lowest must win), row 1 a column at -1e4, row 2 a column
    at -inf, row 3 one-hot (0 and -inf; the hot class changes with the sample)"""
    rng = np.random.default_rng(1000 * C + 10 * n_table + S + seed)
    z = rng.standard_normal((S, n_table, C)) * 3
    l = log_softmax(z.reshape(-1, C)).reshape(S, n_table, C).astype(np.float32)
    if n_table > 0 and C > 1:
        l[:, 0, C - 1] = l[:, 0, 0] = l[:, 0].max(axis=1) + np.float32(0.5)
    if n_table > 1 and C > 1:
        l[:, 1, C // 2] = -1e4
    if n_table > 2 and C > 1:
        l[:, 2, 0] = -np.inf
    if n_table > 3:
        for s in range(S):
            l[s, 3] = -np.inf
            l[s, 3, (s * 3) % C] = 0.0
    return l


def row_lists(n_table):
    """the row lists of the kernel tests: none, a permuted subset, a list with repeats"""
    rng = np.random.default_rng(n_table)
    sub = rng.permutation(n_table)[:max(1, 2 * n_table // 3)].astype(np.int32) if n_table else np.zeros(0, np.int32)
    return [None, sub, np.concatenate([sub, sub[::-1], sub[:1]]).astype(np.int32)]


MODEL_SEED = 11
MODEL_CASES = (("planted-dense", 0), ("planted-dense", "EDGE_COEF"), ("cora-syn", 0))   # (dataset, flags): dense X twice, sparse X
MODEL_RATES = (None, 0.25)                                     # None: the model's own (MODEL_DROPOUT)
MODEL_DROPOUT = 0.5
_DS = {}


def model_dataset(name):
    from cuda_gcn_amd import datagen
    if name not in _DS:
        _DS[name] = datagen.planted_communities(n_comm=7, size=131, p_in=0.5, feats=32, classes=7) if name == "planted-dense" \
            else datagen.make_dataset(name)
    return _DS[name]


def model_hidden(name):
    return 32 if name == "planted-dense" else 16


def model_weights(name):
    """planted weights (set_weights): the CPU tests know them without a GPU.  Scaled so that the logits spread over several units"""
    ds = model_dataset(name)
    F, h, C = ds["input_dim"], model_hidden(name), ds["output_dim"]
    rng = np.random.default_rng(F * 1000 + h)
    nnz_row = max(1.0, np.asarray(ds["f_val"]).size / ds["num_nodes"])
    w1 = (rng.standard_normal((F, h)) * (2.0 / np.sqrt(nnz_row))).astype(np.float32)
    w2 = (rng.standard_normal((h, C)) * (3.0 / np.sqrt(h))).astype(np.float32)
    return w1, w2
