"""Float64 reference for the explanation kernels (csrc/explain.hip) and the acceptance rule their answers are held to.

One query is a row v of the adjacency and a class c.  e_1 .. e_d are the stored edges of row v in stored order, u_i = col(e_i),
a_i the coefficient of e_i, g_i[k] = (H1[u_i, k] > 0), S = A^ . X:

    logit  z      = sum_i a_i sum_k H1[u_i, k] W2[k, c]
    nbr_i         = a_i sum_k H1[u_i, k] W2[k, c]
    hid_k         = W2[k, c] sum_i a_i H1[u_i, k]
    feat_f        = sum_i a_i sum_k g_i[k] W2[k, c] W1[f, k] S[u_i, f]

Everything here works from the inputs — the CSR as the device object stores it, one float64 coefficient per stored edge, plain
(unscaled) H1, W1, W2 and X — and never from a kernel's output.  For the factored form the caller passes a_e = dinv[v] . dinv[u]
and H1 = H1' / dinv (both in float64 from the f32 numbers the kernel is given), which are the same real numbers.

The bounds.  u = 2^-24 (half an ulp of f32, relative); all sums of absolute values are formed in float64.

    E_nbr_i  = (h + 8) u |a_i| sum_k |H1[u_i, k] W2[k, c]|
    E_hid_k  = (d + 8) u |W2[k, c]| sum_i |a_i H1[u_i, k]|
    E_logit  = (d + h + 8) u sum_i sum_k |a_i H1[u_i, k] W2[k, c]|
    E_feat_f = (d + h + D + 32) u sum_i |a_i| sum_k g_i[k] |W2[k, c] W1[f, k]| . sum_w |A^[u_i, w] x(w, f)|

Where they come from (first order in u; the constants 8 and 32 hold the second-order terms, (n u)^2 < u for n <= 4096 terms):
  * a sum of n f32 products formed in ANY order carries at most n u sum |terms|: each product rounds once (or not at all under
    fma), each of the at most n - 1 additions once.  nbr_i is such a sum over k (h terms) times a_i (one rounding; in the
    factored form a_i is dinv[v] and the table row already carries dinv[u_i]): h + 1.  hid_k is a sum over i (d terms), one
    multiply by W2[k, c] and, factored, one by dinv[v]: d + 2.  The logit is a sum of the h values hid_k: (d + 2) + h.
  * feat_f: r_i[k] = a_i g W2[k, c] rounds once; t_i = sum_k r_i[k] W1[f, k] is a sum of h terms; S[u_i, f] t_i rounds once and
    the sum over i has d terms: d + h + 2 relative to sum_i |a_i| sum_k g |W2 W1| |S[u_i, f]|.  S[u_i, f] itself is an f32 sum
    of the row's stored terms A^[u_i, w] x(w, f) — at most D of them, D = the longest stored row among the u_i, each term one or
    two products (factored: dinv2[u_i] . (dinv[w] x), with dinv2 = f32(1 / deg) within 2 u of dinv^2) — so |S - S_exact| <=
    (D + 4) u sum_w |A^ x|, and |S| <= sum_w |A^ x| turns the first part into the same magnitude: d + h + D + 6, the rest of
    the 32 is slack.  The two-hop walk adds the same terms nested the same way (a neighbour's inner sum first), so the same
    count holds.  A feature row that stores one column several times has that many terms per stored edge: D is then the largest
    number of stored terms of one (u_i, f), never less than the longest row.
  * sums of shares: sum_i nbr_i, sum_k hid_k (added in float64 by the test) against the returned logit differ by at most
    sum E + E_logit, both being approximations of the same z.  sum_f feat_f equals z only up to the first layer's own rounding:
    the forward's H1 is f32(S . W1), not S . W1; its distance, measured in float64 from the inputs as
    sum_i |a_i| sum_k g |W2[k, c]| . |H1[u_i, k] - (S W1)[u_i, k]|, is added to sum_f E_feat_f + E_logit.

  * a logit against a float64 forward FROM X (first_layer_bound): the forward's hidden value is f32(ReLU(sum_f S[u, f] W1[f, k]))
    with S itself an f32 sum.  The product sum has F terms (F u sum_f |S W1|), S[u, f] carries (D_u + 4) u sum_w |A^ x| as above
    (D_u = the stored length of row u), and ReLU is 1-Lipschitz, so it neither enlarges the error nor lets a gate that flips
    near zero cost more than the error itself:  |H1[u, k] - ReLU(S W1)[u, k]| <= E_h1[u, k] = (F + D_u + 8) u sum_f S_abs[u, f]
    |W1[f, k]| (4 u of the 8 is slack).  A logit computed from the stored H1 then differs from the float64 forward's by at most
    E_logit + sum_i |a_i| sum_k |W2[k, c]| E_h1[u_i, k].

The acceptance rule for one query: the neighbour ids are the stored row, entry by entry; every share is within its E of the
float64 value; the logit within E_logit.
"""
import numpy as np

U = 2.0 ** -24


def layer1(indptr, indices, coef, x, x_abs=None, x_count=None):
    """(S, S_abs, terms) float64 [n, F]: S = A^ . X from the stored edges (a repeated edge adds twice), the same product on
    absolute values, and the number of stored terms per (row, column); x dense [n, F]; x_abs / x_count: |stored values| summed
    and stored entries counted per cell when X stores a column more than once in a row (default: |x|, x != 0)."""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    n = indptr.size - 1
    x = np.asarray(x, np.float64)
    src = np.repeat(np.arange(n), np.diff(indptr))
    a = np.zeros((n, x.shape[0]), np.float64)
    a_abs, a_cnt = a.copy(), a.copy()
    c = np.asarray(coef, np.float64)
    np.add.at(a, (src, indices), c)
    np.add.at(a_abs, (src, indices), np.abs(c))
    np.add.at(a_cnt, (src, indices), 1.0)
    x_abs = np.abs(x) if x_abs is None else np.asarray(x_abs, np.float64)
    x_count = (x != 0).astype(np.float64) if x_count is None else np.asarray(x_count, np.float64)
    return a @ x, a_abs @ x_abs, a_cnt @ x_count


def first_layer_bound(s_abs, w1, row_lengths):
    """E_h1 [n, h]: the bound of |H1 - ReLU(S W1)| for a hidden layer computed in f32 from X (the docstring has the chain);
    s_abs: layer1()'s second value, row_lengths: the stored length of every row of the adjacency"""
    w1 = np.asarray(w1, np.float64)
    return (w1.shape[0] + np.asarray(row_lengths, np.float64)[:, None] + 8) * U * (np.asarray(s_abs, np.float64) @ np.abs(w1))


def explain64(indptr, indices, coef, h1, w2, v, c, w1=None, s=None, s_abs=None, terms=None, gate_from=None, row_lengths=None):
    """The float64 shares of query (v, c) and their bounds: dict(rows, logit, nbr, hid, feat, E_logit, E_nbr, E_hid, E_feat,
    layer1_gap).  feat needs w1 [F, h] and layer1()'s S, S_abs (and terms for D).  gate_from: another H1 to take the gates from
    (the acceptance tests use it to build a wrong answer).  row_lengths: the stored length of every row of the adjacency, for D,
    when (indptr, indices) holds the queried rows only (default: np.diff(indptr))."""
    indptr = np.asarray(indptr, np.int64)
    e0, e1 = int(indptr[v]), int(indptr[v + 1])
    us = np.asarray(indices, np.int64)[e0:e1]
    a = np.asarray(coef, np.float64)[e0:e1]
    hu = np.asarray(h1, np.float64)[us]
    w = np.asarray(w2, np.float64)[:, c]
    d, h = hu.shape
    t = a[:, None] * hu * w[None, :]
    ta = np.abs(t)
    out = dict(rows=us.astype(np.int32), logit=t.sum(), nbr=t.sum(1), hid=t.sum(0), E_logit=(d + h + 8) * U * ta.sum(),
               E_nbr=(h + 8) * U * ta.sum(1), E_hid=(d + 8) * U * ta.sum(0), feat=None, E_feat=None, layer1_gap=None)
    if w1 is not None:
        w1 = np.asarray(w1, np.float64)
        gate = (np.asarray(h1 if gate_from is None else gate_from)[us] > 0)
        r = a[:, None] * gate * w[None, :]
        su, sa = np.asarray(s, np.float64)[us], np.asarray(s_abs, np.float64)[us]
        lens = (np.diff(indptr) if row_lengths is None else np.asarray(row_lengths))[us]
        big_d = int(lens.max()) if d else 0
        if terms is not None and d:
            big_d = max(big_d, int(np.asarray(terms)[us].max()))
        out["feat"] = ((r @ w1.T) * su).sum(0)
        out["E_feat"] = (d + h + big_d + 32) * U * ((np.abs(r) @ np.abs(w1).T) * sa).sum(0)
        out["layer1_gap"] = float((np.abs(r) * np.abs(np.where(gate, hu - su @ w1, 0.0))).sum())
    return out


def explain_f32(indptr, indices, coef, h1, w2, v, c, w1=None, s=None):
    """The same definition carried out in float32 numpy: dict(rows, logit, nbr, hid, feat)"""
    f = np.float32
    indptr = np.asarray(indptr, np.int64)
    e0, e1 = int(indptr[v]), int(indptr[v + 1])
    us = np.asarray(indices, np.int64)[e0:e1]
    a = np.asarray(coef, f)[e0:e1]
    hu = np.asarray(h1, f)[us]
    w = np.asarray(w2, f)[:, c]
    nbr = (a * (hu * w[None, :]).sum(1, dtype=f)).astype(f)
    hid = (w * (a[:, None] * hu).sum(0, dtype=f)).astype(f)
    out = dict(rows=us.astype(np.int32), logit=hid.sum(dtype=f), nbr=nbr, hid=hid, feat=None)
    if w1 is not None:
        r = (a[:, None] * w[None, :] * (hu > 0)).astype(f)
        out["feat"] = ((r @ np.asarray(w1, f).T) * np.asarray(s, f)[us]).sum(0, dtype=f)
    return out


def violations(got, ref, features=True):
    """what the acceptance rule finds wrong with one query's answer `got` (dict(rows, logit, nbr, hid, feat)); [] = accepted"""
    bad = []
    rows = np.asarray(got["rows"])
    if rows.shape != ref["rows"].shape or not np.array_equal(rows, ref["rows"]):
        return ["the neighbour ids are not the stored row"]
    for name, err in (("nbr", "E_nbr"), ("hid", "E_hid")):
        x = np.asarray(got[name], np.float64)
        if x.shape != ref[name].shape or not np.all(np.abs(x - ref[name]) <= ref[err]):
            bad.append(f"{name}: max excess {np.max(np.abs(x - ref[name]) - ref[err]) if x.shape == ref[name].shape else 'shape'}")
    if not abs(float(got["logit"]) - ref["logit"]) <= ref["E_logit"]:
        bad.append(f"logit: off by {abs(float(got['logit']) - ref['logit'])} > {ref['E_logit']}")
    if features:
        x = np.asarray(got["feat"], np.float64)
        if x.shape != ref["feat"].shape or not np.all(np.abs(x - ref["feat"]) <= ref["E_feat"]):
            bad.append(f"feat: max excess {np.max(np.abs(x - ref['feat']) - ref['E_feat']) if x.shape == ref['feat'].shape else 'shape'}")
    return bad


def sum_violations(got, ref, features=True):
    """the shares of `got` add up to its logit within the stated sum bounds; [] = accepted"""
    bad = []
    z = float(got["logit"])
    for name, err in (("nbr", "E_nbr"), ("hid", "E_hid")):
        gap, bound = abs(np.asarray(got[name], np.float64).sum() - z), ref[err].sum() + ref["E_logit"]
        if not gap <= bound:
            bad.append(f"sum {name}: {gap} > {bound}")
    if features:
        gap, bound = abs(np.asarray(got["feat"], np.float64).sum() - z), ref["E_feat"].sum() + ref["E_logit"] + ref["layer1_gap"]
        if not gap <= bound:
            bad.append(f"sum feat: {gap} > {bound}")
    return bad


def top_feature_agreement(feats, refs, expected):
    """What the feature shares are for.  feats [n, F] (None: the reference's own), refs: explain64 dicts, expected [n]: the column
    each query should rank first.  -> (share of queries whose largest reference share is `expected`, share of OPEN queries — the
    two top reference shares closer than 2 (E_a + E_b) —, and whether feats' argmax equals the reference's on every other query)"""
    hit = opened = 0
    agree = True
    for i, ref in enumerate(refs):
        order = np.argsort(-ref["feat"], kind="stable")
        a, b = order[0], order[1]
        hit += int(a == expected[i])
        is_open = ref["feat"][a] - ref["feat"][b] <= 2 * (ref["E_feat"][a] + ref["E_feat"][b])
        opened += int(is_open)
        if feats is not None and not is_open and int(np.argmax(feats[i])) != int(a):
            agree = False
    return hit / len(refs), opened / len(refs), agree
