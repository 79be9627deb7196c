"""Explaining a logit on the GPU, kernel level: csrc/explain.hip through ops.Device — bit for bit against an int64 numpy answer on
circulant graphs with small-integer tables, within the derived bounds of tests/explain_ref.py on real-valued ones (a random graph
with degrees 1..300, the irregular adjacency of tests/irregular_inputs.py, sparse X with empty rows), determinism, independence
of the other queries of a launch, abs_colsum, and the argument errors."""
import numpy as np
import pytest

from tests import explain_ref as R
from tests import irregular_inputs as irr

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_number_bits(got, want):
    """bit equality with an answer made from integers, which has no negative zero: a share that is w2 . 0 with w2 < 0 is -0.0 in
    IEEE arithmetic, and x + 0.0 maps it to +0.0 and every other value to itself"""
    return same_bits(np.asarray(got) + np.float32(0.0), want)


@pytest.fixture(scope="module")
def dev():
    from cuda_gcn_amd.ops import Device
    d = Device(0)
    yield d
    d.close()


# ---- exact cases -----------------------------------------------------------------------------------------------------------

N_EXACT = 150


def circulant(n, d):
    """every row i stores i + o for d fixed offsets (0 among them): all degrees d, so every coefficient is exactly 1 / d"""
    offs = np.array([0, 1, 5, n - 3] if d == 4 else [0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, n - 1, n - 2, n - 7, n - 20, n - 41])
    assert offs.size == d and np.unique(offs % n).size == d
    indices = ((np.arange(n)[:, None] + offs[None, :]) % n).astype(np.int32)
    return (np.arange(n + 1) * d).astype(np.int32), indices.reshape(-1)


def integer_net(seed, n, h, F, C):
    rng = np.random.default_rng(seed)
    h1 = rng.integers(1, 4, (n, h)) * (rng.random((n, h)) < 0.5)                  # about half zeros, else 1..3 (a ReLU output)
    return (h1.astype(np.int64), rng.integers(-2, 3, (n, F)).astype(np.int64), rng.integers(-2, 3, (F, h)).astype(np.int64),
            rng.integers(-2, 3, (h, C)).astype(np.int64))


def exact_answer(csr, d, q_row, q_class, h1, x, w1, w2):
    """the shares as integers over d (nbr, hid, logit) and d^2 (feat), from the stored order of `csr`; also sum |terms|"""
    indptr, indices, _ = csr
    n = indptr.size - 1
    cnt = np.zeros((n, n), np.int64)
    np.add.at(cnt, (np.repeat(np.arange(n), np.diff(indptr)), indices), 1)
    s_num, s_abs = cnt @ x, cnt @ np.abs(x)
    out = dict(logit=[], hidden=[], nbr_row=[], nbr_val=[], feat=[], mag=0.0)
    for v, c in zip(q_row, q_class):
        us = indices[indptr[v]:indptr[v + 1]].astype(np.int64)
        hu, w = h1[us], w2[:, c]
        nbr, hid = hu @ w, w * hu.sum(0)
        r = (hu > 0) * w[None, :]
        feat = ((r @ w1.T) * s_num[us]).sum(0)
        out["mag"] = max(out["mag"], float(((np.abs(r) @ np.abs(w1).T) * s_abs[us]).sum(0).max()) / d ** 2,
                         float((np.abs(hu) @ np.abs(w)).sum()) / d)
        out["logit"].append(nbr.sum() / d)
        out["hidden"].append(hid / d)
        out["nbr_row"].append(us)
        out["nbr_val"].append(nbr / d)
        out["feat"].append(feat / d ** 2)
    return dict(logit=np.array(out["logit"], np.float32), hidden=np.array(out["hidden"], np.float32),
                nbr_row=np.concatenate(out["nbr_row"]).astype(np.int32), nbr_val=np.concatenate(out["nbr_val"]).astype(np.float32),
                feat=np.array(out["feat"], np.float32), mag=out["mag"])


def queries(n, nq, C, seed):
    rng = np.random.default_rng(seed)
    q = rng.integers(0, n, nq).astype(np.int32)
    c = rng.integers(0, C, nq).astype(np.int32)
    c[0] = C - 1
    if nq > 1:
        q[-1], c[-1] = q[0], c[0]                                 # a repeated query
        c[1] = 0
    return q, c


@pytest.mark.parametrize("h", [1, 16, 41, 128, 256])
def test_shares_are_exact_on_integer_tables(dev, h):
    """Circulant graphs of row length 4 and 16 (coefficients 1/4, 1/16, dinv 1/2, 1/4: exact), H1 in {0..3} with about half zeros,
    X, W1, W2 in {-2..2}; every F, both scalings, nq and C cycling through their values, classes 0 and C - 1, a repeated query,
    strides that are and are not multiples of 4 with NaN padding.  Every intermediate is a multiple of 1/256 (r = w2 / d or
    w2 dinv, S = int / d, ...), so 256 . sum |terms| < 2^24 — asserted from the inputs — makes every f32 operation exact and the
    answer independent of the order of the sums; _agg and _walk on the same dense X must then give the same bits too."""
    n = N_EXACT
    combo = 0
    for d in (4, 16):
        indptr, indices = circulant(n, d)
        g = dev.graph(indptr, indices)
        csr = g.csr()
        assert np.all(np.diff(csr[0]) == d) and np.all(csr[2] == np.float32(1.0 / d))
        dinv = g.scales()[0]
        assert np.all(dinv == np.float32(1.0 / np.sqrt(d)))
        for F in (1, 7, 64, 130):
            nq, C = (1, 19, 67)[combo % 3], (1, 7, 41)[(combo // 2) % 3]
            h1, x, w1, w2 = integer_net(1000 * h + combo, n, h, F, C)
            q, c = queries(n, nq, C, combo)
            want = exact_answer(csr, d, q, c, h1, x, w1, w2)
            assert 256 * want["mag"] < 2 ** 24
            cnt = np.zeros((n, n), np.int64)
            np.add.at(cnt, (np.repeat(np.arange(n), d), csr[1]), 1)
            s = (cnt @ x) / d                                                     # A^ . X, exact in f32
            x_ip = (np.arange(n + 1) * F).astype(np.int32)
            x_ix = np.tile(np.arange(F, dtype=np.int32), n)
            for scaling in (0, 1):
                pad = (combo // 2 + scaling) % 2 == 0             # both kinds of stride under both scalings, F by F
                ld = (lambda w: (w + 3) // 4 * 4 + 4) if pad else (lambda w: w // 4 * 4 + 5)       # a multiple of 4; never one
                f = dinv[:, None] if scaling else 1.0
                got = dev.explain_hops(g, q, c, h1 * f, w2, scaling=scaling, ld_h1=ld(h), ld_w2=ld(C), ld_out=ld(h))
                what = (d, F, nq, C, scaling, pad)
                assert same_number_bits(got["logit"], want["logit"]), what
                assert same_number_bits(got["hidden"], want["hidden"]), what
                assert np.array_equal(got["nbr_row"], want["nbr_row"]) and same_number_bits(got["nbr_val"], want["nbr_val"]), what
                agg = dev.explain_features_agg(g, q, c, h1 * f, w2, w1, s * f, scaling=scaling, ld_h1=ld(h), ld_w2=ld(C), ld_w1=ld(h), ld_s=ld(F), ld_f=ld(F))
                assert same_number_bits(agg, want["feat"]), what
                xf = dev.feat(x_ip, x_ix, (x * f).astype(np.float32).reshape(-1), F)
                assert xf.dense
                walk = dev.explain_features_walk(g, xf, q, c, h1 * f, w2, w1, scaling=scaling, ld_h1=ld(h), ld_w2=ld(C), ld_w1=ld(h), ld_f=ld(F))
                xf.free()
                assert same_number_bits(walk, want["feat"]) and same_bits(walk + np.float32(0.0), agg + np.float32(0.0)), what
                combo += 1
        g.free()


# ---- real values -------------------------------------------------------------------------------------------------------------

def real_net(rng, n, h, F, C, x_dense):
    w1 = (rng.standard_normal((F, h)) / np.sqrt(F)).astype(np.float32)
    w2 = (rng.standard_normal((h, C)) / np.sqrt(h)).astype(np.float32)
    return w1, w2


def check_real(dev, indptr, indices, x64, x_abs, x_count, x_csr, h, C, seed, q_rows, features_agg=True):
    """both scalings of every kernel on one graph against the float64 reference: H1 = f32(ReLU(S W1)) of the f32 S table, so the
    gates are those of a forward"""
    rng = np.random.default_rng(seed)
    g = dev.graph(indptr, indices)
    csr = g.csr()
    n, F = x64.shape
    dinv = g.scales()[0].astype(np.float64)
    src = np.repeat(np.arange(n), np.diff(csr[0]))
    w1, w2 = real_net(rng, n, h, F, C, x64)
    q = np.asarray(q_rows, np.int32)
    c = rng.integers(0, C, q.size).astype(np.int32)
    c[0], c[-1] = C - 1, 0
    for scaling in (0, 1):
        coef = csr[2].astype(np.float64) if scaling == 0 else dinv[src] * dinv[csr[1]]
        s, s_abs, terms = R.layer1(csr[0], csr[1], coef, x64, x_abs, x_count)
        s32 = s.astype(np.float32)
        h1 = np.maximum(s32 @ w1, 0).astype(np.float32)
        if scaling:                                               # the tables the kernel is given carry dinv; the reference's are what they hold
            h1_t, s_t = (h1 * dinv[:, None]).astype(np.float32), (s32 * dinv[:, None]).astype(np.float32)
            h1_ref, s_ref = h1_t / dinv[:, None], s_t / dinv[:, None]
        else:
            h1_t, s_t, h1_ref, s_ref = h1, s32, h1.astype(np.float64), s32.astype(np.float64)
        hops = dev.explain_hops(g, q, c, h1_t, w2, scaling=scaling, ld_h1=h + 1, ld_w2=C + 2, ld_out=h + 3)
        hops2 = dev.explain_hops(g, q, c, h1_t, w2, scaling=scaling, ld_h1=h + 1, ld_w2=C + 2, ld_out=h + 3)
        assert all(same_bits(hops[k], hops2[k]) for k in ("logit", "hidden", "nbr_row", "nbr_val"))
        feats = {}
        if features_agg:
            feats["agg"] = dev.explain_features_agg(g, q, c, h1_t, w2, w1, s_t, scaling=scaling, ld_h1=h + 1, ld_w2=C + 2, ld_w1=h + 1, ld_s=F + 1, ld_f=F + 2)
            again = dev.explain_features_agg(g, q, c, h1_t, w2, w1, s_t, scaling=scaling, ld_h1=h + 1, ld_w2=C + 2, ld_w1=h + 1, ld_s=F + 1, ld_f=F + 2)
            assert same_bits(feats["agg"], again)
        if x_csr is not None:
            xp, xi, xv = x_csr
            row_of = np.repeat(np.arange(n), np.diff(xp))
            vals = (xv * dinv[row_of]).astype(np.float32) if scaling else xv
            xf = dev.feat(xp, xi, vals, F)
            feats["walk"] = dev.explain_features_walk(g, xf, q, c, h1_t, w2, w1, scaling=scaling, ld_h1=h + 1, ld_w2=C + 2, ld_w1=h + 1, ld_f=F + 2)
            again = dev.explain_features_walk(g, xf, q, c, h1_t, w2, w1, scaling=scaling, ld_h1=h + 1, ld_w2=C + 2, ld_w1=h + 1, ld_f=F + 2)
            xf.free()
            assert same_bits(feats["walk"], again)
        worst = {}
        for i, (v, cls) in enumerate(zip(q, c)):
            a, b = int(hops["nbr_ptr"][i]), int(hops["nbr_ptr"][i + 1])
            for name, feat in feats.items():
                s_use = s_ref if name == "agg" else s             # _agg is given the f32 table; the walk starts from X itself
                ref = R.explain64(csr[0], csr[1], coef, h1_ref, w2, int(v), int(cls), w1=w1, s=s_use, s_abs=s_abs, terms=terms)
                got = dict(rows=hops["nbr_row"][a:b], logit=hops["logit"][i], nbr=hops["nbr_val"][a:b], hid=hops["hidden"][i],
                           feat=None if feat is None else feat[i])
                assert R.violations(got, ref, features=feat is not None) == [], (scaling, name, int(v), int(cls))
                assert R.sum_violations(got, ref, features=feat is not None) == [], (scaling, name, int(v), int(cls))
                if feat is not None:
                    worst[name] = max(worst.get(name, 0.0), float(np.max(np.abs(feat[i] - ref["feat"]) / np.maximum(ref["E_feat"], 1e-300))))
        print(f"scaling {scaling}: worst |feat - ref| / E_feat {worst}")
        # one query alone equals the same query inside the batch
        j = q.size // 2
        one = dev.explain_hops(g, q[j:j + 1], c[j:j + 1], h1_t, w2, scaling=scaling, ld_h1=h + 1, ld_w2=C + 2, ld_out=h + 3)
        a, b = int(hops["nbr_ptr"][j]), int(hops["nbr_ptr"][j + 1])
        assert same_bits(one["logit"], hops["logit"][j:j + 1]) and same_bits(one["hidden"], hops["hidden"][j:j + 1])
        assert same_bits(one["nbr_val"], hops["nbr_val"][a:b]) and np.array_equal(one["nbr_row"], hops["nbr_row"][a:b])
        if features_agg:
            one = dev.explain_features_agg(g, q[j:j + 1], c[j:j + 1], h1_t, w2, w1, s_t, scaling=scaling, ld_h1=h + 1, ld_w2=C + 2, ld_w1=h + 1, ld_s=F + 1, ld_f=F + 2)
            assert same_bits(one, feats["agg"][j:j + 1])
    g.free()


def random_graph(rng, n):
    """degrees 1..300: row 0 has the self loop only, row 1 has 300 stored entries (above the kernels' chunk of 16 and the four
    waves of the neighbour pass), the rest 2..40, some one-way, some repeated"""
    rows = []
    for i in range(n):
        k = 0 if i == 0 else (299 if i == 1 else int(rng.integers(1, 40)))
        nb = rng.integers(0, n, k)
        if k > 3 and i % 7 == 0:
            nb[2] = nb[0]
        rows.append(np.concatenate([[i], nb]))
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum([r.size for r in rows])
    return indptr.astype(np.int32), np.concatenate(rows).astype(np.int32)


def dense_csr(x):
    n, F = x.shape
    return (np.arange(n + 1) * F).astype(np.int32), np.tile(np.arange(F, dtype=np.int32), n), x.astype(np.float32).reshape(-1)


@pytest.mark.parametrize("h,F", [(16, 33), (100, 70)])
def test_real_values_on_a_random_graph(dev, h, F):
    rng = np.random.default_rng(h)
    n = 1000
    indptr, indices = random_graph(rng, n)
    assert np.diff(indptr).min() == 1 and np.diff(indptr).max() == 300
    x = (rng.standard_normal((n, F)) * (rng.random((n, F)) < 0.7)).astype(np.float32)
    q = np.concatenate([[0, 1], rng.integers(0, n, 17), [1]])
    check_real(dev, indptr, indices, x.astype(np.float64), None, None, dense_csr(x), h, 7, h + 1, q)


def test_real_values_on_irregular_edges(dev):
    """one-way and repeated edges, rows that list themselves again, a row listing one neighbour 300 times, the hub of 2 500"""
    indptr, indices = irr.gpu_graph()
    n = indptr.size - 1
    rng = np.random.default_rng(5)
    F = 20
    x = rng.standard_normal((n, F)).astype(np.float32)
    lens = np.diff(indptr)
    q = np.concatenate([[0, 1, 2, int(np.flatnonzero(lens == 1)[0])], rng.integers(0, n, 12)])
    check_real(dev, indptr, indices, x.astype(np.float64), None, None, None, 24, 5, 6, q)


def test_real_values_on_sparse_features_with_empty_rows(dev):
    rng = np.random.default_rng(11)
    n, F = 400, 67
    indptr, indices = random_graph(rng, n)
    rows = []
    for i in range(n):
        k = 0 if i % 9 == 0 or i == n - 1 else int(rng.integers(1, 9))
        rows.append(rng.choice(F, k, replace=False))
    xp = np.zeros(n + 1, np.int64)
    xp[1:] = np.cumsum([r.size for r in rows])
    xi = np.concatenate(rows).astype(np.int32)
    xv = rng.standard_normal(xi.size).astype(np.float32)
    x64 = irr.dense_features(xp, xi, xv, F)
    q = np.concatenate([[0, 1], rng.integers(0, n, 10)])
    check_real(dev, indptr, indices, x64, None, None, (xp.astype(np.int32), xi, xv), 16, 6, 12, q, features_agg=False)


# ---- abs_colsum, argument errors ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C,F", [(1, 1), (7, 67), (41, 130), (256, 64)])
def test_abs_colsum_is_exact_over_two_batches(dev, C, F):
    rng = np.random.default_rng(C)
    batches, want, count = [], np.zeros((C, F), np.float64), np.zeros(C, np.int64)
    for nq in (19, 67):
        feat = rng.integers(-50, 51, (nq, F)).astype(np.float32) / 8
        cls = rng.integers(0, C, nq).astype(np.int32)
        cls[0] = C - 1
        np.add.at(want, cls, np.abs(feat.astype(np.float64)))
        np.add.at(count, cls, 1)
        batches.append((feat, cls))
    acc, cnt = dev.explain_abs_colsum(batches, C, ld_f=F + 3)
    assert same_bits(acc, want) and np.array_equal(cnt, count)
    acc2, cnt2 = dev.explain_abs_colsum(batches, C, ld_f=F + 3)
    assert same_bits(acc, acc2) and np.array_equal(cnt, cnt2)


def test_argument_errors_come_before_any_launch(dev):
    from cuda_gcn_amd.ops import GcnHipError
    n, d = 40, 4
    indptr = (np.arange(n + 1) * d).astype(np.int32)
    indices = ((np.arange(n)[:, None] + np.array([0, 1, 2, 3])) % n).astype(np.int32).reshape(-1)
    g = dev.graph(indptr, indices)
    h1, w2, w1, s = np.ones((n, 8), np.float32), np.ones((8, 3), np.float32), np.ones((5, 8), np.float32), np.ones((n, 5), np.float32)
    xf = dev.feat(*dense_csr(s), 5)
    for rows, cls, why in (([0, n], [0, 0], "query row"), ([0, -1], [0, 0], "query row"), ([0, 1], [0, 3], "query class"), ([0, 1], [-1, 0], "query class")):
        with pytest.raises(GcnHipError, match=why):
            dev.explain_hops(g, rows, cls, h1, w2)
        with pytest.raises(GcnHipError, match=why):
            dev.explain_features_agg(g, rows, cls, h1, w2, w1, s)
        with pytest.raises(GcnHipError, match=why):
            dev.explain_features_walk(g, xf, rows, cls, h1, w2, w1)
    with pytest.raises(GcnHipError, match="query class"):
        dev.explain_abs_colsum([(np.ones((2, 5), np.float32), [0, 3])], 3)
    with pytest.raises(GcnHipError, match="C <= 256"):
        dev.explain_abs_colsum([(np.ones((2, 5), np.float32), [0, 1])], 257)
    with pytest.raises(GcnHipError, match="h <= 256"):
        dev.explain_hops(g, [0], [0], np.ones((n, 257), np.float32), np.ones((257, 3), np.float32))
    with pytest.raises(GcnHipError, match="scaling"):
        dev.explain_hops(g, [0], [0], h1, w2, scaling=2)
    with pytest.raises(GcnHipError, match="exclusive scan"):
        dev.explain_hops(g, [0, 1], [0, 0], h1, w2, nbr_ptr=[0, 3, 8])
    # the accepted call still works afterwards, and an empty query list is no error
    ok = dev.explain_hops(g, [0, 1], [0, 2], h1, w2)
    assert ok["logit"].shape == (2,) and np.all(ok["logit"] == 8.0)
    assert dev.explain_hops(g, [], [], h1, w2)["logit"].shape == (0,)
    xf.free()
    g.free()
