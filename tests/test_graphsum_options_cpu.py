"""tests/graphsum_ref.py before a GPU sees it: the float64 restatement of one GraphSum call against the dense product the
irregular-input tests use, against the CPU oracle, and against itself through the identities the option table relies on
(factored coefficients, accumulate over complementary column restrictions); and the planted graph's promised degrees and
segment counts."""
import numpy as np
import pytest

from tests import irregular_inputs as irr
from tests.graphsum_ref import HUB_DEGREES, SPLIT, dinv_f32, graphsum_ref, keep_decisions, pack_positive, planted_graph, planted_row_sets, segments

EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def planted():
    return planted_graph()


def x_of(n, dim, seed=0):
    return np.random.default_rng(100 + dim + seed).standard_normal((n, dim)).astype(np.float32)


def test_planted_graph_has_the_degrees_and_segments_it_promises(planted):
    gp, gi, hubs = planted
    n = gp.size - 1
    deg = np.diff(gp)
    assert 380 <= n <= 420
    assert tuple(deg[hubs]) == HUB_DEGREES
    is_hub = np.zeros(n, bool); is_hub[hubs] = True
    for h in hubs:                                                   # a hub is wired to leaves only: its degree is exact
        nb = gi[gp[h]:gp[h + 1]]
        assert nb[0] == h and not is_hub[nb[1:]].any() and np.unique(nb).size == nb.size
    assert np.all(deg[-6:] == 1) and np.all(gi[gp[-7:-1]] == np.arange(n - 6, n))     # self loop only
    ns = segments(gp, SPLIT)
    assert tuple(ns[hubs]) == (1, 2, 3, 4, 4, 5, 6, 7, 8, 9, 10, 19)
    assert set(range(1, 10)) <= set(ns.tolist())                     # every tail length of gs_segment_sum, with and without a batch of four
    assert np.all(segments(gp, 10 ** 6) == 1)
    ra, rb, nz = planted_row_sets(gp, hubs)                          # the row selections of the GPU table
    h65, h300 = hubs[HUB_DEGREES.index(65)], hubs[HUB_DEGREES.index(300)]
    assert ra[h65] and ra[h300] and not rb[h65] and not rb[h300] and nz[h300]
    assert set(ns[ra].tolist()) >= {1, 2, 3, 4, 5, 7, 9, 19} and set(ns[rb].tolist()) >= {1, 2, 3, 4, 6, 8, 10}
    assert (ns[~ra] > 1).any() and (ns[~rb] > 1).any()
    assert 0.3 < ra.mean() < 0.5 and 0.4 < rb.mean() < 0.6 and 0.5 < nz.mean() < 0.7
    a = irr.dense_adjacency(gp, gi)
    assert np.array_equal(a, a.T) and np.all(np.diag(a) > 0)         # symmetric, self loops stored


@pytest.mark.parametrize("dim", [1, 7, 41, 128])
def test_all_options_off_is_the_dense_product_and_the_oracle(planted, oracle, dim):
    from tests.test_ops_gpu import close_mag
    gp, gi, _ = planted
    n = gp.size - 1
    x = x_of(n, dim)
    want, mag, touched = graphsum_ref(gp, gi, x)
    a = irr.dense_adjacency(gp, gi)
    assert np.array_equal(want, a @ x.astype(np.float64)) and np.array_equal(mag, a @ np.abs(x).astype(np.float64))
    assert touched.all()
    close_mag(oracle.graphsum(gp, gi, x, dim), want, mag)


@pytest.mark.parametrize("dim", [3, 64])
def test_factored_scalings_reproduce_the_per_edge_operator(planted, dim):
    gp, gi, _ = planted
    n = gp.size - 1
    x = x_of(n, dim).astype(np.float64)
    deg = np.diff(gp).astype(np.float64)
    dr, dr2 = dinv_f32(gp)
    assert np.array_equal(dr, (1 / np.sqrt(deg)).astype(np.float32)) and np.array_equal(dr2, (1 / deg).astype(np.float32))
    want, mag, _ = graphsum_ref(gp, gi, x)
    xs = x / np.sqrt(deg)[:, None]                                   # x . dinv_col in float64
    tol = 4 * EPS * mag + 1e-300                                     # the f32 factors are half an ulp from 1/sqrt(deg), 1/deg
    s1 = graphsum_ref(gp, gi, xs, scaling=1)[0]
    s2 = graphsum_ref(gp, gi, xs, scaling=2)[0] * np.sqrt(deg)[:, None]
    s3 = graphsum_ref(gp, gi, xs, scaling=3)[0] / np.sqrt(deg)[:, None]
    assert np.all(np.abs(s1 - want) <= tol) and np.all(np.abs(s2 - want) <= tol)
    assert np.all(np.abs(s3 - want) <= 1e-12 * mag + 1e-300)         # no f32 factor: float64 rounding only
    p = x_of(n, dim, 9).astype(np.float64)                           # accumulate adds before the factor
    got = graphsum_ref(gp, gi, xs, scaling=1, accumulate=1, prev=p)[0]
    assert np.allclose(got, (p + graphsum_ref(gp, gi, xs, scaling=3)[0]) * dr.astype(np.float64)[:, None], rtol=1e-14, atol=0)


def test_accumulate_over_complementary_columns_is_the_whole_operator(planted):
    gp, gi, _ = planted
    n = gp.size - 1
    x = x_of(n, 16)
    own = np.random.default_rng(3).random(n) < 0.5
    nz = np.random.default_rng(4).random(n) < 0.7
    for kw in (dict(), dict(in_row_bits=nz), dict(scaling=1)):
        whole, mag, _ = graphsum_ref(gp, gi, x, **kw)
        first = graphsum_ref(gp, gi, x, keep_cols=own, **dict(kw, scaling=3 if kw.get("scaling") else 0))[0]
        both, mag2, _ = graphsum_ref(gp, gi, x, keep_cols=~own, accumulate=1, prev=first, **kw)
        assert np.all(np.abs(both - whole) <= 1e-13 * mag + 1e-300)
        assert np.all(mag2 <= mag * (1 + 1e-13) + 1e-300)            # |prev| is the first part's |sum|, at most its sum of |terms|


def test_epilogue_rows_and_bits(planted):
    gp, gi, hubs = planted
    n = gp.size - 1
    dim = 32
    x = x_of(n, dim)
    base = graphsum_ref(gp, gi, x)[0]
    rows = np.random.default_rng(1).random(n) < 0.4
    ob = np.random.default_rng(2).random(n) < 0.6
    relu, _, touched = graphsum_ref(gp, gi, x, relu_dropout=1, rows=rows, out_row_bits=ob)
    assert np.array_equal(touched, rows & ob)
    assert np.array_equal(relu, np.where(touched[:, None], np.maximum(base, 0), 0))
    km = (np.random.default_rng(3).random((n, dim)) < 0.5).astype(np.uint8)
    got, mag, _ = graphsum_ref(gp, gi, x, relu_dropout=1, training=1, p=0.3, keep_mask=km)
    scale = float(np.float32(1) / (np.float32(1) - np.float32(0.3)))
    assert np.array_equal(got, np.where(km != 0, np.maximum(base, 0) * scale, 0))
    assert np.array_equal(mag, graphsum_ref(gp, gi, x)[1] * scale)
    for off in (0, 77):                                              # the Philox stream: reproducible, offset moves it, p = 0.3 keeps ~70 %
        k = keep_decisions(n, dim, 1, 0.3, seed=11, epoch=2, elem_offset=off)
        assert np.array_equal(k, keep_decisions(n, dim, 1, 0.3, seed=11, epoch=2, elem_offset=off)) and 0.65 < k.mean() < 0.75
    assert np.array_equal(keep_decisions(n, dim, 1, 0.3, seed=11, epoch=2, elem_offset=77).reshape(-1)[:-77],
                          keep_decisions(n, dim, 1, 0.3, seed=11, epoch=2, elem_offset=0).reshape(-1)[77:])
    w = pack_positive(relu.astype(np.float32))
    assert w.shape == (n, 1) and all(((int(w[r, 0]) >> c) & 1) == (relu[r, c] > 0) for r in hubs[:3] for c in range(dim))
