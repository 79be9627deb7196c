"""gcnhip_attach_gather (csrc/attach.hip) through ops.Device: the gather of rows that are not rows of an adjacency object, from
two tables, against a float64 gather; its ReLU and predict epilogues; bit identity across launches, batches and row order; both
load paths (16-byte pieces, 4 bytes at a time)."""
import numpy as np
import pytest

from tests.test_ops_gpu import close_mag, EPS

pytestmark = pytest.mark.gpu

N_A = 300
HUB = 5000                         # entries of the hub row, over 200 distinct columns
KINDS = ["hub", "empty", "one", "wave+1", "own", "only_b", "mixed", "at_long", "past_long", "wave", "two_waves"]


@pytest.fixture(scope="module")
def dev():
    from cuda_gcn_amd.ops import Device
    d = Device(0)
    yield d
    d.close()


def make_rows(m, seed):
    """m rows over columns [0, N_A + m): row i is of kind KINDS[i % len(KINDS)] (so m = 1 is the hub alone, a block with one row
    whose sum takes all four waves), and the last row of a batch of more than one is a second hub (a block that is not full)"""
    rng = np.random.default_rng(seed)
    both = N_A + m
    rows, kinds = [], []
    for i in range(m):
        kind = "hub" if (m > 1 and i == m - 1) else KINDS[i % len(KINDS)]
        if kind == "hub":
            r = rng.choice(rng.permutation(both)[:min(200, both)], HUB)
        elif kind == "empty":
            r = np.zeros(0, np.int64)
        elif kind == "one":
            r = rng.integers(0, N_A, 1)
        elif kind == "wave+1":
            r = rng.integers(0, both, 65)                   # one past a wave chunk, both tables
        elif kind == "own":
            r = np.concatenate([[N_A + i], rng.integers(0, both, 6), [N_A + i]])      # its own table_b row, twice
        elif kind == "only_b":
            r = N_A + rng.integers(0, m, 9)
        elif kind == "mixed":
            r = rng.integers(0, both, rng.integers(2, 41))
        elif kind == "at_long":
            r = rng.integers(0, both, 512)                  # the longest row one wave sums
        elif kind == "past_long":
            r = rng.integers(0, both, 513)                  # the shortest the block sums
        elif kind == "wave":
            r = rng.integers(0, both, 64)
        else:
            r = rng.integers(0, both, 128)
        rows.append(np.asarray(r, np.int64))
        kinds.append(kind)
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    col = np.concatenate(rows).astype(np.int32)
    coef = (rng.random(col.size) + 0.1).astype(np.float32)
    return ptr, col, coef, kinds


def subset(ptr, col, coef, order):
    """the rows `order` of a batch as a batch of their own (same columns: the tables stay)"""
    parts = [np.arange(ptr[i], ptr[i + 1]) for i in order]
    e = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    p = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int32)
    return p, col[e], coef[e]


def gather64(ptr, col, coef, ta, tb):
    """(sum, sum of |terms|) in float64"""
    t = np.concatenate([ta, tb]).astype(np.float64)
    m = ptr.size - 1
    row_of = np.repeat(np.arange(m), np.diff(ptr))
    c = coef.astype(np.float64)[:, None]
    out, mag = np.zeros((m, t.shape[1])), np.zeros((m, t.shape[1]))
    np.add.at(out, row_of, c * t[col])
    np.add.at(mag, row_of, np.abs(c * t[col]))
    return out, mag


def repeating_rows(ptr, col, at_least=100):
    """irregular_inputs.rows_repeating_one_entry for a CSR that is not square: rows in which one column occurs `at_least` times or
    more — a run of identical terms, whose f32 rounding errors share a sign instead of cancelling (its note)"""
    return [i for i in range(ptr.size - 1) if ptr[i + 1] > ptr[i] and np.unique(col[ptr[i]:ptr[i + 1]], return_counts=True)[1].max() >= at_least]


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def log_softmax(z):
    z = np.asarray(z, np.float64)
    s = z - z.max(axis=1, keepdims=True)
    return s - np.log(np.exp(s).sum(axis=1, keepdims=True))


@pytest.mark.parametrize("m", [1, 5, 65, 257])
@pytest.mark.parametrize("dim", [1, 3, 7, 41, 64, 65, 128, 200, 256])
def test_attach_gather(dev, m, dim):
    ptr, col, coef, kinds = make_rows(m, seed=1000 * m + dim)
    rng = np.random.default_rng(dim)
    ta = (rng.standard_normal((N_A, dim)) * 3).astype(np.float32)
    tb = (rng.standard_normal((m, dim)) * 3).astype(np.float32)
    want, mag = gather64(ptr, col, coef, ta, tb)
    pad = (dim + 3) // 4 * 4 + 4
    odd = (dim | 1) + 2
    # row strides: dim itself (unaligned rows when it is odd), padded to 16 bytes (the 16-byte loads), and one table of each
    strides = [(dim, dim), (pad, pad), (pad, odd)]
    outs = [dev.attach_gather(ptr, col, coef, ta, tb, ld_a=a, ld_b=b, ld_out=pad if a == pad else dim) for a, b in strides]
    base = outs[1]
    heavy = repeating_rows(ptr, col)
    rest = np.setdiff1d(np.arange(m), heavy)
    close_mag(base[rest], want[rest], mag[rest])
    for r in heavy:
        # a run of identical terms: float64 within max(8, the distance of the reference's own sequential f32 sum on this row)
        seq = np.zeros(dim, np.float32)
        for e in range(ptr[r], ptr[r + 1]):
            seq = seq + coef[e] * (ta[col[e]] if col[e] < N_A else tb[col[e] - N_A])
        unit = EPS * mag[r] + 1e-300
        own = float((np.abs(seq.astype(np.float64) - want[r]) / unit).max())
        print(f"m {m} dim {dim} row {r} ({kinds[r]}): sequential f32 {own:.1f}, GPU {float((np.abs(base[r] - want[r]) / unit).max()):.1f} eps.mag from float64")
        close_mag(base[r], want[r], mag[r], k=max(8.0, own))
    for i, k in enumerate(kinds):
        if k == "empty":
            assert np.all(bits(base[i]) == 0), i                # a row without edges: +0 everywhere
    # both load paths add the same terms in the same order: the same bits
    for o in outs:
        assert np.array_equal(bits(o), bits(base))
    # two launches
    assert np.array_equal(bits(dev.attach_gather(ptr, col, coef, ta, tb, ld_a=pad, ld_b=pad)), bits(base))
    # ReLU is exact on the stored sums
    for a, b in strides[:2]:
        relu = dev.attach_gather(ptr, col, coef, ta, tb, epilogue="relu", ld_a=a, ld_b=b)
        assert np.array_equal(bits(relu), bits(np.where(base > 0, base, np.float32(0))))
    # the batch in permuted row order, and rows on their own (every kind of row, first and last of the batch)
    perm = np.random.default_rng(7).permutation(m)
    p2, c2, f2 = subset(ptr, col, coef, perm)
    assert np.array_equal(bits(dev.attach_gather(p2, c2, f2, ta, tb, ld_a=pad, ld_b=pad)), bits(base[perm]))
    alone = sorted(set(list(range(min(m, len(KINDS)))) + [m - 1, m // 2]))
    for i in alone:
        p1, c1, f1 = subset(ptr, col, coef, [i])
        for a, b in strides[:2]:
            assert np.array_equal(bits(dev.attach_gather(p1, c1, f1, ta, tb, ld_a=a, ld_b=b)), bits(base[i:i + 1])), (i, kinds[i])
    # the predict epilogue against numpy on the returned logits
    if dim > 64:
        if m == 1:
            with pytest.raises(Exception, match="at most 64 columns"):
                dev.attach_gather(ptr, col, coef, ta, tb, epilogue="predict")
        return
    for a, b in strides:
        for beta in (1.0, 0.5):
            got = dev.attach_gather(ptr, col, coef, ta, tb, epilogue="predict", beta=beta, ld_a=a, ld_b=b, logp=True)
            z = got["z"]
            assert np.array_equal(bits(z), bits(base))
            assert np.array_equal(got["pred"], np.argmax(z, axis=1))                  # the lowest class on a tie
            lz = log_softmax(beta * z.astype(np.float64))
            assert np.allclose(got["prob"], np.exp(lz.max(axis=1)), rtol=2e-6, atol=0)
            assert np.allclose(got["logp"], lz, rtol=0, atol=2e-5 * max(1.0, float(np.abs(z).max())))
            lean = dev.attach_gather(ptr, col, coef, ta, tb, epilogue="predict", beta=beta, ld_a=a, ld_b=b, store=False)
            assert "z" not in lean and np.array_equal(lean["pred"], got["pred"]) and np.array_equal(bits(lean["prob"]), bits(got["prob"]))
            for i, k in enumerate(kinds):
                if k == "empty":                                # zeros: class 0, probability 1 / dim
                    assert got["pred"][i] == 0 and abs(float(got["prob"][i]) - 1.0 / dim) <= 2e-6 / dim


def test_refusals(dev):
    ptr, col, coef, _ = make_rows(5, seed=3)
    t = lambda n, d: np.ones((n, d), np.float32)
    with pytest.raises(Exception, match="at most 64 columns"):
        dev.attach_gather(ptr, col, coef, t(N_A, 65), t(5, 65), epilogue="predict")
    with pytest.raises(Exception, match="1 <= dim <= 256"):
        dev.attach_gather(ptr, col, coef, t(N_A, 257), t(5, 257))
    with pytest.raises(Exception, match="beta must be finite and > 0"):
        dev.attach_gather(ptr, col, coef, t(N_A, 7), t(5, 7), epilogue="predict", beta=0.0)
    assert dev.attach_gather(np.zeros(1, np.int32), [], [], t(N_A, 7), np.zeros((0, 7), np.float32)).shape == (0, 7)      # m = 0: no launch
