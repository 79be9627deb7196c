"""The three launches of csrc/ranking.hip through cuda_gcn_amd.ops against numpy: the segmented sort bit for bit with np.sort at
the sizes where it changes path (one tile, the tile's edges, several merge passes, a short last run), the key tables and their
counts against tests/ranking_ref.py, u2 exactly and ap_sum within P . 2^-52 relative (the bound of a float64 sum of P correctly
rounded positive terms in any order), and the three chained on integer-valued scores."""
import numpy as np
import pytest

from tests import ranking_ref as R

pytestmark = pytest.mark.gpu
CANARY, SCRATCH = 0xDEADBEEF, 0xC3C3C3C3


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def dev():
    from cuda_gcn_amd.ops import Device
    d = Device(0)
    yield d
    d.close()


def tile():
    from cuda_gcn_amd import ops
    return ops.SORT_TILE


def sort_data(rng, s, n):
    """the data kinds of the sort test, each uint32 [s, n]"""
    head = rng.integers(0, 2 ** 32, (s, n), dtype=np.uint64).astype(np.uint32)
    head[:, n - n // 3:] = R.SENTINEL
    edges = rng.integers(0, 2 ** 32, (s, n), dtype=np.uint64).astype(np.uint32)
    edges[rng.random((s, n)) < 0.3] = 0
    edges[rng.random((s, n)) < 0.3] = 0xFFFFFFFF
    return dict(random=rng.integers(0, 2 ** 32, (s, n), dtype=np.uint64).astype(np.uint32),
                equal=np.full((s, n), 0x12345678, np.uint32),
                ascending=np.broadcast_to(np.arange(n, dtype=np.uint32) * 3, (s, n)).copy(),
                descending=np.broadcast_to(np.arange(n, dtype=np.uint32)[::-1] * 5 + 1, (s, n)).copy(),
                three=rng.choice(np.array([7, 0x80000000, 0xFFFFFF00], np.uint32), (s, n)),
                edges=edges, sentinel_tail=head)


SORT_SIZES = ["0", "1", "2", "63", "64", "65", "T-1", "T", "T+1", "2*T+3", "5*T+17", "16*T"]


@pytest.mark.parametrize("size", SORT_SIZES)
def test_sort_segments_equal_numpy_sort(dev, size):
    """n keys per segment, S segments (3 and 130 only at the small n), stride n and n + 5 with a canary in the gap that must
    survive in the keys and in the scratch; random, all equal, ascending, descending, three values, 0 and 0xFFFFFFFF, a random
    head with a sentinel tail"""
    T = tile()
    n = eval(size, {"T": T})
    rng = np.random.default_rng(1000 + n)
    for s in ((1, 3, 130) if n <= 65 else (1, 3) if n <= T + 1 else (1,)):
        for name, data in sort_data(rng, s, n).items():
            for gap in (0, 5):
                keys = np.full((s, n + gap), CANARY, np.uint32)
                keys[:, :n] = data
                if n + gap == 0:
                    keys = np.zeros((s, 1), np.uint32)         # a table needs a byte; n stays 0
                got, scratch = dev.sort_segments(keys, n=n, scratch_fill=SCRATCH, return_scratch=True)
                assert same_bits(got[:, :n], np.sort(data, axis=1)), (size, s, name, gap)
                assert np.all(got[:, n:] == keys[:, n:]) and np.all(scratch[:, n:] == SCRATCH), (size, s, name, gap)


def test_sort_twice_and_refusals(dev):
    from cuda_gcn_amd.ops import GcnHipError
    T = tile()
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 2 ** 32, (2, 3 * T + 11), dtype=np.uint64).astype(np.uint32)
    a, b = dev.sort_segments(keys), dev.sort_segments(keys)
    assert same_bits(a, b) and same_bits(a, np.sort(keys, axis=1))
    # one tile needs no scratch; more than one does
    assert same_bits(dev.sort_segments(keys[:, :T], scratch=False), np.sort(keys[:, :T], axis=1))
    small = np.zeros((1, 8), np.uint32)
    for kw, msg in ((dict(n=2 ** 24 + 1), r"0 <= n <= 2\^24"), (dict(n=-1), r"0 <= n <= 2\^24"), (dict(segments=0), "at least one segment"),
                    (dict(segments=-3), "at least one segment"), (dict(n=9), "the segment stride is below n")):
        with pytest.raises(GcnHipError, match=f"gcnhip_sort_segments_u32: {msg}"):
            dev.sort_segments(small, **kw)
    with pytest.raises(GcnHipError, match="needs a scratch table"):
        dev.sort_segments(keys, scratch=False)


def score_table(rng, n, c):
    """f32 scores with ties, -0.0 and +0.0, +-inf and NaN"""
    s = rng.integers(-4, 5, (n, c)).astype(np.float32) / 4
    s[rng.random((n, c)) < 0.05] = -0.0
    s[rng.random((n, c)) < 0.02] = np.inf
    s[rng.random((n, c)) < 0.02] = -np.inf
    s[rng.random((n, c)) < 0.03] = np.nan
    return s


@pytest.mark.parametrize("c,c0,c1", [(7, 0, 7), (70, 0, 70), (70, 3, 69), (130, 64, 130)])
def test_rank_keys_against_the_reference(dev, c, c0, c1):
    """a table with ld > C, a row list with repeats (150 of 90 rows: three row tiles, the last one short) and every row; int32
    truth with -1 and C among the labels, and bit rows; scores with -0.0, +-inf and NaN.  Both tables equal the reference entry
    by entry and, sorted by the device, segment by segment; the counts are exact; the gap behind n is not written"""
    rng = np.random.default_rng(c * 1000 + c0)
    n_table = 90
    s = score_table(rng, n_table, c)
    label = rng.integers(-1, c + 1, n_table).astype(np.int32)
    bits = rng.random((n_table, c)) < 0.3
    for rows in (rng.integers(0, n_table, 150).astype(np.int32), None):
        idx = np.arange(n_table) if rows is None else rows
        n = idx.size
        for truth, kw in ((label, dict(truth=label)), (bits, dict(truth_bits=bits))):
            pk, nk, pos, neg, inv, unl = dev.rank_keys(s, c0, c1, rows=rows, ld=c + 3, stride=n + 5, fill=0x5A5A5A5A, **kw)
            sub = truth[idx] if truth.ndim == 1 else truth[idx][:, c0:c1]
            wp, wn = R.key_tables(s[idx][:, c0:c1], sub, classes=np.arange(c0, c1), num_classes=c)
            st = R.table_stats(s[idx][:, c0:c1], sub, classes=np.arange(c0, c1), num_classes=c)
            assert same_bits(pk[:, :n], wp) and same_bits(nk[:, :n], wn)
            assert np.all(pk[:, n:] == 0x5A5A5A5A) and np.all(nk[:, n:] == 0x5A5A5A5A)
            assert np.array_equal(pos, st["pos"]) and np.array_equal(neg, st["neg"]) and np.array_equal(inv, st["invalid"]) and unl == st["unlabelled"]
            assert np.array_equal((pk[:, :n] != R.SENTINEL).sum(axis=1), pos) and inv.sum() > 0 and (truth.ndim == 2 or unl > 0)
            sp, sn = dev.sort_segments(pk, n=n), dev.sort_segments(nk, n=n)
            for j in range(c1 - c0):
                assert same_bits(sp[j, :pos[j]], st["pos_keys"][j]) and np.all(sp[j, pos[j]:n] == R.SENTINEL)
                assert same_bits(sn[j, :neg[j]], st["neg_keys"][j]) and np.all(sn[j, neg[j]:n] == R.SENTINEL)
            again = dev.rank_keys(s, c0, c1, rows=rows, ld=c + 3, stride=n + 5, fill=0x5A5A5A5A, **kw)
            assert all(same_bits(x, y) for x, y in zip((pk, nk, pos, neg, inv), again[:5])) and again[5] == unl


def test_rank_keys_refusals(dev):
    from cuda_gcn_amd.ops import GcnHipError
    s = np.zeros((4, 3), np.float32)
    t = np.zeros(4, np.int32)
    for kw, msg in ((dict(c0=2, c1=2, truth=t), "the class range"), (dict(c1=4, truth=t), "the class range"), (dict(), "give either int32 truth or truth bit rows"),
                    (dict(truth=t, truth_bits=np.zeros((4, 3), bool)), "give either int32 truth or truth bit rows"),
                    (dict(truth=t, stride=3), "the column stride"), (dict(truth=t, n=5, stride=8), "without a row list n is at most n_table"),
                    (dict(truth=t, n=2 ** 24 + 1), r"0 <= n <= 2\^24")):
        with pytest.raises(GcnHipError, match=f"gcnhip_rank_keys: {msg}"):
            dev.rank_keys(s, **kw)


def test_rank_stats_on_hand_built_tables(dev):
    """sorted tables with heavy ties (keys from 9 values), a class without positives, one without negatives, one with neither,
    and one whose positives outnumber a launch's threads (the grid-stride path): u2 exact, ap_sum within P . 2^-52 relative,
    zeros where there is no positive; the padding behind the counts is never compared with; two launches give the same bits"""
    rng = np.random.default_rng(11)
    n = 9000
    counts = [(700, 1300), (0, 500), (400, 0), (0, 0), (8700, 300), (1, 1), (n, n)]
    pk, nk = np.full((len(counts), n), R.SENTINEL, np.uint32), np.full((len(counts), n), R.SENTINEL, np.uint32)
    want_u2, want_ap = [], []
    for j, (p, q) in enumerate(counts):
        vals = R.key(np.arange(-1.0, 1.01, 0.25).astype(np.float32)) if j != 6 else rng.integers(0, 2 ** 32, 4 * n, dtype=np.uint64).astype(np.uint32)
        pk[j, :p], nk[j, :q] = np.sort(rng.choice(vals, p)), np.sort(rng.choice(vals, q))
        u, a = R.sorted_stats(pk[j, :p], nk[j, :q])
        want_u2.append(u)
        want_ap.append(a)
    pk[1, :] = 5                                               # behind a count of 0: must not be read as keys
    nk[2, :] = 5
    pos, neg = np.array([c[0] for c in counts], np.int32), np.array([c[1] for c in counts], np.int32)
    u2, ap = dev.rank_stats(pk, nk, pos, neg)
    assert u2.dtype == np.int64 and u2.tolist() == want_u2
    for j, (p, q) in enumerate(counts):
        assert abs(ap[j] - want_ap[j]) <= p * 2.0 ** -52 * want_ap[j], (j, ap[j], want_ap[j])
    assert u2[1] == u2[2] == u2[3] == 0 and ap[1] == ap[3] == 0.0 and ap[2] == 400.0
    again = dev.rank_stats(pk, nk, pos, neg)
    assert same_bits(u2, again[0]) and same_bits(ap, again[1])


@pytest.mark.parametrize("c", [3, 33, 65])
def test_keys_sort_stats_end_to_end(dev, c):
    """2 T + 3 rows of integer-valued scores (every tie is real), C bit-row classes: u2 equals the reference exactly"""
    n = 2 * tile() + 3
    rng = np.random.default_rng(c)
    s = rng.integers(-20, 21, (n, c)).astype(np.float32)
    y = rng.random((n, c)) < rng.random(c)[None, :] * 0.5
    y[:, 0] = False                                            # a class without positives
    pk, nk, pos, neg, inv, unl = dev.rank_keys(s, truth_bits=y, ld=c + 1)
    st = R.table_stats(s, y)
    assert np.array_equal(pos, st["pos"]) and np.array_equal(neg, st["neg"]) and not inv.any() and unl == 0
    both = dev.sort_segments(np.concatenate([pk, nk]))         # 2 C segments in one call, as the model does it
    u2, ap = dev.rank_stats(both[:c], both[c:], pos, neg)
    assert np.array_equal(u2, st["u2"]) and u2[0] == 0 and ap[0] == 0.0
    assert np.all(np.abs(ap - st["ap_sum"]) <= st["pos"] * 2.0 ** -52 * st["ap_sum"])
