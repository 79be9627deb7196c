"""The three launches of csrc/thresholds.hip through cuda_gcn_amd.ops against tests/thresholds_ref.py.  The scan is compared
exactly on every output — the threshold's bits, the integer counts and the bits of the float64 F: the counts are integers and
F is one expression of correctly rounded float64 operations on both sides, so there is nothing to tolerate.  The two _thr
kernels are compared with the rule in numpy, and at thr = the smallest positive float with the existing z > 0 kernels."""
import numpy as np
import pytest

from tests import ranking_ref as R
from tests import thresholds_ref as TR

pytestmark = pytest.mark.gpu
CANARY = 0xDEADBEEF
BETAS = (0.5, 1.0, 2.0)


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


def assert_scan_equals(got, want, what):
    thr, cnt, f, defined = got
    assert thr.dtype == np.float32 and f.dtype == np.float64 and cnt.dtype == np.int32 and defined.dtype == np.int32
    assert same_bits(thr, want["threshold"]), (what, thr, want["threshold"])
    assert np.array_equal(cnt[0], want["tp"]) and np.array_equal(cnt[1], want["fp"]) and np.array_equal(cnt[2], want["fn"]), what
    assert same_bits(f, want["f"]), (what, f, want["f"])
    assert np.array_equal(defined, want["defined"]), what
    assert not np.isnan(thr).any() and not np.isnan(f).any()


@pytest.fixture(scope="module")
def hand_tables():
    """Sorted tables with heavy ties (keys of 9 values), classes without positives, without negatives, with neither, with one
    of each, with every score equal, and one with more positives (9000) than the 32 x 256 threads of its blocks, so that the
    strided walk, every block and the fold take part.  What lies behind a count is not a key: the sentinel, or a 5 that
    would win if it were read.  (counts, pos_keys, neg_keys) with n = 9500 keys per class."""
    rng = np.random.default_rng(11)
    n = 9500
    counts = [(700, 1300), (0, 500), (400, 0), (0, 0), (9000, 500), (1, 1), (n, n), (300, 200), (9300, 9500)]
    pk, nk = np.full((len(counts), n), R.SENTINEL, np.uint32), np.full((len(counts), n), R.SENTINEL, np.uint32)
    nine = R.key(np.arange(-1.0, 1.01, 0.25).astype(np.float32))
    for j, (p, q) in enumerate(counts):
        vals = rng.integers(0x007FFFFF, 0xFF800001, 4 * n, dtype=np.uint64).astype(np.uint32) if j in (6, 8) else nine
        if j == 7:
            vals = nine[3:4]                                   # every score equal
        pk[j, :p], nk[j, :q] = np.sort(rng.choice(vals, p)), np.sort(rng.choice(vals, q))
    pk[1, :] = 5
    nk[2, :] = 5
    return counts, pk, nk


@pytest.mark.parametrize("beta", BETAS)
def test_scan_on_hand_built_tables(dev, hand_tables, beta):
    """exact on every output; stride n and n + 5 with a canary in the gap; the same bits on a second launch"""
    counts, pk, nk = hand_tables
    n = pk.shape[1]
    pos, neg = np.array([c[0] for c in counts], np.int32), np.array([c[1] for c in counts], np.int32)
    want = TR.fit_columns([pk[j, :p] for j, (p, q) in enumerate(counts)], [nk[j, :q] for j, (p, q) in enumerate(counts)], beta)
    got = dev.threshold_scan(pk, nk, pos, neg, beta=beta)
    assert_scan_equals(got, want, "stride n")
    assert want["defined"].tolist() == [1, 0, 1, 0, 1, 1, 1, 1, 1] and got[2][1] == got[2][3] == 0.0 and got[0][1] == 0.0
    assert got[1][1][1] == int((nk[1, :500] >= TR.KEY_ZERO).sum())                              # P = 0: FP of the cut 0.0
    assert got[2][2] == 1.0 and got[1][:, 2].tolist() == [400, 0, 0]                            # N = 0: everything, F = 1
    gap = lambda t: np.concatenate([t, np.full((t.shape[0], 5), CANARY, np.uint32)], axis=1)
    assert_scan_equals(dev.threshold_scan(gap(pk), gap(nk), pos, neg, beta=beta, n=n), want, "stride n + 5")
    again = dev.threshold_scan(pk, nk, pos, neg, beta=beta)
    assert all(same_bits(a, b) for a, b in zip(got, again))


def score_table(rng, n, c):
    """f32 scores with ties, -0.0 and +0.0, +-inf, NaN and denormals"""
    s = rng.integers(-4, 5, (n, c)).astype(np.float32) / 4
    s[rng.random((n, c)) < 0.05] = -0.0
    s[rng.random((n, c)) < 0.03] = np.float32(1e-45)
    s[rng.random((n, c)) < 0.03] = np.float32(-3e-42)
    s[rng.random((n, c)) < 0.02] = np.inf
    s[rng.random((n, c)) < 0.02] = -np.inf
    s[rng.random((n, c)) < 0.03] = np.nan
    return s


@pytest.mark.parametrize("size", ["0", "1", "65", "T+1", "2*T+3"])
@pytest.mark.parametrize("c,c0,c1", [(3, 0, 3), (70, 3, 69), (130, 64, 130)])
def test_keys_sort_scan_end_to_end(dev, c, c0, c1, size):
    """n listed rows (a list with repeats; every row when C = 70) of a table with ld > C, the classes [c0, c1): keys,
    one sort of both tables, the scan — against the reference on the same rows.  The first class of the range has no
    positive, the second no negative, the third only NaN scores."""
    n = eval(size, {"T": tile()})
    rng = np.random.default_rng(c * 100000 + n)
    use_list = n == 0 or c != 70
    n_table = n // 2 + 1 if use_list else n
    s = score_table(rng, n_table, c)
    y = rng.random((n_table, c)) < rng.random(c)[None, :] * 0.6
    y[:, c0] = False
    if c1 - c0 > 1:
        y[:, c0 + 1] = True
    if c1 - c0 > 2:
        s[:, c0 + 2] = np.nan
    rows = rng.integers(0, n_table, n).astype(np.int32) if use_list else None
    idx = np.arange(n_table) if rows is None else rows
    pk, nk, pos, neg, inv, unl = dev.rank_keys(s, c0, c1, truth_bits=y, rows=rows, ld=c + 3)
    S = c1 - c0
    both = dev.sort_segments(np.concatenate([pk, nk]), n=n)
    beta = BETAS[(c + n) % 3]
    want = TR.table_fit(s[idx][:, c0:c1], y[idx][:, c0:c1], beta)
    assert np.array_equal(pos, want["pos"]) and np.array_equal(neg, want["neg"]) and np.array_equal(inv, want["invalid"])
    got = dev.threshold_scan(both[:S], both[S:], pos, neg, beta=beta, n=n)
    assert_scan_equals(got, want, (c, c0, c1, n))
    assert got[3][0] == 0 and (S < 3 or (got[3][2] == 0 and pos[2] == neg[2] == 0))
    # the cuts, applied to the rows they were fitted on, count what the scan counted; a positive with a NaN score is in no P,
    # and is a miss of every cut
    if n > 0:
        cnt = dev.bce_class_counts_rows_thr(s[:, c0:c1], y[:, c0:c1], got[0], rows=rows)
        nan_pos = (np.isnan(s[idx][:, c0:c1]) & y[idx][:, c0:c1]).sum(0)
        assert np.array_equal(cnt[:2], got[1][:2]) and np.array_equal(cnt[2], got[1][2] + nan_pos)


def test_scan_refusals(dev):
    from cuda_gcn_amd.ops import GcnHipError
    k = np.zeros((2, 8), np.uint32)
    one = np.ones(2, np.int32)
    for kw, msg in ((dict(beta=0.0), "beta must be finite and > 0"), (dict(beta=-1.0), "beta must be finite and > 0"),
                    (dict(beta=float("nan")), "beta must be finite and > 0"), (dict(beta=float("inf")), "beta must be finite and > 0"),
                    (dict(n=2 ** 24 + 1), r"0 <= n <= 2\^24"), (dict(n=-1), r"0 <= n <= 2\^24"), (dict(n=9), "the column stride")):
        with pytest.raises(GcnHipError, match=f"gcnhip_threshold_scan: {msg}"):
            dev.threshold_scan(k, k, one, one, **kw)
    # a work block that is not 8-byte aligned, and a missing output
    lib, b = dev.lib, [dev.buf(np.zeros(64, np.float64)) for _ in range(8)]
    ptr = [x.ptr for x in b]
    assert lib.gcnhip_threshold_scan(dev.ctx, ptr[0], ptr[1], 8, 8, 1, ptr[2], ptr[3], 1.0, ptr[4] + 4, ptr[5], ptr[6], ptr[7], ptr[7] + 64) == -1
    assert b"gcnhip_threshold_scan: the work block must be 8-byte aligned" in lib.gcnhip_last_error()
    assert lib.gcnhip_threshold_scan(dev.ctx, ptr[0], ptr[1], 8, 8, 1, ptr[2], ptr[3], 1.0, ptr[4], None, ptr[6], ptr[7], ptr[7] + 64) == -1
    assert b"gcnhip_threshold_scan: invalid argument" in lib.gcnhip_last_error()
    assert lib.gcnhip_threshold_scan(dev.ctx, ptr[0], ptr[1], 8, 8, 0, ptr[2], ptr[3], 1.0, ptr[4], ptr[5], ptr[6], ptr[7], ptr[7] + 64) == -1
    assert b"1 <= classes <= 65535" in lib.gcnhip_last_error()


def logit_table(rng, n, c):
    """logits with +-0, +-inf, NaN, denormals of both signs and the smallest normal"""
    z = (rng.standard_normal((n, c)) * 2).astype(np.float32)
    for v in (0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 3e-42, -3e-42, 1.17549435e-38):
        z[rng.random((n, c)) < 0.04] = np.float32(v)
    return z


@pytest.fixture(scope="module", params=[1, 33, 256])
def thr_case(request):
    """a logit table, its truth, a row list with repeats, and per-class cuts among which are +-0, a denormal, +-inf and values
    the table holds (so that z == t happens)"""
    c = request.param
    rng = np.random.default_rng(c)
    n = 150
    z = logit_table(rng, n, c)
    y = rng.random((n, c)) < 0.3
    rows = rng.integers(0, n, 333).astype(np.int32)
    thr = (rng.standard_normal(c) * 1.5).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-45, -3e-42, np.inf, -np.inf], np.float32)
    pick = rng.random(c) < 0.4
    thr[pick] = rng.choice(special, int(pick.sum()))
    take = rng.random(c) < 0.3
    held = z[rng.integers(0, n, c), np.arange(c)]
    thr[take] = np.where(np.isnan(held), np.float32(0.25), held)[take]
    return c, z, y, rows, thr


def test_thr_kernels_equal_the_rule(dev, thr_case):
    """bits, sigmoid rows and counts, with a row list with repeats and with every row, ld > C with NaN padding"""
    c, z, y, rows, thr = thr_case
    for rr in (rows, None):
        idx = np.arange(z.shape[0]) if rr is None else rr
        bits, prob = dev.bce_predict_rows_thr(z, thr, rows=rr, ld=c + 5)
        assert np.array_equal(bits, TR.predict(z[idx], thr))
        old_bits, old_prob = dev.bce_predict_rows(z, rows=rr, ld=c + 5)
        assert same_bits(prob, old_prob)                       # prob stays sigmoid(z)
        bits_only, none = dev.bce_predict_rows_thr(z, thr, rows=rr, prob=False)
        assert none is None and np.array_equal(bits_only, bits)
        cnt = dev.bce_class_counts_rows_thr(z, y, thr, rows=rr, ld=c + 5)
        assert cnt.dtype == np.int32 and np.array_equal(cnt, TR.counts(z[idx], y[idx], thr))
        assert same_bits(cnt, dev.bce_class_counts_rows_thr(z, y, thr, rows=rr, ld=c + 5))
    assert np.array_equal(dev.bce_class_counts_rows_thr(z, y, thr, rows=np.zeros(0, np.int32)), np.zeros((3, c), np.int32))


def test_smallest_positive_cut_is_the_training_rule(dev, thr_case):
    """z >= the smallest positive float is z > 0: bits, probabilities and counts equal those of the existing kernels on a table
    that holds denormals of both signs — the comparison is one of integers, whatever the float denormal mode"""
    c, z, y, rows, _ = thr_case
    thr = np.full(c, np.nextafter(np.float32(0), np.float32(1)), np.float32)
    assert thr[0] > 0 and thr.view(np.uint32)[0] == 1
    bits, prob = dev.bce_predict_rows_thr(z, thr, rows=rows, ld=c + 2)
    old_bits, old_prob = dev.bce_predict_rows(z, rows=rows, ld=c + 2)
    assert np.array_equal(bits, old_bits) and same_bits(prob, old_prob)
    assert np.array_equal(bits, z[rows] > 0) and bits[z[rows] == np.float32(1e-45)].all()
    assert same_bits(dev.bce_class_counts_rows_thr(z, y, thr, rows=rows, ld=c + 2), dev.bce_class_counts_rows(z, y, rows=rows, ld=c + 2))
    # a NaN cut predicts its class for no row
    thr[0] = np.nan
    assert not dev.bce_predict_rows_thr(z, thr, prob=False)[0][:, 0].any()
    assert dev.bce_class_counts_rows_thr(z, y, thr)[:2, 0].tolist() == [0, 0]


def test_thr_refusals(dev):
    from cuda_gcn_amd.ops import GcnHipError
    z, y = np.zeros((4, 257), np.float32), np.zeros((4, 257), bool)
    with pytest.raises(GcnHipError, match="gcnhip_bce_predict_rows_thr: at most 256 classes"):
        dev.bce_predict_rows_thr(z, np.zeros(257, np.float32))
    with pytest.raises(GcnHipError, match="gcnhip_bce_class_counts_rows_thr: at most 256 classes"):
        dev.bce_class_counts_rows_thr(z, y, np.zeros(257, np.float32))
    lib, b = dev.lib, [dev.buf(np.zeros(64, np.float32)) for _ in range(4)]
    ptr = [x.ptr for x in b]
    for args, msg in (((ptr[0], 4, None, 2, 4, None, ptr[2], 1, None, 0), b"invalid argument"),
                      ((ptr[0], 3, None, 2, 4, ptr[1], ptr[2], 1, None, 0), b"invalid argument"),
                      ((ptr[0], 40, None, 1, 40, ptr[1], ptr[2], 1, None, 0), b"words_per_row"),
                      ((ptr[0], 4, None, 2, 4, ptr[1], ptr[2], 1, ptr[3], 3), b"the row stride of prob")):
        assert lib.gcnhip_bce_predict_rows_thr(dev.ctx, *args) == -1 and msg in lib.gcnhip_last_error()
    for args, msg in (((ptr[0], 4, ptr[1], 1, None, 2, 4, None, ptr[2]), b"invalid argument"),
                      ((ptr[0], 4, ptr[1], 1, None, -1, 4, ptr[3], ptr[2]), b"invalid argument"),
                      ((ptr[0], 40, ptr[1], 1, None, 1, 40, ptr[3], ptr[2]), b"words_per_row")):
        assert lib.gcnhip_bce_class_counts_rows_thr(dev.ctx, *args) == -1 and msg in lib.gcnhip_last_error()
