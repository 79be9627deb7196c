"""The dropout stream on the CPU: Philox against published vectors, the kernels' recurrence against the definition.

Every GPU test of a dropout decision compares with test_ops_gpu.philox_keep, which restates the kernels' own walk over the
bit planes.  Here that restatement is tied to two things outside it: philox4x32 (its and dropout_ref's) to the Random123
known answers, and philox_keep to dropout_ref.keep, the materialised U16(j) >= thr16, on every (threshold, offset, seed) of
the shared table.  The keep rate of the first 2^20 decisions is held to 5 binomial sigma of 1 - thr16 / 65536, the
threshold to its rounding edges, and three mutants of the recurrence show which table cases notice them.

Found here: the float below p = 2^-17 does not give thr16 = 0.  p * 65536 + 0.5 = 1 - 2^-25 is a tie and rounds to 1.0, so
the threshold turns from 0 to 1 one float further down (dropout_ref.P_ZERO | P_BELOW).  Both pairs are checked as they are.

Keep rate, worst case of the table: 2.04 sigma (thr16(0.3), seed 42, epoch 5: 0.70091 kept against 0.69999); the worst of
the other two seeds are 0.96 and 1.26 sigma.

A missing lowest bit plane changes one decision in 2^n_planes, so on short runs only the thresholds of one or two planes
are sure to notice it; the mutant test says so and the GPU tests carry such thresholds to every producer.
"""
import numpy as np
import pytest

from tests import dropout_ref as D
from tests.test_ops_gpu import philox4x32, philox_keep, thr_of

N_RUN = 4096
N_RATE = 1 << 20


# ----------------------------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("ctr,key,want", D.KNOWN_ANSWERS)
def test_philox_known_answers(ctr, key, want):
    assert [int(x) for x in D.philox4x32_10(ctr, key)] == list(want)
    assert [int(x) for x in philox4x32(*ctr, *key)] == list(want)            # the one under every existing GPU test


def test_philox_on_arrays_is_philox_on_each_element():
    rng = np.random.default_rng(1)
    c = rng.integers(0, 1 << 32, (4, 50), dtype=np.uint64)
    key = (0x9abcdef0, 0x12345678)
    got = D.philox4x32_10(tuple(c), key)
    for e in (0, 17, 49):
        assert np.array_equal(got[e], D.philox4x32_10(tuple(int(x) for x in c[:, e]), key))
    assert np.array_equal(got, np.stack(philox4x32(*c, *key), axis=-1))


# ------------------------------------------------------------------------------------------- definition and recurrence
def test_u16_takes_each_bit_from_its_own_philox_call():
    """u16 of single indices, spelled out with Python integers: plane i gives bit 16 - i, word (j >> 5) & 3, bit j & 31,
    counter {lo32(j >> 7), hi32(j >> 7), epoch, i}, key {lo32 seed, hi32 seed}"""
    for (seed, epoch), j in zip(D.SEEDS, (77, 2 ** 32 + 96, 2 ** 45 + 77)):
        want = 0
        for i in range(1, 17):
            out = D.philox4x32_10(((j >> 7) & D.M32, (j >> 7) >> 32, epoch, i), (seed & D.M32, seed >> 32))
            want |= ((int(out[(j >> 5) & 3]) >> (j & 31)) & 1) << (16 - i)
        assert int(D.u16(seed, epoch, [j])[0]) == want
    assert (2 ** 45 + 77) >> 39 != 0 and D.SEEDS[1][0] >> 32 != 0           # a counter and a key with a high word took part


@pytest.mark.parametrize("seed,epoch", D.SEEDS)
@pytest.mark.parametrize("off", D.OFFSETS)
def test_recurrence_equals_definition(off, seed, epoch):
    j = np.arange(N_RUN, dtype=np.uint64) + np.uint64(off)
    u = D.u16_cached(seed, epoch, off, N_RUN)
    for label, t, _ in D.THR:
        assert np.array_equal(philox_keep(seed, epoch, j, t), u >= t), label


def test_the_table_holds_what_it_is_meant_to():
    ts = [t for _, t, _ in D.THR]
    assert set(D.THR_RAW) <= set(ts) and {D.thr16(p) for p in (0.1, 0.25, 0.3, 0.9)} <= set(ts)
    assert {D.n_planes(t) for t in ts} >= {0, 1, 2, 15, 16}
    assert any(off < 2 ** 32 <= off + N_RUN for off in D.OFFSETS)           # the index crosses 2^32 inside a run
    assert any(off >> 39 == 0 and (off + N_RUN) >> 39 for off in D.OFFSETS)  # the block counter's high word turns non-zero
    assert any(s >> 32 for s, _ in D.SEEDS) and any(e == D.M32 for _, e in D.SEEDS)
    for _, t, p in D.THR:                                                   # a rate for every threshold
        assert D.thr16(p) == t == thr_of(p) and 0 <= p < 1


# ------------------------------------------------------------------------------------------------------------ mutants
def recurrence(seed, epoch, idx, thr16, mutant=None):
    """philox_keep's walk with one slip: 'ctr_hi' drops the counter's high word, 'key_hi' the key's, 'planes' reads one
    plane too few"""
    idx = np.asarray(idx, np.uint64)
    if thr16 == 0:
        return np.ones(idx.shape, bool)
    n_planes = D.n_planes(thr16) - (mutant == "planes")
    blk = idx >> np.uint64(7)
    g = ((idx >> np.uint64(5)) & np.uint64(3)).astype(np.int64)
    ge = np.full(idx.shape + (4,), D.M32, np.uint64)
    for i in range(n_planes, 0, -1):
        P = D.philox4x32_10((blk & np.uint64(D.M32), 0 if mutant == "ctr_hi" else blk >> np.uint64(32), epoch, i),
                            (seed & D.M32, 0 if mutant == "key_hi" else seed >> 32))
        ge = (P & ge) if (thr16 >> (16 - i)) & 1 else (P | ge)
    word = np.take_along_axis(ge, g[..., None], axis=-1)[..., 0]
    return ((word >> (idx & np.uint64(31))) & np.uint64(1)).astype(bool)


def noticed_by(mutant, n=512):
    """the (threshold, offset, seed) cases on which the slip changes a decision among the last n of a run"""
    hit = set()
    for (seed, epoch) in D.SEEDS:
        for off in D.OFFSETS:
            j = np.arange(N_RUN - n, N_RUN, dtype=np.uint64) + np.uint64(off)
            u = D.u16_cached(seed, epoch, off, N_RUN)[N_RUN - n:]
            for label, t, _ in D.THR:
                if not np.array_equal(recurrence(seed, epoch, j, t, mutant), u >= t):
                    hit.add((label, off, seed))
    return hit


def test_the_table_notices_three_slips_of_the_recurrence():
    assert not noticed_by(None)
    live = {label for label, t, _ in D.THR if t != 0}                        # thr16 = 0 keeps everything whatever is drawn
    mid = {label for label, t, _ in D.THR if 0x1000 <= t <= 0xF000}          # (a rate near 0 or 1 can agree by chance on 512 elements)
    everywhere = lambda labels, offs, seeds: {(l, off, s) for l in labels for off in offs for s in seeds}
    all_seeds = [s for s, _ in D.SEEDS]
    high = [off for off in D.OFFSETS if (off + N_RUN) >> 39]
    a = noticed_by("ctr_hi")                                                # only where j >> 7 reaches 2^32
    assert everywhere(mid, high, all_seeds) <= a <= everywhere(live, high, all_seeds)
    assert high == [2 ** 39 - 200, 2 ** 45 + 77]
    wide = [s for s in all_seeds if s >> 32]
    b = noticed_by("key_hi")                                                # only the seeds with a high word
    assert everywhere(mid, D.OFFSETS, wide) <= b <= everywhere(live, D.OFFSETS, wide)
    assert wide == [0xabcdef12345, 2 ** 64 - 1]
    # a missing lowest plane changes one decision in 2^n_planes: sure to show on 512 elements only where few planes are read
    few = {label for label, t, _ in D.THR if 1 <= D.n_planes(t) <= 2}
    c = noticed_by("planes")
    assert everywhere(few, D.OFFSETS, all_seeds) <= c <= everywhere(live, D.OFFSETS, all_seeds)
    assert few == {"thr0x4000", "thr0x8000", "thr0xc000", "p0.25"}


# ---------------------------------------------------------------------------------------------------------- keep rate
@pytest.mark.parametrize("seed,epoch", D.SEEDS)
def test_keep_rate_within_five_sigma(seed, epoch):
    """the streams are fixed, so this is deterministic: kept count of the first 2^20 decisions against the binomial"""
    u = D.u16_cached(seed, epoch, 0, N_RATE)
    worst = 0.0
    for label, t, _ in D.THR:
        q = 1 - t / 65536
        kept = int((u >= t).sum())
        sigma = (N_RATE * q * (1 - q)) ** 0.5
        if sigma == 0:
            assert kept == N_RATE, label
            continue
        z = abs(kept - N_RATE * q) / sigma
        worst = max(worst, z)
        print(f"{label}: kept {kept / N_RATE:.5f} of {q:.5f}, {z:.2f} sigma")
        assert z <= 5, (label, kept, N_RATE * q, sigma)
    print("worst", worst)


# ---------------------------------------------------------------------------------------------------- threshold edges
def test_threshold_edges():
    assert [D.thr16(p) for p in (0.0, 0.5, 0.25, 0.75)] == [0, 0x8000, 0x4000, 0xC000]
    assert [D.thr16(p) for p in (0.1, 0.3, 0.9)] == [6554, 19661, 58982]    # round(p * 65536) of the float32 rate
    # around p = 2^-17, where p * 65536 + 0.5 reaches 1: the tie at one float below rounds up
    f32 = np.float32
    assert f32(D.P_EDGE) == f32(2.0 ** -17) and f32(D.P_BELOW) < f32(D.P_EDGE) < f32(D.P_ABOVE)
    assert np.nextafter(f32(D.P_BELOW), f32(1)) == f32(D.P_EDGE) == np.nextafter(f32(D.P_ABOVE), f32(0))
    assert np.nextafter(f32(D.P_ZERO), f32(1)) == f32(D.P_BELOW)
    assert [D.thr16(p) for p in (D.P_ZERO, D.P_BELOW, D.P_EDGE, D.P_ABOVE)] == [0, 1, 1, 1]
    # the top: 0.999999 * 65536 + 0.5 passes 65536 and is clamped
    assert int(f32(0.999999) * f32(65536.0) + f32(0.5)) == 65536 and D.thr16(0.999999) == 65535
    assert D.thr16(D.p_of(0xFFFF)) == 0xFFFF and D.thr16(float(np.nextafter(f32(1), f32(0)))) == 65535
    for p in (0.0, 0.1, 0.3, 0.5, 0.9, D.P_ZERO, D.P_ABOVE, 0.999999):
        assert D.thr16(p) == thr_of(p)
    assert D.scale(0.5) == 2 and D.scale(0.0) == 1 and D.scale(D.p_of(0xFFFF)) == 65536
    assert D.scale(0.3) == f32(1) / (f32(1) - f32(0.3)) and D.scale(0.3).dtype == np.float32
