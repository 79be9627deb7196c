"""The max-shifted softmax of every loss and prediction kernel against tests/softmax_ref.py (float64 with derived f32 bounds) on
hard logits: xent_kernel and xent_lane_kernel (csrc/xent.hip) through every entry point and both sides of every dispatch test of
xent_launch, the loss and predict epilogues of the logit aggregation (csrc/graphsum.hip, unsplit and split rows), attach_finish
(csrc/attach.hip) and xent_terms_kernel.  The epilogues see logits only as the result of a gather, so the operators here are
built to give the hard rows back exactly (row i gathers table row i and zero rows), and the stored logits are compared bit for bit
with the intended values before anything else is judged.

One deviation from a construction that cannot exist: a 65-edge row has no column degree that makes row length x column degree a
power of four, so on the per-edge and bf16 paths its coefficient is f32(1 / sqrtf(65)) (read back from the object) and the
intended logits are the singly rounded f32 products coefficient x hard row, formed in numpy; the stored logits equal them bit
for bit as well.  Lengths 1, 256 and 4096 give the exact factors 1, 2^-4 and 2^-6.

Padding columns: xent_lane_kernel and the loss epilogue store whole 16-byte quads of a gradient row, so the columns C .. 4 ceil(C / 4) - 1
of a computed row are written as +0 (their comments say so); every column past that, and every column >= C in the wave form,
keeps the fill bits.

Found by these tests:
  * attach_finish at beta != 1 against gcnhip_calib_scale_rows on its beta = 1 log-softmax rows: NOT the same bits, on mild rows
    as on hard ones, from C = 3 on (C = 1 has one term).  attach_finish adds the exponentials left to right, calib_scale_kernel
    in a shuffle tree; the results differ by an ulp or two of the rescaled row.  Nothing depends on the identity, so the kernels
    stay as they are: the comment in csrc/attach.hip now says what differs, and the pair is held to float64 here (both inside
    calib_ref.scale's bounds on the same f32 rows).  Every other identity holds on the hard table.
  * the gradient bound as first stated (error x |factor| (1 + U) for a class weight or a row factor) left out the rounding of
    the product itself; the label's entry of a confidently wrong row exceeded it in the weighted kernels (three roundings
    against 2 U |g|).  softmax_ref's derivation now counts one rounding per product; the kernels are as they were.

Measured on an MI355X (measurements against the reference, not inputs to any bound): 169 cases in 2.7 s of wall time, the slowest
test_block_cap_of_the_loss_kernels[lane-524300-4] at 0.13 s.  Worst |got - want| / bound per family: lane form 0.635, wave form
0.617, loss epilogue unsplit 0.579 and split 0.529, predict epilogue f32 0.493, bf16 0.493 and split 0.426, attach predict 0.448
(gcnhip_calib_scale_rows on the same rows 0.576), terms kernel 0.075, sigmoid loss past its cap 0.091.

Mutants, each built once and run against this file, then discarded: without the shift by the maximum in xent_kernel all 23
wave-form cases of test_loss_kernels_on_hard_rows and test_block_cap_of_the_loss_kernels[wave-16400-3] fail; with `mx >= tv` for
`mx > tv` in xent_lane_kernel its 12 lane-form cases, test_block_cap_of_the_loss_kernels[lane-524300-4] and the cases of
test_loss_epilogue_on_hard_rows (the epilogue no longer has the kernel's counts; seen on the 16 unsplit cases, the split ones
carried the next mutant in that build) fail; with the exponentials added right to left
in xent_row_epilogue1 alone exactly the 16 split-row cases of test_loss_epilogue_on_hard_rows (lengths 256, 1200, 4096) fail —
which also shows that those rows are split and the shorter ones are not.
"""
import time

import numpy as np
import pytest

from tests import calib_ref
from tests import softmax_ref as R
from tests.calib_ref import U, EXP_ATOL

pytestmark = pytest.mark.gpu

FILL = np.uint32(0xFFC5A5A5)                       # a NaN with a payload no kernel produces
WORST = {}
T0 = [None]


@pytest.fixture(scope="module")
def dev():
    from cuda_gcn_amd.ops import Device
    d = Device(0)
    T0[0] = time.time()
    yield d
    print("\nworst |got - want| / bound per family: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    print(f"wall time of this file's cases: {time.time() - T0[0]:.1f} s")
    d.close()


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def filled(shape):
    return np.full(shape, FILL, np.uint32).view(np.float32)


def note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), float(ratio))
    return ratio


def within(family, got, want, bound, what=""):
    r = note(family, R.worst(got, want, bound))
    assert r <= 1.0, f"{family} {what}: |got - want| is {r:.3f} of the bound"


def table_of(z, ld):
    t = filled((z.shape[0], ld))
    t[:, :z.shape[1]] = z
    return t


def is_lane_form(c, ld, ld_grad, offset=0, grad_offset=0, training=True):
    nv4 = (c + 3) // 4
    ok = c <= 64 and ld % 4 == 0 and ld >= 4 * nv4 and offset % 4 == 0
    return ok and (not training or (ld_grad % 4 == 0 and ld_grad >= 4 * nv4 and grad_offset % 4 == 0))


def check_loss_call(family, res, z, ref, c, ld, listed, lane, training, shift, list_form, weighted=False):
    """one loss call against the reference: sums, counts, gradient rows, stray writes, the shifted table"""
    assert res["rc"] == 0
    n = z.shape[0]
    scored = np.zeros(n, bool)
    scored[listed] = True
    scored &= ref["scored"]
    want, bound = R.loss_sum(ref, np.flatnonzero(scored))
    within(family, res["result"][0], want, bound, "loss sum")
    total, correct = int(scored.sum()), int(ref["correct"][scored].sum())
    assert res["result_i"].tolist() == [correct, total], (res["result_i"], correct, total)
    if weighted:
        within(family, res["result"][1], ref["wsum_listed"], 8 * U * ref["wsum_listed"] + 1e-30, "weight sum")
    else:
        assert res["result"][1] == total
    assert res["result"][2] == correct and res["result"][3] == total
    # the logit table: shifted rows are z - max, one f32 subtraction (exact to the bit); everything else keeps its bits
    want_t = table_of(z, ld)
    if shift:
        want_t[scored, :c] = z[scored] - z[scored].max(axis=1, keepdims=True)
    assert np.array_equal(bits(res["table"]), bits(want_t)), "logit table"
    g = res["grad"]
    if not training:
        assert np.all(bits(g) == FILL), "evaluation wrote a gradient"
        return
    w4 = 4 * ((c + 3) // 4) if lane else c
    within(family, g[scored, :c], ref["grad"][scored], ref["E_grad"][scored], "gradient")
    assert np.all(bits(g[scored, c:w4]) == 0) and np.all(bits(g[:, w4:]) == FILL), "padding columns"
    visited = np.ones(n, bool) if not list_form else scored
    if list_form:
        assert np.all(bits(g[~visited]) == FILL), "rows outside the list were written"
    else:
        assert np.all(bits(g[~scored, :w4]) == 0), "an unlabelled row's gradient is not zero"


LANE_C = [1, 2, 3, 4, 5, 8, 9, 41, 60, 61, 64]
SHAPES = [("lane", c, 4 * ((c + 3) // 4), 0, 0) for c in LANE_C] + [("lane", 41, 52, 0, 0)] + \
         [("wave", c, c + 1 + c % 2, 0, 0) for c in LANE_C] + \
         [("wave", 64, 64, o, 0) for o in (1, 2, 3)] + [("wave", 64, 64, 0, o) for o in (1, 2, 3)] + \
         [("wave", c, c, 0, 0) for c in (65, 128, 129, 192, 193, 256)]


@pytest.mark.parametrize("family,c,ld,off,goff", SHAPES)
def test_loss_kernels_on_hard_rows(dev, family, c, ld, off, goff):
    """gcnhip_xent_fwd, _rows, _rows_scaled, gcnhip_wxent_fwd_rows and gcnhip_accuracy on hard_rows(c) at one (C, ld, alignment):
    the loss sum, counts and every gradient entry inside the reference's bounds, the shifted table exact, no stray write, the
    same bits from a second call, from both forms of the final reduction, from the list form and the full pass, and from the
    weighted kernel with every weight 1"""
    z, t = R.hard_rows(c)
    n = z.shape[0]
    lane = is_lane_form(c, ld, ld, off, goff)
    assert lane == (family == "lane")
    fam = family + " form"
    tame = R.tame_rows(z)
    rng = np.random.default_rng(c * 1000 + ld)
    tab, g0 = table_of(z, ld), filled((n, ld))
    kw = dict(offset=off, grad_offset=goff)
    full_grad = {}
    for which in ("all", "tame"):
        tt = t.copy()
        tt[[1, 9, 20]] = -1                                   # a control, a wide and a tie (or underflow) row are not scored
        if which == "tame":
            tt[~tame] = -1
        count = int((tt >= 0).sum())
        ref = R.reference(z, tt, count=count)
        everything = np.arange(n)
        for training in (True, False):
            for cnt in (count, 0):
                for shift in (0, 1):
                    lane_now = is_lane_form(c, ld, ld, off, goff, training)
                    out = []
                    for fin in (0, 1):
                        dev.set_option("xent_finalize", fin)
                        out.append(dev.xent_call("fwd", tab, tt, c, grad=g0, training=training, count=cnt, shift_in_place=shift, **kw))
                    dev.set_option("xent_finalize", 0)
                    a, b = out
                    check_loss_call(fam, a, z, ref, c, ld, everything, lane_now, training, shift, False)
                    for key in ("result", "result_i", "table", "grad"):
                        assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), f"xent_finalize changes {key}"
                    if training and cnt and not shift:
                        full_grad[which] = a["grad"]
        acc = dev.xent_call("accuracy", tab, tt, c, offset=off)
        assert acc["rc"] == 0 and acc["result_i"].tolist() == [int(ref["correct"].sum()), count]
        assert np.array_equal(bits(acc["table"]), bits(tab))
    # the list forms: all rows are labelled here; a sorted subset, a single row, the full list (and the tame rows alone)
    scale = (rng.random(n) + 0.5).astype(np.float32)
    weight = (0.25 + 3.75 * rng.random(c)).astype(np.float32)
    weight[rng.integers(0, c)] = 4.0
    lists = [np.sort(rng.choice(n, n // 2, replace=False)), np.array([n - 3]), np.arange(n), np.flatnonzero(tame)]
    for li, rows in enumerate(lists):
        rows = rows.astype(np.int32)
        for sc in (None, scale):
            ref = R.reference(z, t, count=rows.size, row_scale=sc)
            for training in (True, False):
                lane_now = is_lane_form(c, ld, ld, off, goff, training)
                entry = "scaled" if sc is not None else "rows"
                a = dev.xent_call(entry, tab, t, c, grad=g0, rows=rows, training=training, count=rows.size, grad_row_scale=sc, **kw)
                check_loss_call(fam, a, z, ref, c, ld, rows, lane_now, training, 0, True)
                if sc is None:
                    s0 = dev.xent_call("scaled", tab, t, c, grad=g0, rows=rows, training=training, count=rows.size, **kw)
                    assert all(np.array_equal(a[k].view(np.uint32), s0[k].view(np.uint32)) for k in ("result", "result_i", "grad"))
                # every weight 1.0: the weighted kernels return the unweighted bits
                one = dev.xent_call("weighted", tab, t, c, grad=g0, rows=rows, training=training, count=rows.size, grad_row_scale=sc,
                                    weight=np.ones(c, np.float32), weight_sum=float(rows.size), **kw)
                assert one["rc"] == 0
                assert np.array_equal(one["result"].view(np.uint32), a["result"].view(np.uint32)), (one["result"], a["result"])
                assert np.array_equal(one["result_i"], a["result_i"]) and np.array_equal(bits(one["grad"]), bits(a["grad"]))
                # weights in [0.25, 4]
                wsum = float(weight.astype(np.float64)[t[rows]].sum())
                wref = R.reference(z, t, count=wsum, row_scale=sc, weight=weight)
                wref["wsum_listed"] = wsum
                wres = dev.xent_call("weighted", tab, t, c, grad=g0, rows=rows, training=training, count=rows.size, grad_row_scale=sc,
                                     weight=weight, weight_sum=wsum, **kw)
                check_loss_call(fam, wres, z, wref, c, ld, rows, lane_now, training, 0, True, weighted=True)
        if li >= 2:
            # the list form and the full pass run the same kernel on the same rows: the labelled gradient rows have the same bits
            which = "all" if li == 2 else "tame"
            tt = t.copy()
            tt[[1, 9, 20]] = -1
            if which == "tame":
                tt[~tame] = -1
            keep = np.flatnonzero(tt >= 0).astype(np.int32)
            a = dev.xent_call("rows", tab, t, c, grad=g0, rows=keep, training=True, count=keep.size, **kw)
            assert np.array_equal(bits(a["grad"][keep]), bits(full_grad[which][keep])), "list form and full pass differ"
    # the same call twice
    a = dev.xent_call("fwd", tab, t, c, grad=g0, training=True, count=0, shift_in_place=1, **kw)
    b = dev.xent_call("fwd", tab, t, c, grad=g0, training=True, count=0, shift_in_place=1, **kw)
    assert all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in ("result", "result_i", "table", "grad"))


def test_more_than_256_classes_is_an_error_that_writes_nothing(dev):
    c = 257
    z, t = R.hard_rows(c)
    n = z.shape[0]
    tab, g0 = table_of(z, 260), filled((n, 260))
    rows = np.arange(n, dtype=np.int32)
    for entry in ("fwd", "rows", "scaled", "weighted", "accuracy"):
        a = dev.xent_call(entry, tab, t, c, grad=g0, rows=rows, training=True, count=n, weight=np.ones(c, np.float32), weight_sum=float(n))
        assert a["rc"] != 0, entry
        assert np.all(a["result"].view(np.uint32) == 0x5A5A5A5A) and np.all(a["result_i"].view(np.uint32) == 0x5A5A5A5A), entry
        assert np.array_equal(bits(a["table"]), bits(tab)) and np.all(bits(a["grad"]) == FILL), entry


@pytest.mark.parametrize("family,n,ld", [("wave", 16400, 3), ("lane", 524300, 4)])
def test_block_cap_of_the_loss_kernels(dev, family, n, ld):
    """past the block cap (2048 blocks: 16 384 rows in the wave form, 524 288 in the lane form, whose grid-stride loop then runs
    a second pass): mild logits, C = 3, a third of the rows unlabelled, the count made on the device"""
    c = 3
    rng = np.random.default_rng(n)
    z = (rng.standard_normal((n, c)) * 3).astype(np.float32)
    t = rng.integers(0, c, n).astype(np.int32)
    t[rng.random(n) < 1 / 3] = -1
    t[[0, n - 1]] = 1                                          # the first row and the last row past the cap are scored
    ref = R.reference(z, t)
    a = dev.xent_call("fwd", table_of(z, ld), t, c, grad=filled((n, ld)), training=True, count=0)
    assert a["rc"] == 0
    fam = family + " form"
    want, bound = R.loss_sum(ref)
    within(fam, a["result"][0], want, bound, "loss sum past the cap")
    assert a["result_i"].tolist() == [int(ref["correct"].sum()), int(ref["scored"].sum())]
    pick = np.unique(np.concatenate([rng.choice(n, 996, replace=False), [0, 1, n - 2, n - 1]]))
    within(fam, a["grad"][pick, :c], ref["grad"][pick], ref["E_grad"][pick] + 0.0, "sampled gradient rows past the cap")
    scored = ref["scored"]
    assert np.all(np.isfinite(a["grad"][scored, :c])) and np.all(bits(a["grad"][~scored, :c]) == 0)
    assert np.all(bits(a["grad"][:, c:]) == (0 if family == "lane" else FILL))


@pytest.mark.parametrize("c", [1, 33])
def test_block_cap_of_the_sigmoid_loss(dev, c):
    """gcnhip_bce_fwd_rows past its block cap (1024 blocks of 16 rows: 16 384 listed rows), with one multi-hot word per row more
    than C needs and every bit at or past C set to noise.  Bounds, in the style of softmax_ref: an element is
    a + l with a = max(z, 0) - y z (one rounding) and l = log1pf(expf(-|z|)); expf is EXP_ATOL off, which moves log1p by at most
    1.5 EXP_ATOL l (x <= 1.45 log1p(x) on [0, 1]), log1pf adds EXP_ATOL l:  E = 2.5 EXP_ATOL l + U (|a| + |a + l|); the sum is
    sum E + 8 U sum |element|.  A gradient entry is a sigmoid (expf, one addition, one division) over the divisor:
    |g| (EXP_ATOL + 4 U) plus one f32 denormal step."""
    n = 16400
    rng = np.random.default_rng(c)
    z = (rng.standard_normal((n, c)) * 4).astype(np.float32)
    y = rng.random((n, c)) < 0.3
    wpr = (c + 31) // 32 + 1
    words = rng.integers(0, 2 ** 32, (n, wpr), dtype=np.uint64).astype(np.uint32)
    for j in range(c):
        w, b = j >> 5, np.uint32(1 << (j & 31))
        words[:, w] = np.where(y[:, j], words[:, w] | b, words[:, w] & ~b)
    rows = np.arange(n, dtype=np.int32)
    got = dev.bce_fwd_rows(z, y, rows=rows, training=True, ld=c + 3, words=words)
    zz = z.astype(np.float64)
    a = np.maximum(zz, 0) - y * zz
    l = np.log1p(np.exp(-np.abs(zz)))
    e = 2.5 * EXP_ATOL * l + U * (np.abs(a) + np.abs(a + l))
    within("sigmoid loss", got["loss_sum"], (a + l).sum(), e.sum() + 8 * U * np.abs(a + l).sum(), "loss sum past the cap")
    pos = z > 0
    assert (got["tp"], got["fp"], got["fn"], got["rows"]) == (int((pos & y).sum()), int((pos & ~y).sum()), int((~pos & y).sum()), n)
    assert got["denom"] == np.float32(n * c)
    g = (1 / (1 + np.exp(-zz)) - y) / (float(n) * c)
    within("sigmoid loss", got["grad"], g, np.abs(g) * (EXP_ATOL + 4 * U) + R.DENORM, "gradient past the cap")


# ---- operators that hand the hard rows to an epilogue exactly --------------------------------------------------------------

EPI_C = [1, 3, 7, 8, 9, 41, 64]


def bf16_round(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


class Operator:
    """row i gathers table row i and length - 1 distinct zero rows; every column has degree 1, so the per-edge coefficient is
    f32(1 / sqrtf(length))"""

    def __init__(self, dev, n, length):
        self.n, self.length = n, length
        assert n * length < 128 * 8192                        # plan::split_length: a graph this small cuts rows above 128 edges
        ptr = np.arange(n + 1, dtype=np.int32) * length
        col = np.empty((n, length), np.int32)
        col[:, 0] = np.arange(n)
        col[:, 1:] = n + np.arange(length - 1)
        self.n_cols = n + length - 1
        self.g = dev.graph(ptr, col.ravel(), n_cols=self.n_cols, col_deg=np.ones(self.n_cols, np.int32))
        coef = self.g.coef()
        assert np.all(coef == coef[0])
        self.coef = np.float32(coef[0])
        if length in (1, 256, 4096):
            assert self.coef == np.float32(1.0 / np.sqrt(length)) and float(np.log2(float(self.coef))).is_integer()

    def table(self, z):
        x = np.zeros((self.n_cols, z.shape[1]), np.float32)
        x[:self.n] = z
        return x

    def logits(self, z, scaling):
        """what the aggregation must store, to the bit"""
        return z.copy() if scaling == 3 else (self.coef * z).astype(np.float32)


@pytest.fixture(scope="module")
def operators(dev):
    n = R.hard_rows(7)[0].shape[0]
    assert all(R.hard_rows(c)[0].shape[0] == n for c in EPI_C if c >= 5)
    cache = {}

    def get(n_rows, length):
        if (n_rows, length) not in cache:
            cache[n_rows, length] = Operator(dev, n_rows, length)
        return cache[n_rows, length]
    yield get
    for op in cache.values():
        op.g.free()


def split_name(length):
    return "split" if length > 128 else "unsplit"


@pytest.mark.parametrize("c", [3, 7, 41, 64])
@pytest.mark.parametrize("scaling,length", [(3, 1), (3, 65), (3, 256), (3, 1200), (0, 1), (0, 65), (0, 256), (0, 4096)])
def test_loss_epilogue_on_hard_rows(dev, operators, c, scaling, length):
    """gcnhip_graphsum_ex with a gcnhip_gs_loss + gcnhip_xent_from_row_terms: the stored logits are the intended values, the row
    terms, the gradient rows, the sum of the terms kernel and the counts are inside the reference's bounds, and all of it has
    the bits of gcnhip_xent_fwd_rows_scaled on the stored logits"""
    z, t = R.hard_rows(c)
    n = z.shape[0]
    op = operators(n, length)
    x, zz = op.table(z), op.logits(z, scaling)
    fam = "loss epilogue " + split_name(length)
    rng = np.random.default_rng(c + length)
    scale = (rng.random(n) + 0.5).astype(np.float32)
    w4 = 4 * ((c + 3) // 4)
    tame = R.tame_rows(zz)
    for which in ("all", "subset", "tame"):
        tt = t.copy()
        if which == "all":
            tt[[1, 9]] = -1                                   # computed, not scored: zero terms and a zero gradient row
        if which == "subset":
            tt[rng.random(n) < 0.4] = -1
        if which == "tame":
            tt[~tame] = -1
        scored = tt >= 0
        rs = op.g.add_rowset(scored) if which != "all" else None
        for training in (True, False):
            for sc in (None, scale):
                ref = R.reference(zz, tt, row_scale=sc)
                a = dev.graphsum_loss(op.g, x, scaling, tt, rows=rs, training=training, grad_row_scale=sc, epilogue=True, grad_fill=7.0)
                b = dev.graphsum_loss(op.g, x, scaling, tt, rows=rs, training=training, grad_row_scale=sc, epilogue=False, grad_fill=7.0)
                computed = scored if rs is not None else np.ones(n, bool)
                assert np.array_equal(bits(a["logits"][computed]), bits(zz[computed])), "the operator does not return the hard rows"
                assert np.all(np.isnan(a["logits"][~computed]))
                within(fam, a["terms"][scored, 0], ref["term"][scored], ref["E_term"][scored], "row terms")
                assert np.array_equal(a["terms"][scored, 1] != 0, ref["correct"][scored])
                assert np.all(bits(a["terms"][computed & ~scored]) == 0) and np.all(np.isnan(a["terms"][~computed]))
                want, bound = R.loss_sum(ref)
                within("terms kernel", a["loss_sum"], want, bound, "sum of the row terms")
                assert (a["correct"], a["total"]) == (int(ref["correct"].sum()), int(scored.sum())) == (b["correct"], b["total"])
                assert np.array_equal(bits(a["res"]), bits(b["res"])), (a["res"], b["res"])
                ga, gb = a["grad"], b["grad"]
                if training:
                    within(fam, ga[scored, :c], ref["grad"][scored], ref["E_grad"][scored], "gradient")
                    assert np.all(bits(ga[scored, c:w4]) == 0) and np.all(ga[:, w4:] == 7.0)
                    assert np.all(bits(ga[computed & ~scored, :w4]) == 0) and np.all(ga[~computed] == 7.0)
                    assert np.array_equal(bits(ga[scored]), bits(gb[scored])), "the epilogue and the loss kernel differ"
                else:
                    assert np.all(ga == 7.0)
                again = dev.graphsum_loss(op.g, x, scaling, tt, rows=rs, training=training, grad_row_scale=sc, epilogue=True, grad_fill=7.0)
                assert all(np.array_equal(bits(a[k]), bits(again[k])) for k in ("res", "grad", "terms"))
        if rs is not None:
            op.g.remove_rowset(rs)


@pytest.mark.parametrize("c", EPI_C)
@pytest.mark.parametrize("path,length", [("per-edge", 1), ("per-edge", 65), ("per-edge", 256), ("per-edge", 4096),
                                         ("factored", 1), ("factored", 65), ("factored", 256), ("factored", 1200),
                                         ("bf16", 1), ("bf16", 65), ("bf16", 256), ("bf16", 4096)])
def test_predict_epilogue_on_hard_rows(dev, operators, c, path, length):
    """gcnhip_graphsum_predict: pred is exact (the lowest class among the maxima), prob and logp inside their bounds, rows outside
    a subset untouched, and the same pred / prob bits without logp and without the stored logits"""
    z, _ = R.hard_rows(c)
    n = z.shape[0]
    op = operators(n, length)
    if path == "bf16":
        zb = bf16_round(z)
        ld8 = (c + 7) // 8 * 8
        tb = np.zeros((op.n_cols, ld8), np.uint16)
        tb[:n, :c] = (zb.view(np.uint32) >> 16).astype(np.uint16)
        kw, zz = dict(table_bf16=tb, dim=c), op.logits(zb, 0)
    else:
        scaling = 0 if path == "per-edge" else 3
        kw, zz = dict(x=op.table(z), scaling=scaling), op.logits(z, scaling)
    fam = "predict epilogue " + ("split" if length > 128 else ("bf16" if path == "bf16" else "f32"))
    ref = R.reference(zz, np.zeros(n, np.int32))
    subset = np.random.default_rng(c).random(n) < 0.5
    rs = op.g.add_rowset(subset)
    for rows, mask in ((None, np.ones(n, bool)), (rs, subset)):
        got = dev.graphsum_predict(op.g, rows=rows, **kw)
        assert np.array_equal(bits(got["logits"][mask]), bits(zz[mask])), "the operator does not return the hard rows"
        assert np.all(np.isnan(got["logits"][~mask])) and np.all(got["pred"][~mask] == -1)
        assert np.all(np.isnan(got["prob"][~mask])) and np.all(np.isnan(got["logp"][~mask]))
        assert np.array_equal(got["pred"][mask], ref["pred"][mask])
        within(fam, got["prob"][mask], ref["prob"][mask], ref["E_prob"][mask], "prob")
        within(fam, got["logp"][mask], ref["logp"][mask], ref["E_logp"][mask], "logp")
        for logp, store in ((False, False), (True, False), (False, True)):
            lean = dev.graphsum_predict(op.g, rows=rows, logp=logp, store_logits=store, **kw)
            assert np.array_equal(lean["pred"], got["pred"]) and np.array_equal(bits(lean["prob"]), bits(got["prob"]))
            if logp:
                assert np.array_equal(bits(lean["logp"]), bits(got["logp"]))
        again = dev.graphsum_predict(op.g, rows=rows, **kw)
        assert all(np.array_equal(again[k].view(np.uint32), got[k].view(np.uint32)) for k in ("pred", "prob", "logp", "logits"))
    op.g.remove_rowset(rs)


@pytest.mark.parametrize("c", EPI_C)
def test_attach_predict_on_hard_rows(dev, operators, c):
    """gcnhip_attach_gather with the predict epilogue: one edge of coefficient 1 per row, and three 600-edge rows (the four-wave
    form) whose other columns are zero rows; beta 1, 0.5 and 3; both load paths.  At beta = 1 the bits of gcnhip_graphsum_predict
    on the same logits; at beta != 1 attach_finish and gcnhip_calib_scale_rows applied to the beta = 1 log-softmax rows are both
    inside calib_ref.scale's bounds on those rows (not the same bits: the module docstring)."""
    z, _ = R.hard_rows(c)
    n = z.shape[0]
    long_of = [9, n - 1, n // 2]                              # a wide row, an underflow row, a tie (or constant) row
    zeros = 599
    ta = np.concatenate([z, np.zeros((zeros, c), np.float32)])
    m = n + len(long_of)
    tb = np.zeros((m, c), np.float32)
    rng = np.random.default_rng(c)
    cols = [[i] for i in range(n)] + [[i] + list(n + np.arange(zeros)) for i in long_of]
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in cols])]).astype(np.int32)
    col = np.concatenate(cols).astype(np.int32)
    coef = (rng.random(col.size) + 0.5).astype(np.float32)
    coef[ptr[:-1]] = 1.0                                      # the hard row's own edge comes first in every row
    zz = np.concatenate([z, z[long_of]])
    op = operators(n, 1)
    base = dev.graphsum_predict(op.g, x=op.table(z), scaling=3)
    pad = (c + 3) // 4 * 4
    first = None
    for beta in (1.0, 0.5, 3.0):
        ref = R.reference(zz, np.zeros(m, np.int32), beta=beta)
        for ld in (c, pad):
            got = dev.attach_gather(ptr, col, coef, ta, tb, epilogue="predict", beta=beta, ld_a=ld, ld_b=ld, ld_out=ld, logp=True)
            assert np.array_equal(bits(got["z"]), bits(zz)), "the gather does not return the hard rows"
            assert np.array_equal(got["pred"], ref["pred"])
            if beta == 1.0:
                within("attach predict", got["prob"], ref["prob"], ref["E_prob"], "prob")
                within("attach predict", got["logp"], ref["logp"], ref["E_logp"], "logp")
                assert np.array_equal(got["pred"][:n], base["pred"]) and np.array_equal(bits(got["prob"][:n]), bits(base["prob"]))
                assert np.array_equal(bits(got["logp"][:n]), bits(base["logp"])), "attach_finish and the predict epilogue differ"
                first = first or got
            else:
                within("attach predict", got["prob"], ref["sprob"], ref["E_sprob"], f"prob at beta {beta}")
                within("attach predict", got["logp"], ref["scaled"], ref["E_scaled"], f"logp at beta {beta}")
                # calib_scale_kernel on the beta = 1 rows: NOT the same bits (it adds in a shuffle tree, attach_finish left to
                # right; see the module docstring) — both are held to float64 on exactly these f32 rows instead
                out, prob = dev.calib_scale_rows(first["logp"], beta)
                o, e_o, pr, e_pr = calib_ref.scale(first["logp"], calib_ref.f32(beta))
                within("calib scale of the attach rows", out, o, e_o, f"logp at beta {beta}")
                within("calib scale of the attach rows", prob, pr, e_pr, f"prob at beta {beta}")
                # (calib_ref's eps_Z has 8 U for the kernel's tree sum; the left-to-right sum of C terms gets the any-order bound)
                more = max(0.0, 1.01 * (c - 1) - 8) * U
                within("attach predict", got["logp"], o, e_o + more, f"logp at beta {beta} against its own beta = 1 rows")
                within("attach predict", got["prob"], pr, e_pr + pr * 1.01 * more, f"prob at beta {beta} against its own beta = 1 rows")
            for k in ("pred", "prob", "logp"):                # both load paths, two launches, the long rows and their short twins
                assert np.array_equal(got[k].view(np.uint32)[n:], got[k].view(np.uint32)[long_of])
            lean = dev.attach_gather(ptr, col, coef, ta, tb, epilogue="predict", beta=beta, ld_a=ld, ld_b=ld, store=False)
            assert np.array_equal(lean["pred"], got["pred"]) and np.array_equal(bits(lean["prob"]), bits(got["prob"]))
            if ld == c:
                unaligned = got
            else:
                assert all(np.array_equal(unaligned[k].view(np.uint32), got[k].view(np.uint32)) for k in ("pred", "prob", "logp"))


@pytest.mark.parametrize("c", [7, 100])
@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_one_non_finite_logit_stays_in_its_row(dev, operators, c, bad):
    """+inf, -inf and NaN in one column of one scored row of a mild table: every other row's gradient bits, row terms, pred, prob
    and logp are those of the run without it (the bad row's own outputs are compared with nothing)"""
    n = R.hard_rows(7)[0].shape[0]                            # the operators of the other tests
    rng = np.random.default_rng(c)
    z = (rng.standard_normal((n, c)) * 3).astype(np.float32)
    t = rng.integers(0, c, n).astype(np.int32)
    t[rng.random(n) < 0.3] = -1
    row = 17
    t[row] = 2
    zb = z.copy()
    zb[row, 3] = bad
    others = np.arange(n) != row
    for ld in (c, (c + 3) // 4 * 4):
        runs = [dev.xent_call("fwd", table_of(q, ld), t, c, grad=filled((n, ld)), training=True, count=0) for q in (z, zb)]
        assert runs[0]["rc"] == 0 and runs[1]["rc"] == 0
        assert np.array_equal(bits(runs[0]["grad"][others]), bits(runs[1]["grad"][others]))
        assert runs[0]["result_i"][1] == runs[1]["result_i"][1]
        rows = np.flatnonzero(t >= 0).astype(np.int32)
        for keep in (rows, rows[rows != row]):
            runs = [dev.xent_call("rows", table_of(q, ld), t, c, grad=filled((n, ld)), rows=keep, training=True, count=keep.size) for q in (z, zb)]
            assert np.array_equal(bits(runs[0]["grad"][others]), bits(runs[1]["grad"][others]))
            if keep.size < rows.size:                          # the bad row is not listed: nothing at all changes
                assert all(np.array_equal(runs[0][k].view(np.uint32), runs[1][k].view(np.uint32)) for k in ("result", "result_i", "grad"))
    if c > 64:
        return
    for length in (1, 256):
        op = operators(n, length)
        a, b = (dev.graphsum_loss(op.g, op.table(q), 3, t, training=True, epilogue=True, grad_fill=7.0) for q in (z, zb))
        assert np.array_equal(bits(a["logits"][others]), bits(b["logits"][others]))
        assert np.array_equal(bits(a["grad"][others]), bits(b["grad"][others])) and np.array_equal(bits(a["terms"][others]), bits(b["terms"][others]))
        assert a["total"] == b["total"]
        a, b = (dev.graphsum_predict(op.g, x=op.table(q), scaling=3) for q in (z, zb))
        for k in ("pred", "prob", "logp"):
            assert np.array_equal(a[k][others].view(np.uint32), b[k][others].view(np.uint32)), k
