"""The element-wise layer AS LAUNCHED by the model (csrc/elementwise.hip, and the bf16 converter of csrc/graphsum.hip) against
the float64 references of tests/elementwise_ref.py: Adam from non-zero state with m and v looked at, the step-size table and
the epoch word the launch advances, variable boundaries at every place a fused index can split, the capped grids of Adam and
the sum of squares with their empty trailing blocks, the strided ReLU / Dropout forms with their two indices, and the special
values of the bf16 converter.  Every tolerance comes from elementwise_ref (its docstring has the derivations); whatever is
claimed to hold bit for bit is asserted on the bit patterns.  tests/test_elementwise_cpu.py shows, without a GPU, that these
bounds reject each subtly wrong kernel on these very inputs."""
import numpy as np
import pytest

from tests import elementwise_ref as R
from tests.test_ops_gpu import philox_keep, thr_of

pytestmark = pytest.mark.gpu

STEP = R.step_size(0.01, 0.9, 0.999, 3)
bits = R.bits


@pytest.fixture(scope="module")
def dev():
    from cuda_gcn_amd.ops import Device
    d = Device(0)
    yield d
    d.close()


def adam_once(dev, ws, gs, ms, vs, flags, hyper, step=STEP, **kw):
    b1, b2, eps, wd = hyper
    return dev.adam_step_state(ws, gs, ms, vs, flags, step_size=step, weight_decay=wd, beta1=b1, beta2=b2, eps=eps, **kw)


def same_result(a, b):
    """w, m, v of every variable and sumsq: the same bits"""
    return all(np.array_equal(bits(x), bits(y)) for key in ("w", "m", "v") for x, y in zip(a[key], b[key])) and \
        np.array_equal(bits(np.float32(a["sumsq"])), bits(np.float32(b["sumsq"])))


def check_against_reference(r, ws, gs, ms, vs, flags, hyper, step=STEP):
    for k in range(len(ws)):
        viol = R.adam_violations(ws[k], gs[k], ms[k], vs[k], flags[k], step, hyper, r["w"][k], r["m"][k], r["v"][k])
        print(f"  variable {k} ({ws[k].size} elements, decay {flags[k]}): violation w {viol[0]:.3e} m {viol[1]:.3e} v {viol[2]:.3e}")
        assert max(viol) <= 0, (k, viol)
    blocks, chunk = R.adam_grid(sum(w.size for w in ws))
    want = R.sumsq_f64(r["w"][0])
    bound = R.sumsq_bound(ws[0].size, blocks, chunk, want)
    print(f"  sumsq {float(r['sumsq']):.9e} float64 {want:.9e} bound {bound:.3e}")
    assert abs(float(r["sumsq"]) - want) <= bound


# ------------------------------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize("hyper", [R.HYPER_MODEL, R.HYPER_INEXACT], ids=["model", "inexact-1-minus-beta"])
@pytest.mark.parametrize("case", range(len(R.LAYOUTS) + 1))
def test_adam_one_step_from_given_state(dev, case, hyper):
    """one step from random non-zero m and v >= 0: w, m and v of every variable inside adam_step_ref's bounds, sum(w0^2) of
    variable 0 alone inside sumsq_bound, and the last-block sum equal to the second launch bit for bit (adam_sum_launch).
    The betas of 0.4 are the set at which 1 - beta formed in float differs from the double."""
    layout, flags = (R.LAYOUTS + [R.BOUNDARY_LAYOUT])[case]
    ws, gs, ms, vs = R.adam_state(layout, 20 + case)
    out = []
    try:
        for two in (0, 1):
            dev.set_option("adam_sum_launch", two)
            print(f"layout {layout} flags {flags} adam_sum_launch {two}")
            out.append(adam_once(dev, ws, gs, ms, vs, flags, hyper))
            check_against_reference(out[-1], ws, gs, ms, vs, flags, hyper)
    finally:
        dev.set_option("adam_sum_launch", 0)
    assert same_result(out[0], out[1])


def test_adam_edge_values(dev):
    edge = R.adam_edge_states()
    # g = m = v = 0: nothing moves, bit for bit
    w, g, m, v, decay, hyper = edge["zero"]
    r = adam_once(dev, [w], [g], [m], [v], [decay], hyper)
    assert np.array_equal(bits(r["w"][0]), bits(w)) and not bits(r["m"][0]).any() and not bits(r["v"][0]).any()
    # g = 1e20: grad . grad is a double product — v' is finite and the reference's
    w, g, m, v, decay, hyper = edge["double_square"]
    r = adam_once(dev, [w], [g], [m], [v], [decay], hyper)
    assert np.all(np.isfinite(r["v"][0])) and np.all(r["v"][0] > 9e36)
    check_against_reference(r, [w], [g], [m], [v], [decay], hyper)
    # (1 - beta2) g^2 above the f32 range: v' = +inf, and w' = w - step m' / inf stays w, bit for bit
    w, g, m, v, decay, hyper = edge["overflow"]
    r = adam_once(dev, [w], [g], [m], [v], [decay], hyper)
    assert np.all(r["v"][0] == np.inf) and np.all(np.isfinite(r["m"][0])) and np.all(np.isfinite(r["w"][0]))
    assert np.array_equal(bits(r["w"][0]), bits(w))
    check_against_reference(r, [w], [g], [m], [v], [decay], hyper)
    # wd = 0: the decay flag changes no bit
    w, g, m, v, _, hyper = edge["no_wd"]
    a = adam_once(dev, [w], [g], [m], [v], [1], hyper)
    b = adam_once(dev, [w], [g], [m], [v], [0], hyper)
    assert same_result(a, b)
    check_against_reference(a, [w], [g], [m], [v], [1], hyper)


@pytest.mark.parametrize("e", [0, 5, 15])
def test_adam_reads_the_step_size_table_at_the_epoch_word(dev, e):
    """d_step_sizes[*d_epoch]: the table is NaN except at index e, the scalar argument is NaN too, and the result is the scalar
    call's with that entry, bit for bit; gcnhip_adam_step leaves the epoch words alone"""
    layout, flags = R.LAYOUTS[3]
    ws, gs, ms, vs = R.adam_state(layout, 31)
    table = np.full(16, np.nan, np.float32)
    table[e] = np.float32(STEP)
    tb = dev.buf(table)
    words = dev.buf(np.array([e, 0xFFFFFFFF], np.uint32))
    want = adam_once(dev, ws, gs, ms, vs, flags, R.HYPER_MODEL, step=STEP)
    got = adam_once(dev, ws, gs, ms, vs, flags, R.HYPER_MODEL, step=np.nan, step_table=tb, epoch_words=words)
    assert np.all(np.isfinite(got["w"][0])) and same_result(got, want)
    assert words.download().tolist() == [e, 0xFFFFFFFF]
    check_against_reference(got, ws, gs, ms, vs, flags, R.HYPER_MODEL)


@pytest.mark.parametrize("case", [3, 5], ids=["four-variables", "block-cap"])
@pytest.mark.parametrize("two", [0, 1])
def test_adam_as_the_model_launches_it(dev, case, two):
    """HipAdam::step's form: gcnhip_adam_step_advance with the table, d_epoch the very word the launch advances, four times from
    counter = 3, done = 0xFFFFFFFF.  Afterwards counter = 7 and done = 6, and after every step w, m, v and sumsq are the bits of
    a scalar-step gcnhip_adam_step call with tab[3 + k] (every block read the word before the last block moved it)"""
    layout, flags = R.LAYOUTS[case]
    ws, gs, ms, vs = R.adam_state(layout, 41)
    rng = np.random.default_rng(42)
    grads = [[rng.standard_normal(n).astype(np.float32) for n in layout] for _ in range(4)]
    table = np.array([R.step_size(0.01, 0.9, 0.999, t) for t in range(1, 9)], np.float32)
    assert np.unique(table).size == table.size
    tb = dev.buf(table)
    words = dev.buf(np.array([3, 0xFFFFFFFF], np.uint32))
    try:
        dev.set_option("adam_sum_launch", two)
        model = scalar = None
        for k in range(4):
            model = adam_once(dev, ws, grads[k], ms, vs, flags, R.HYPER_MODEL, step=np.nan, step_table=tb, epoch_words=words, advance=True,
                              state=model["state"] if model else None)
            scalar = adam_once(dev, ws, grads[k], ms, vs, flags, R.HYPER_MODEL, step=float(table[3 + k]), state=scalar["state"] if scalar else None)
            assert same_result(model, scalar), k
            assert words.download().tolist() == [4 + k, 3 + k]
        assert words.download().tolist() == [7, 6]
        assert np.all(np.isfinite(model["w"][0])) and not np.array_equal(model["w"][0], ws[0])
    finally:
        dev.set_option("adam_sum_launch", 0)


# -------------------------------------------------------------------------------------------------------- sum of squares
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097, 1024 * 4096 + 1])
def test_sumsq_inside_its_bound_and_reproducible(dev, n):
    """gcnhip_sumsq up to the block cap (1024 blocks of 4352 with a remainder: the trailing blocks are empty)"""
    x = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    want = R.sumsq_f64(x)
    blocks, chunk = R.sumsq_grid(n)
    bound = R.sumsq_bound(n, blocks, chunk, want)
    a, b = np.float32(dev.sumsq(x)), np.float32(dev.sumsq(x))
    print(f"n {n}: sumsq {float(a):.9e} float64 {want:.9e} bound {bound:.3e}")
    assert abs(float(a) - want) <= bound
    assert np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------- strided ReLU / Dropout
SHAPES = [(300, cols, ld) for cols in (1, 7, 41) for ld in (cols, cols + 1, 48)] + [(13001, 41, 44)]     # the last: a second grid-stride pass


def matrix(rows, cols, seed):
    """random f32 [rows, cols] with -0.0, +0.0 and NaN sprinkled in"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, cols)).astype(np.float32)
    kind = rng.integers(0, 40, (rows, cols))
    x[kind == 0], x[kind == 1], x[kind == 2] = -0.0, np.nan, 0.0
    x[0, 0], x[rows - 1, cols - 1], x[rows // 2, cols // 2] = np.nan, -0.0, 1.5
    return x


def padding_kept(buf, cols):
    return bool(np.all(bits(buf)[:, cols:] == R.PAD_BITS))


@pytest.mark.parametrize("rows,cols,ld", SHAPES)
def test_relu_strided(dev, rows, cols, ld):
    x, g = matrix(rows, cols, rows + cols), matrix(rows, cols, ld)
    xb, gb = R.padded(x, ld), R.padded(g, ld)
    want, want_mask = R.relu_fwd_2d_ref(xb, cols)
    got, mask = dev.relu_fwd_2d(xb, cols, training=True, mask_fill=0xAB)
    assert np.array_equal(mask, want_mask)                                   # mask[r . cols + c]
    assert np.array_equal(bits(got), bits(want)) and padding_kept(got, cols)  # kept values bit-unchanged, every padding word too
    with np.errstate(invalid="ignore"):
        dropped = ~(x > 0)
    assert dropped[0, 0] and dropped[rows - 1, cols - 1] and not bits(got)[:, :cols][dropped].any()   # NaN, -0.0 -> +0.0
    got_eval, mask_eval = dev.relu_fwd_2d(xb, cols, training=False, mask_fill=0xAB)
    assert np.array_equal(bits(got_eval), bits(want)) and np.all(mask_eval == 0xAB)
    back = dev.relu_bwd_2d(gb, cols, mask)
    assert np.array_equal(bits(back), bits(R.relu_bwd_2d_ref(gb, cols, want_mask))) and padding_kept(back, cols)
    assert np.array_equal(bits(back)[:, :cols][~dropped], bits(g)[~dropped])


@pytest.mark.parametrize("rows,cols,ld", SHAPES)
def test_dropout_strided(dev, rows, cols, ld):
    x, g = matrix(rows, cols, rows + cols + 1), matrix(rows, cols, ld + 1)
    xb, gb = R.padded(x, ld), R.padded(g, ld)
    n = rows * cols
    seed, epoch, off = 42, 5, 12345
    for p in (0.5, 0.1, 0.0):
        scale = np.float32(1) / (np.float32(1) - np.float32(p))
        keep = philox_keep(seed, epoch, np.arange(n, dtype=np.uint64) + np.uint64(off), thr_of(p))
        got, mask = dev.dropout_fwd_2d(xb, cols, p, seed=seed, epoch=epoch, elem_offset=off)
        assert np.array_equal(mask != 0, keep) and set(np.unique(mask).tolist()) <= {0, 1}      # the stream at elem_offset + r . cols + c
        want, _ = R.dropout_fwd_2d_ref(xb, cols, keep, scale)
        assert R.same_bits_or_nan(got[:, :cols], want[:, :cols]) and padding_kept(got, cols)
        flat, flat_mask = dev.dropout_fwd(x, p, seed=seed, epoch=epoch, elem_offset=off)      # the flat form on the packed matrix
        assert np.array_equal(bits(np.ascontiguousarray(got[:, :cols])).ravel(), bits(flat)) and np.array_equal(mask, flat_mask)
        nomask, none = dev.dropout_fwd_2d(xb, cols, p, seed=seed, epoch=epoch, elem_offset=off, want_mask=False)
        assert none is None and np.array_equal(bits(nomask), bits(got))
        back = dev.dropout_bwd_2d(gb, cols, mask, p)
        assert np.array_equal(bits(np.ascontiguousarray(back[:, :cols])).ravel(), bits(dev.dropout_bwd(g, mask, p))) and padding_kept(back, cols)
        assert R.same_bits_or_nan(back[:, :cols], R.dropout_bwd_2d_ref(gb, cols, mask, scale)[:, :cols])
    # injected decisions are read at r . cols + c
    keep_in = (np.random.default_rng(ld).random(n) < 0.6).astype(np.uint8)
    got, mask = dev.dropout_fwd_2d(xb, cols, 0.25, keep_in=keep_in)
    want, want_mask = R.dropout_fwd_2d_ref(xb, cols, keep_in, np.float32(1) / (np.float32(1) - np.float32(0.25)))
    assert np.array_equal(mask, want_mask) and R.same_bits_or_nan(got[:, :cols], want[:, :cols]) and padding_kept(got, cols)


@pytest.mark.parametrize("rows,ld_grad,ld_h,dim", [(333, 20, 16, 16), (333, 16, 24, 16), (333, 44, 48, 41), (13001, 44, 48, 41)])
def test_relu_dropout_bwd_strided(dev, rows, ld_grad, ld_h, dim):
    """exactly where(h > 0, g . scale, 0) with two different row strides; the padding of grad untouched (h's is NaN: never read
    as data).  The last shape takes a second grid-stride pass."""
    h = matrix(rows, dim, ld_h)
    g = np.random.default_rng(ld_grad).standard_normal((rows, dim)).astype(np.float32)
    gb, hb = R.padded(g, ld_grad), R.padded(h, ld_h)
    got = dev.relu_dropout_bwd(gb, hb, 2.0, ld_grad=ld_grad, ld_h=ld_h, dim=dim)
    with np.errstate(invalid="ignore"):
        want = np.where(h > 0, g * np.float32(2), np.float32(0)).astype(np.float32)
    assert np.array_equal(bits(np.ascontiguousarray(got[:, :dim])), bits(want)) and padding_kept(got, dim)
    assert np.array_equal(bits(got), bits(R.relu_dropout_bwd_ref(gb, hb, dim, 2.0)))


# ------------------------------------------------------------------------------------------------------------------ bf16
def check_specials(codes, where):
    for (bits_in, want), code in zip(R.BF16_SPECIALS, codes):
        if want is None:
            assert R.bf16_is_nan(code) and (int(code) >> 15) == (bits_in >> 31), (where, hex(bits_in), hex(int(code)))
        else:
            assert int(code) == want, (where, hex(bits_in), hex(int(code)))


def test_f32_to_bf16_specials_in_one_row(dev):
    x = np.array([s[0] for s in R.BF16_SPECIALS], np.uint32).view(np.float32).reshape(1, 16)
    check_specials(dev.to_bf16(x, ld_dst=16)[0], "row")


def test_f32_to_bf16_specials_in_a_second_grid_stride_pass(dev):
    """one column in rows of 8 codes: more than 65536 . 256 eight-element groups, so the capped grid takes a second pass; the
    specials sit in the first pass and in the second, the other columns of every row are written as 0"""
    first = 65536 * 256
    rows = first + 300
    special = np.array([s[0] for s in R.BF16_SPECIALS], np.uint32).view(np.float32)
    x = np.tile(np.random.default_rng(6).standard_normal(1 << 16).astype(np.float32), rows // (1 << 16) + 1)[:rows].copy()
    x[3:3 + special.size] = special
    x[first + 7:first + 7 + special.size] = special
    tab = dev.to_bf16(x.reshape(rows, 1), ld_dst=8)
    check_specials(tab[3:3 + special.size, 0], "first pass")
    check_specials(tab[first + 7:first + 7 + special.size, 0], "second pass")
    want = R.bf16_ref(x)
    nan = R.bf16_is_nan(want)
    assert np.array_equal(tab[:, 0][~nan], want[~nan]) and np.all(R.bf16_is_nan(tab[:, 0][nan]))
    assert not tab[:, 1:].any()
