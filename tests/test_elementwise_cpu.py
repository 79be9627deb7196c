"""The float64 references and bounds of the element-wise layer (tests/elementwise_ref.py) against the CPU oracle and the golden
fixtures, the f32 emulation of adam_kernel inside the bounds, and — the evidence that the GPU tests of test_elementwise_gpu.py
would fail on a subtly wrong kernel — every mutant of the emulation OUTSIDE them, on the inputs the GPU tests use.  No GPU."""
import os

import numpy as np
import pytest

from tests import elementwise_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STEP = R.step_size(0.01, 0.9, 0.999, 3)


def worst(ws, gs, ms, vs, flags, step, hyper, got):
    """(viol_w, viol_m, viol_v): the largest violation over the variables of a layout (<= 0: inside the bounds)"""
    w2, m2, v2 = got[:3]
    per_var = [R.adam_violations(ws[k], gs[k], ms[k], vs[k], flags[k], step, hyper, w2[k], m2[k], v2[k]) for k in range(len(ws))]
    return tuple(max(p[j] for p in per_var) for j in range(3))


def test_reference_contains_the_oracle_and_the_golden_fixtures_step_by_step(oracle):
    """carrying the oracle's f32 state (w, m, v) from step to step, every step of or_adam_step_var lies inside adam_step_ref's
    bounds from the state before it; the tenth w is the golden fixture (the reference's own run) bit for bit"""
    mods = np.load(os.path.join(GOLD, "modules.npz"))
    rng = np.random.default_rng(4)
    runs = [(mods["adam_w0"], mods["adam_grads"], 1, mods["adam_w_decay"]), (mods["adam_w0"], mods["adam_grads"], 0, mods["adam_w_nodecay"]),
            (rng.standard_normal(777).astype(np.float32), rng.standard_normal((6, 777)).astype(np.float32), 1, None),
            (rng.standard_normal(777).astype(np.float32) * 50, rng.standard_normal((6, 777)).astype(np.float32) * 1e-3, 0, None)]
    for w0, grads, decay, golden in runs:
        w, m, v = w0.copy(), np.zeros_like(w0), np.zeros_like(w0)
        for t in range(1, grads.shape[0] + 1):
            w2, m2, v2 = oracle.adam_steps(w0, grads[:t], decay, 0.01, 5e-4)
            step = R.step_size(0.01, 0.9, 0.999, t)
            viol = R.adam_violations(w, grads[t - 1], m, v, decay, step, (0.9, 0.999, 1e-8, 5e-4), w2, m2, v2)
            assert max(viol) <= 0, (t, decay, viol)
            w, m, v = w2, m2, v2
        if golden is not None:
            assert np.array_equal(R.bits(w), R.bits(golden))


@pytest.mark.parametrize("hyper", [R.HYPER_MODEL, R.HYPER_INEXACT])
def test_emulation_stays_inside_the_bounds_on_random_states(hyper):
    """on random states of every layout of the GPU tests (the million-element ones too), at several scales of the moments"""
    for li, (layout, flags) in enumerate(R.LAYOUTS):
        for scale_m in (0.1, 1e-4, 30.0):
            ws, gs, ms, vs = R.adam_state(layout, 100 + li, scale_m)
            got = R.adam_kernel_emul(ws, gs, ms, vs, flags, STEP, hyper)
            assert max(worst(ws, gs, ms, vs, flags, STEP, hyper, got)) <= 0, (layout, scale_m)
            blocks, chunk = R.adam_grid(sum(layout))
            want = R.sumsq_f64(got[0][0])
            assert abs(got[3] - want) <= R.sumsq_bound(layout[0], blocks, chunk, want)


def test_emulation_stays_inside_the_bounds_on_the_edge_states():
    """the edge values of the GPU tests: all-zero state leaves w alone, g = 1e20 gives a finite v', g = 1e21 gives v' = +inf and
    w' = w, wd = 0 makes the decay flag irrelevant — each inside the bounds, and exactly so where the GPU test asserts bits"""
    edge = R.adam_edge_states()
    for name, (w, g, m, v, decay, hyper) in edge.items():
        got = R.adam_kernel_emul([w], [g], [m], [v], [decay], STEP, hyper)
        assert max(worst([w], [g], [m], [v], [decay], STEP, hyper, got)) <= 0, name
    w, g, m, v, decay, hyper = edge["zero"]
    w2, m2, v2, _ = R.adam_kernel_emul([w], [g], [m], [v], [decay], STEP, hyper)
    assert np.array_equal(R.bits(w2[0]), R.bits(w)) and not m2[0].any() and not v2[0].any()
    w, g, m, v, decay, hyper = edge["double_square"]
    _, _, v2, _ = R.adam_kernel_emul([w], [g], [m], [v], [decay], STEP, hyper)
    assert np.all(np.isfinite(v2[0])) and np.all(v2[0] > 9e36)
    w, g, m, v, decay, hyper = edge["overflow"]
    w2, m2, v2, _ = R.adam_kernel_emul([w], [g], [m], [v], [decay], STEP, hyper)
    assert np.all(v2[0] == np.inf) and np.all(np.isfinite(m2[0])) and np.array_equal(R.bits(w2[0]), R.bits(w))
    (_, _, V), (_, _, ev) = R.adam_step_ref(w, g, m, v, decay, STEP, *hyper)
    assert np.all(V == np.inf) and not ev.any()
    w, g, m, v, decay, hyper = edge["no_wd"]
    a = R.adam_kernel_emul([w], [g], [m], [v], [1], STEP, hyper)
    b = R.adam_kernel_emul([w], [g], [m], [v], [0], STEP, hyper)
    assert all(np.array_equal(R.bits(a[j][0]), R.bits(b[j][0])) for j in range(3))


def test_bounds_reject_a_float_square():
    """g = 1e20: the f32 product g . g is +inf, the double product gives v' ~ 1e37"""
    w, g, m, v, decay, hyper = R.adam_edge_states()["double_square"]
    got = R.adam_kernel_emul([w], [g], [m], [v], [decay], STEP, hyper, mutant="float_square")
    assert np.all(got[2][0] == np.inf)
    assert worst([w], [g], [m], [v], [decay], STEP, hyper, got)[2] == np.inf


def test_bounds_reject_one_minus_beta_formed_in_float():
    """1.0f - beta is exact at the model's 0.9f and 0.999f (that mutant computes the same bits there, which is asserted), so the
    GPU tests run every layout at betas of 0.4 as well, where it is 0.83 u off: m' and v' leave their bounds"""
    for layout, flags in R.LAYOUTS[2:5]:
        ws, gs, ms, vs = R.adam_state(layout, 7)
        same = R.adam_kernel_emul(ws, gs, ms, vs, flags, STEP, R.HYPER_MODEL, mutant="float_one_minus_beta")
        good = R.adam_kernel_emul(ws, gs, ms, vs, flags, STEP, R.HYPER_MODEL)
        assert all(np.array_equal(a, b) for j in range(3) for a, b in zip(same[j], good[j]))
        got = R.adam_kernel_emul(ws, gs, ms, vs, flags, STEP, R.HYPER_INEXACT, mutant="float_one_minus_beta")
        viol = worst(ws, gs, ms, vs, flags, STEP, R.HYPER_INEXACT, got)
        assert viol[1] > 0 and viol[2] > 0, (layout, viol)


@pytest.mark.parametrize("hyper", [R.HYPER_MODEL, R.HYPER_INEXACT])
def test_bounds_reject_decay_on_the_wrong_variable(hyper):
    """every layout whose decay flags differ between variables"""
    for layout, flags in R.LAYOUTS + [R.BOUNDARY_LAYOUT]:
        if len(set(flags)) < 2 or sum(layout) > 100000:
            continue
        ws, gs, ms, vs = R.adam_state(layout, 7)
        got = R.adam_kernel_emul(ws, gs, ms, vs, flags, STEP, hyper, mutant="decay_wrong_variable")
        viol = worst(ws, gs, ms, vs, flags, STEP, hyper, got)
        assert viol[1] > 0 and viol[2] > 0, (layout, viol)


def test_bounds_reject_a_variable_boundary_off_by_one():
    """one element takes its neighbour's decay flag: on the two-variable layout kept for this, and on every mixed layout"""
    for layout, flags in [R.BOUNDARY_LAYOUT] + R.LAYOUTS[2:5]:
        ws, gs, ms, vs = R.adam_state(layout, 7)
        got = R.adam_kernel_emul(ws, gs, ms, vs, flags, STEP, R.HYPER_MODEL, mutant="boundary_off_by_one")
        good = R.adam_kernel_emul(ws, gs, ms, vs, flags, STEP, R.HYPER_MODEL)
        differs = sum(int((a != b).sum()) for a, b in zip(got[1], good[1]))
        assert 1 <= differs <= len(layout) - 1                         # only boundary elements moved
        viol = worst(ws, gs, ms, vs, flags, STEP, R.HYPER_MODEL, got)
        assert viol[1] > 0 and viol[2] > 0, (layout, viol)


def test_bounds_reject_table_index_zero():
    """the GPU test's table: NaN everywhere but at index e; reading index 0 instead gives NaN weights unless e = 0"""
    ws, gs, ms, vs = R.adam_state([300], 7)
    for e in (5, 15):
        tab = np.full(16, np.nan, np.float32)
        tab[e] = STEP
        good = R.adam_kernel_emul(ws, gs, ms, vs, [1], None, R.HYPER_MODEL, table=tab, epoch=e)
        assert max(worst(ws, gs, ms, vs, [1], STEP, R.HYPER_MODEL, good)) <= 0
        got = R.adam_kernel_emul(ws, gs, ms, vs, [1], None, R.HYPER_MODEL, table=tab, epoch=e, mutant="table_index_zero")
        assert worst(ws, gs, ms, vs, [1], STEP, R.HYPER_MODEL, got)[0] == np.inf


def test_bounds_reject_a_sum_of_squares_over_all_variables():
    for layout, flags in R.LAYOUTS + [R.BOUNDARY_LAYOUT]:
        if len(layout) < 2:
            continue
        ws, gs, ms, vs = R.adam_state(layout, 7)
        got = R.adam_kernel_emul(ws, gs, ms, vs, flags, STEP, R.HYPER_MODEL, mutant="sumsq_all_variables")
        blocks, chunk = R.adam_grid(sum(layout))
        want = R.sumsq_f64(got[0][0])
        assert abs(got[3] - want) > R.sumsq_bound(layout[0], blocks, chunk, want), layout


def test_bounds_reject_m_updated_from_the_new_v():
    for layout, flags in R.LAYOUTS[:5]:
        ws, gs, ms, vs = R.adam_state(layout, 7)
        got = R.adam_kernel_emul(ws, gs, ms, vs, flags, STEP, R.HYPER_MODEL, mutant="m_from_new_v")
        assert worst(ws, gs, ms, vs, flags, STEP, R.HYPER_MODEL, got)[1] > 0, layout


def test_a_wrong_moment_is_not_reported_as_a_wrong_weight():
    """E_w is stated against the m', v' that were stored: with m' off by a percent, w' computed from that m' is inside E_w"""
    ws, gs, ms, vs = R.adam_state([300], 7)
    w2, m2, v2, _ = R.adam_kernel_emul(ws, gs, ms, vs, [1], STEP, R.HYPER_MODEL)
    m_bad = (m2[0] * np.float32(1.01)).astype(np.float32)
    w_bad = (ws[0] - np.float32(STEP) * m_bad / (np.sqrt(v2[0]) + np.float32(1e-8))).astype(np.float32)
    vw, vm, vv = R.adam_violations(ws[0], gs[0], ms[0], vs[0], 1, STEP, R.HYPER_MODEL, w_bad, m_bad, v2[0])
    assert vw <= 0 and vm > 0 and vv <= 0


def test_sumsq_bound_follows_the_kernels_tree():
    """depth by hand: n = 1 -> 1 + 9 + 1 + 9; the capped grids of Adam (1024 blocks of 1280) and gcnhip_sumsq (1024 of 4352)"""
    assert R.sumsq_grid(1) == (1, 256) and R.sumsq_depth(1, 1, 256) == 20
    assert R.sumsq_grid(4097) == (2, 2304) and R.sumsq_depth(4097, 2, 2304) == 9 + 9 + 1 + 9
    assert R.sumsq_grid(1024 * 4096 + 1) == (1024, 4352) and R.sumsq_depth(1024 * 4096 + 1, 1024, 4352) == 17 + 9 + 4 + 9
    assert R.adam_grid(1024 * 1024 + 1) == (1024, 1280) and R.adam_grid(300) == (1, 512) and R.adam_grid(1419) == (2, 768)
    assert R.sumsq_bound(1, 1, 256) == 21 * R.EPS_F32 and R.sumsq_bound(1, 1, 256, 3.0) == 63 * R.EPS_F32
    # an f32 tree of that shape is inside the bound; a single dropped term of average size is not
    rng = np.random.default_rng(2)
    x = rng.standard_normal(4097).astype(np.float32)
    blocks, chunk = R.sumsq_grid(x.size)
    sq = np.zeros(blocks * chunk, np.float32)
    sq[:x.size] = x * x
    lanes = sq.reshape(blocks, chunk // 256, 256)
    acc = np.zeros((blocks, 256), np.float32)
    for j in range(lanes.shape[1]):
        acc = acc + lanes[:, j]
    part = acc.sum(axis=1, dtype=np.float32)
    got, want = float(part.sum(dtype=np.float32)), R.sumsq_f64(x)
    bound = R.sumsq_bound(x.size, blocks, chunk, want)
    assert abs(got - want) <= bound < want / x.size


def test_strided_references_agree_with_the_flat_ones_on_packed_data():
    """ld == cols: the strided references are the flat ones; ld > cols: the same values at r . ld + c, the padding bit-unchanged"""
    rng = np.random.default_rng(3)
    rows, cols = 37, 7
    x = rng.standard_normal((rows, cols)).astype(np.float32)
    x[0, 0], x[1, 2], x[5, 6] = -0.0, np.nan, 0.0
    g = rng.standard_normal((rows, cols)).astype(np.float32)
    keep = rng.random(rows * cols) < 0.6
    scale = np.float32(1) / (np.float32(1) - np.float32(0.4))
    y, mask = R.relu_fwd_ref(x)
    assert R.bits(y)[0] == 0 and R.bits(y)[cols + 2] == 0 and mask[0] == 0 and mask[cols + 2] == 0          # -0.0 and NaN -> +0.0
    assert np.array_equal(R.bits(y)[mask != 0], R.bits(x).ravel()[mask != 0])
    dy, dmask = R.dropout_fwd_ref(x, keep, scale)
    for ld in (cols, cols + 1, 16):
        xb, gb = R.padded(x, ld), R.padded(g, ld)
        yb, mask2 = R.relu_fwd_2d_ref(xb, cols)
        assert np.array_equal(R.bits(yb[:, :cols]).ravel(), R.bits(y)) and np.array_equal(mask2, mask)
        assert np.all(R.bits(yb[:, cols:]) == R.PAD_BITS) and np.all(R.bits(xb[:, cols:]) == R.PAD_BITS)
        assert np.array_equal(R.bits(R.relu_bwd_2d_ref(gb, cols, mask)[:, :cols]).ravel(), R.bits(R.relu_bwd_ref(g, mask)))
        db, dmask2 = R.dropout_fwd_2d_ref(xb, cols, keep, scale)
        assert R.same_bits_or_nan(np.ascontiguousarray(db[:, :cols]).ravel(), dy) and np.array_equal(dmask2, dmask)
        assert np.all(R.bits(db[:, cols:]) == R.PAD_BITS)
        bb = R.dropout_bwd_2d_ref(gb, cols, dmask, scale)
        assert np.array_equal(R.bits(bb[:, :cols]).ravel(), R.bits(R.dropout_bwd_ref(g, dmask, scale)))
        fb = R.relu_dropout_bwd_ref(gb, R.padded(y.reshape(rows, cols), ld + 3), cols, 2.0)
        assert np.array_equal(fb[:, :cols], np.where(y.reshape(rows, cols) > 0, g * np.float32(2), np.float32(0)))
        assert np.all(R.bits(fb[:, cols:]) == R.PAD_BITS)


def test_bf16_reference_on_the_special_values():
    u = np.array([s[0] for s in R.BF16_SPECIALS], np.uint32)
    codes = R.bf16_ref(u.view(np.float32))
    for (bits_in, want), code in zip(R.BF16_SPECIALS, codes):
        if want is None:
            assert R.bf16_is_nan(code) and (int(code) >> 15) == (bits_in >> 31), hex(bits_in)
        else:
            assert int(code) == want, hex(bits_in)
