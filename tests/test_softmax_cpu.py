"""tests/softmax_ref.py without a GPU: the hard-logit table has the properties its docstring promises, an f32 restatement of the
kernel statements (left-to-right sum, with subnormal results kept and flushed) stays inside the reference's bounds — so the
reference alone is inside its own bounds — and the exact outputs (correct, pred) on the tie rows are what they must be."""
import numpy as np
import pytest

from tests import softmax_ref as R

CLASSES = [1, 2, 3, 5, 7, 41, 64, 65, 129, 256]


@pytest.mark.parametrize("C", CLASSES)
def test_hard_rows_properties(C):
    z, t = R.hard_rows(C)
    kinds = R.hard_kinds(C)
    assert z.dtype == np.float32 and t.dtype == np.int32 and z.shape == (len(kinds), C) and t.shape == (len(kinds),)
    assert np.all(np.isfinite(z)) and z.min() >= np.float32(-9e29) and z.max() <= np.float32(1e30)
    assert not np.any(np.signbit(z) & (z == 0)), "-0.0 in the table"
    assert np.all((t >= 0) & (t < C))
    z2, t2 = R.hard_rows(C)
    assert np.array_equal(z.view(np.uint32), z2.view(np.uint32)) and np.array_equal(t, t2)      # the same table every time
    count = {k: kinds.count(k) for k in set(kinds)}
    assert count["control"] == 8 and count["wide"] == 2 * len(R.WIDE_A) and count["constant"] == len(R.CONSTANTS)
    assert count["underflow"] == 2 * len(R.UNDERFLOW_D)
    if C >= 5:
        assert count["tie"] == 6
    if C >= 2:
        # truth on and off the maximum in the wide and underflow rows; the widest row reaches both ends of the range
        for kind in ("wide", "underflow"):
            idx = [i for i, k in enumerate(kinds) if k == kind]
            on = [int(np.argmax(z[i]) == t[i]) for i in idx]
            assert on == [1, 0] * (len(idx) // 2), kind
        assert z.max() == np.float32(1e30) and z.min() == np.float32(-9e29)
        # the gaps bracket expf's limits: one row underflows to a subnormal, one to zero, one stays normal
        gaps = sorted({float(np.round((z[i].max() - np.delete(z[i], np.argmax(z[i])).mean()))) for i, k in enumerate(kinds) if k == "underflow"})
        assert gaps[0] == 17 and gaps[-1] == 120 and any(87 <= g <= 88 for g in gaps) and any(103 <= g <= 104 for g in gaps)


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("flush", [False, True])
def test_f32_restatement_is_inside_the_bounds(C, flush):
    z, t = R.hard_rows(C)
    ref = R.reference(z, t)
    assert np.all(np.isfinite(ref["term"])) and np.all(np.isfinite(ref["grad"]))
    assert np.all(np.isfinite(ref["E_term"])) and np.all(np.isfinite(ref["E_grad"])) and np.all(ref["E_grad"] > 0)
    term, g = R.restate_f32(z, t, ref["count"], flush)
    wt, wg = R.worst(term, ref["term"], ref["E_term"]), R.worst(g, ref["grad"], ref["E_grad"])
    print(f"C {C} flush {flush}: worst term {wt:.3f}, worst gradient {wg:.3f} of the bound")
    assert wt < 1.0 and wg < 1.0
    # the bound is not vacuous where the logits are tame: a term that is 1e-4 off is caught
    tame = R.tame_rows(z)
    assert np.all(ref["E_term"][tame] < 1e-4) and np.all(ref["E_grad"][tame] < 1e-5)


@pytest.mark.parametrize("C", CLASSES)
def test_f32_restatement_with_the_gradient_factors(C):
    """a class weight and a row factor: each is one more rounded product, which the bound counts (softmax_ref, g_j)"""
    z, t = R.hard_rows(C)
    rng = np.random.default_rng(C)
    weight = (0.25 + 3.75 * rng.random(C)).astype(np.float32)
    scale = (rng.random(z.shape[0]) + 0.5).astype(np.float32)
    for w, s in ((weight, None), (None, scale), (weight, scale)):
        ref = R.reference(z, t, row_scale=s, weight=w)
        term, g = R.restate_f32(z, t, ref["count"], row_scale=s, weight=w)
        wt, wg = R.worst(term, ref["term"], ref["E_term"]), R.worst(g, ref["grad"], ref["E_grad"])
        print(f"C {C} weight {w is not None} scale {s is not None}: worst term {wt:.3f}, worst gradient {wg:.3f} of the bound")
        assert wt < 1.0 and wg < 1.0


@pytest.mark.parametrize("C", [2, 5, 7, 41, 64, 256])
def test_exact_counts_on_ties_and_constant_rows(C):
    z, t = R.hard_rows(C)
    kinds = np.array(R.hard_kinds(C))
    ref = R.reference(z, t)
    tie, const = kinds == "tie", kinds == "constant"
    assert np.all(ref["correct"][tie]) and np.all(ref["correct"][const])          # nothing is strictly above the label's logit
    assert np.all(ref["pred"][const] == 0)                                        # every class ties: the lowest wins
    if C >= 5:
        assert ref["pred"][tie].tolist() == [0, 0, 3, 3, C // 2, C // 2]           # the lower column of each pair
        assert t[tie].tolist() == [0, C - 1, 3, 4, C // 2, C - 1]
    wide = np.flatnonzero(kinds == "wide")
    assert ref["correct"][wide].tolist() == [True, False] * (wide.size // 2)
    # a row that is not scored counts nowhere
    t2 = t.copy()
    t2[tie] = -1
    ref2 = R.reference(z, t2, count=ref["count"])
    assert int(ref2["correct"].sum()) == int(ref["correct"].sum()) - int(tie.sum())
    assert np.all(ref2["grad"][tie] == 0) and np.all(ref2["term"][tie] == 0)
    assert np.array_equal(ref2["grad"][~tie], ref["grad"][~tie])


def test_scaled_row_is_calib_refs():
    from tests import calib_ref
    z, t = R.hard_rows(7)
    ref = R.reference(z, t, beta=0.5)
    o, e_o, prob, _ = calib_ref.scale(ref["logp"], 0.5)
    assert np.array_equal(ref["scaled"], o) and np.all(ref["E_scaled"] >= e_o) and np.array_equal(ref["sprob"], prob)
    assert "scaled" not in R.reference(z, t)
