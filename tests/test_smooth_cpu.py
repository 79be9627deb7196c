"""The float64 reference of label propagation and Correct & Smooth (tests/smooth_ref.py) against hand-worked cases, and the
argument checks of HipGCNModel.propagate / label_propagation / correct_and_smooth that need no GPU."""
import types

import numpy as np
import pytest

from tests import smooth_ref as R


def two_triangles():
    """nodes 0-1-2 and 3-4-5 are triangles, joined by the edge 2-3; self loops included.  Degrees 3 3 4 4 3 3."""
    nbr = {0: [0, 1, 2], 1: [0, 1, 2], 2: [0, 1, 2, 3], 3: [2, 3, 4, 5], 4: [3, 4, 5], 5: [3, 4, 5]}
    indptr = np.cumsum([0] + [len(nbr[i]) for i in range(6)]).astype(np.int32)
    indices = np.concatenate([nbr[i] for i in range(6)]).astype(np.int32)
    return indptr, indices, R.edge_coef(indptr, indices)


def test_edge_coefficients_by_hand():
    indptr, indices, coef = two_triangles()
    assert coef.dtype == np.float32
    dense = np.zeros((6, 6))
    for r in range(6):
        dense[r, indices[indptr[r]:indptr[r + 1]]] = coef[indptr[r]:indptr[r + 1]]
    assert np.allclose(dense, dense.T)
    assert abs(dense[0, 0] - 1 / 3) < 1e-7 and abs(dense[2, 3] - 0.25) < 1e-7 and abs(dense[1, 2] - 1 / np.sqrt(12)) < 1e-7
    assert dense[0, 3] == 0


def test_one_step_on_two_triangles_by_hand():
    """one labelled node per triangle: Y_1 = alpha A^ Y_0 + (1 - alpha) Y_0 worked out entry by entry"""
    csr = two_triangles()
    truth = np.array([0, -1, -1, -1, -1, 1])
    a = 0.9
    y1, b1 = R.propagate(csr, R.onehot_rows(truth, 2), a, 1, 0.0, 1.0)
    want = np.zeros((6, 2))
    want[0, 0] = a / 3 + (1 - a)
    want[1, 0] = a / 3
    want[2, 0] = a / np.sqrt(12)
    want[:, 1] = want[::-1, 0]
    assert np.allclose(y1, want, rtol=0, atol=1e-7)
    # the bound of one step from exact inputs: 8 eps (alpha |A^| |Y_0| + (1 - alpha) |Y_0|) — here every term is >= 0
    assert np.allclose(b1, 8 * R.EPS * want, rtol=1e-6, atol=0)
    one, bound = R.blend_step(csr, R.onehot_rows(truth, 2), R.onehot_rows(truth, 2), a, 1 - a, 0.0, 1.0)
    assert np.array_equal(one, y1) and np.allclose(bound, b1, rtol=1e-12, atol=0)


def test_label_propagation_splits_the_two_triangles():
    csr = two_triangles()
    pred, y, b = R.label_propagation(csr, np.array([0, -1, -1, -1, -1, 1]), 2, alpha=0.9, iters=50)
    assert pred.tolist() == [0, 0, 0, 1, 1, 1]
    assert np.all((y >= 0) & (y <= 1)) and np.allclose(y[:, 0], y[::-1, 1])
    assert b.max() < 1e-5 and np.all(R.clear_rows(y, b))
    # the recurrence equals K single steps
    z = R.onehot_rows(np.array([0, -1, -1, -1, -1, 1]), 2)
    y0 = z
    for _ in range(50):
        z, _ = R.blend_step(csr, z, y0, 0.9, 1 - 0.9, 0.0, 1.0)
    assert np.array_equal(z, y)


def test_alpha_zero_returns_y0_and_iters_zero_too():
    csr = two_triangles()
    y0 = np.random.default_rng(0).standard_normal((6, 3))
    y, b = R.propagate(csr, y0, 0.0, 7)
    assert np.array_equal(y, y0) and np.allclose(b, 8 * R.EPS * np.abs(y0), rtol=1e-12, atol=0)      # nothing accumulates
    y, b = R.propagate(csr, y0, 0.7, 0)
    assert np.array_equal(y, y0) and not b.any()


def test_the_clamp_bites():
    csr = two_triangles()
    x = np.array([[2.0, 0.1, -3.0]] * 6)
    out, _ = R.blend_step(csr, x, x, 1.0, 1.0, -1.0, 1.0)
    free, _ = R.blend_step(csr, x, x, 1.0, 1.0)
    assert np.all(out[:, 0] == 1.0) and np.all(out[:, 2] == -1.0)
    assert np.array_equal(out[:, 1], free[:, 1]) and np.all(np.abs(free[:, 1]) < 1)
    assert np.all(free[:, 0] > 1) and np.all(free[:, 2] < -1)
    # the bound is that of the unclamped value: the clamp is 1-Lipschitz
    y, b = R.propagate(csr, x, 0.5, 3, -1.0, 1.0)
    assert np.all(np.abs(y) <= 1) and np.all(b > 0)


def test_error_rows_count_only_known_classes():
    logp = np.log(np.array([[0.5, 0.25, 0.25], [0.1, 0.8, 0.1], [0.2, 0.2, 0.6], [1 / 3, 1 / 3, 1 / 3]]))
    e, sigma = R.error_rows(logp, np.array([0, -1, 3, 2]))
    assert np.allclose(e[0], [0.5, -0.25, -0.25]) and not e[1].any() and not e[2].any()          # -1 and a class >= C: nothing
    assert np.allclose(e[3], [-1 / 3, -1 / 3, 2 / 3])
    assert sigma[1] == 2 and abs(sigma[0] - (1.0 + 4 / 3)) < 1e-12
    e2, sigma2 = R.error_rows(logp, np.array([0, -1, 3, 2]), rows=[0, 1])                      # listed rows only
    assert not e2[3].any() and sigma2 == (1.0, 1)


def test_autoscale_guard_and_correct_rows():
    """a row with sum |E^| = 0 gets s = 1, and so does a row whose s would exceed 1000; known rows are reset to their labels"""
    logp = np.log(np.full((4, 2), 0.5))
    e_hat = np.array([[0.0, 0.0], [1e-6, -1e-6], [0.1, -0.1], [0.3, 0.2]])
    sigma = (0.8, 2)                                              # sigma = 0.4
    s = R.autoscale(e_hat, sigma)
    assert s[0] == 1.0                                            # 0.4 / 0 = inf
    assert s[1] == 1.0                                            # 0.4 / 2e-6 = 2e5 > 1000
    assert abs(s[2] - 2.0) < 1e-12 and abs(s[3] - 0.8) < 1e-12
    assert R.autoscale(e_hat, (0.0, 0)).tolist() == [1.0] * 4     # no known row at all: 0 / 0
    g0 = R.correct_rows(logp, e_hat, np.array([-1, -1, -1, 1]), sigma)
    assert np.allclose(g0[0], [0.5, 0.5]) and np.allclose(g0[1], [0.5 + 1e-6, 0.5 - 1e-6]) and np.allclose(g0[2], [0.7, 0.3])
    assert g0[3].tolist() == [0.0, 1.0]


def test_correct_and_smooth_on_two_triangles():
    """a classifier that is unsure everywhere and WRONG on node 4; nodes 0 and 5 are known.  The residual of node 5 pulls node 4
    over, and the bounds stay far below the margins."""
    csr = two_triangles()
    p = np.array([[0.6, 0.4], [0.6, 0.4], [0.55, 0.45], [0.45, 0.55], [0.52, 0.48], [0.4, 0.6]])
    truth = np.array([0, -1, -1, -1, -1, 1])
    out = R.correct_and_smooth(csr, np.log(p), truth)
    assert np.argmax(p, axis=1).tolist() == [0, 0, 0, 1, 0, 1]
    assert out["pred"].tolist() == [0, 0, 0, 1, 1, 1]
    assert out["sigma"][1] == 2 and abs(out["sigma"][0] - 1.6) < 1e-12
    assert out["G0"][0].tolist() == [1.0, 0.0] and out["G0"][5].tolist() == [0.0, 1.0]
    assert not out["B_G0"][0].any() and np.all(out["B_G0"][1:5] >= R.EXP_ATOL)
    assert out["B_G"].max() < 1e-4 and np.all(R.clear_rows(out["G"], out["B_G"]))
    assert out["guard_margin"] > 0.5


# ---- argument checks of the model's methods: all raise before the library is touched ------------------------------------

def bare_model(num_nodes=10, classes=4, multilabel=False):
    from cuda_gcn_amd.model import HipGCNModel
    m = HipGCNModel.__new__(HipGCNModel)
    m.params = types.SimpleNamespace(num_nodes=num_nodes, output_dim=classes)
    m.multilabel = multilabel
    m.lib = None                                                  # any call into the library would fail loudly
    m.h = None
    return m


def test_model_argument_validation_needs_no_gpu():
    m = bare_model()
    y = np.zeros((10, 3), np.float32)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"alpha must be in \[0, 1\]"):
            m.propagate(y, bad, 3)
        with pytest.raises(ValueError, match=r"alpha must be in \[0, 1\]"):
            m.label_propagation(alpha=bad)
        with pytest.raises(ValueError, match=r"alpha_smooth must be in \[0, 1\]"):
            m.correct_and_smooth(alpha_smooth=bad)
    with pytest.raises(ValueError, match="iters must be an integer >= 0"):
        m.propagate(y, 0.5, -1)
    with pytest.raises(ValueError, match="iters must be an integer >= 0"):
        m.correct_and_smooth(iters_correct=-2)
    for shape in ((9, 3), (10, 65), (10, 0), (10,)):
        with pytest.raises(ValueError, match="y0 must be"):
            m.propagate(np.zeros(shape, np.float32), 0.5, 1)
    with pytest.raises(ValueError, match="lo <= hi"):
        m.propagate(y, 0.5, 1, clamp=(1.0, 0.0))
    for splits in ((), (0,), (4,), (1, 7)):
        with pytest.raises(ValueError, match="splits are 1"):
            m.label_propagation(splits=splits)
    with pytest.raises(ValueError, match="multi-label model"):
        bare_model(multilabel=True).correct_and_smooth()
    with pytest.raises(ValueError, match="multi-label model"):
        bare_model(multilabel=True).label_propagation()
    with pytest.raises(ValueError, match="at most 64 classes"):
        bare_model(classes=65).correct_and_smooth()
    assert m._smooth_args("x", [("alpha", 0.5, 3)], (1, 2, 2)) == 6 and m._smooth_args("x", [("alpha", 1, 0)], 3) == 8
