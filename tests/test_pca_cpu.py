"""The host side of the PCA query, without a GPU: the symmetric eigen solver (model.sym_eigen) against the two conditions
DESIGN §4.21 states for it and against numpy.linalg.eigh, what a fit derives from a scatter matrix (model.pca_from_scatter) against the formulas of
tests/pca_ref.py and, where it imports, scikit-learn, and the scratch plan."""
import ctypes as C

import numpy as np
import pytest

from tests import pca_ref as R

HS = [1, 2, 5, 41, 128, 256]


@pytest.fixture(scope="module")
def M():
    from cuda_gcn_amd import model
    return model


@pytest.mark.parametrize("h", HS)
def test_sym_eigen_meets_both_conditions(M, h):
    """residual ratio max_j |S v_j - lambda_j v_j|_2 / (h 2^-52 |S|_F) <= 8 and orthogonality ratio max |V^T V - I| / (h 2^-52) <= 8
    (conditions, not measurements); eigenvalues descending, the sign rule, and agreement with numpy's eigenvalues within the sum of
    the two solvers' residual norms |S V - V L|_F (Weyl: a pair (L, V) with orthonormal V is the exact eigensystem of S - R V^T,
    and |R V^T|_2 <= |R|_F)."""
    for name, s in R.solver_matrices(h).items():
        lam, v = M.sym_eigen(s)
        w, u = R.eigh_desc(s)
        mine, theirs = (R.residual_ratio(s, lam, v), R.orthogonality_ratio(v)), (R.residual_ratio(s, w, u), R.orthogonality_ratio(u))
        print(f"h={h} {name}: sym_eigen residual {mine[0]:.3g} orthogonality {mine[1]:.3g}; eigh residual {theirs[0]:.3g} orthogonality {theirs[1]:.3g}")
        assert np.all(np.isfinite(lam)) and np.all(np.isfinite(v)), name
        assert mine[0] <= 8, (name, mine)
        assert mine[1] <= 8, (name, mine)
        assert np.all(np.diff(lam) <= 0), name
        assert R.sign_rule(v), name
        bound = np.linalg.norm(s @ v - v * lam) + np.linalg.norm(s @ u - u * w)
        print(f"h={h} {name}: max eigenvalue difference {np.abs(lam - w).max():.3g}, the two residual norms {bound:.3g}")
        assert np.abs(lam - w).max() <= bound, (name, np.abs(lam - w).max(), bound)


def test_sym_eigen_known_answers(M):
    lam, v = M.sym_eigen(np.diag([1.0, 5.0, -2.0]))
    assert np.array_equal(lam, [5.0, 1.0, -2.0]) and np.array_equal(v, np.eye(3)[:, [1, 0, 2]])
    lam, v = M.sym_eigen(np.array([[2.0, 1.0], [1.0, 2.0]]))
    assert np.allclose(lam, [3.0, 1.0], rtol=0, atol=4 * R.EPS) and v[0, 0] > 0 and v[0, 1] > 0    # equal magnitudes: the lowest index is positive
    lam, v = M.sym_eigen(np.zeros((4, 4)))
    assert np.array_equal(lam, np.zeros(4)) and np.array_equal(v, np.eye(4))
    lam, v = M.sym_eigen(np.array([[-3.0]]))
    assert lam[0] == -3.0 and v[0, 0] == 1.0


def test_sym_eigen_refusals(M):
    bad = np.eye(3)
    bad[1, 2] = np.nan
    bad[2, 1] = np.nan
    with pytest.raises(M.GcnHostError, match=r"sym_eigen: entry \(1, 2\) is not finite"):
        M.sym_eigen(bad)
    asym = np.eye(3)
    asym[0, 2] = 1e-300
    with pytest.raises(M.GcnHostError, match=r"sym_eigen: the matrix is not symmetric at \(0, 2\)"):
        M.sym_eigen(asym)
    with pytest.raises(M.GcnHostError, match=r"sym_eigen: the width must be in 1\.\.256, got 0"):
        M.sym_eigen(np.zeros((0, 0)))
    with pytest.raises(M.GcnHostError, match=r"sym_eigen: the width must be in 1\.\.256, got 257"):
        M.sym_eigen(np.eye(257))
    with pytest.raises(M.GcnHostError, match="sym_eigen: a square matrix"):
        M.sym_eigen(np.zeros((2, 3)))


@pytest.mark.parametrize("h", [1, 5, 41, 128])
def test_pca_from_scatter_follows_the_formulas(M, h):
    rows = 1000
    for name in ("planted", "rank1", "zero", "indefinite", "planted_1e-30", "planted_1e+30"):
        s = R.solver_matrices(h)[name]
        k = max(1, h // 2)
        got = M.pca_from_scatter(s, np.zeros(h), rows, k=k, whiten=True)
        lam, v = M.sym_eigen(s)
        want = R.from_scatter_ref(lam, rows, k, whiten=True)
        for key in ("eigenvalues", "explained_variance", "explained_variance_ratio", "singular_values", "scale"):
            assert np.all(np.isfinite(got[key])), (name, key)
            assert np.all(np.abs(got[key] - want[key]) <= 1e-12 * np.abs(want[key])), (name, key)
        assert got["rank"] == want["rank"] and got["rows"] == rows
        assert np.array_equal(got["components"], v.T[:k])
        assert np.all(got["eigenvalues"] >= 0) and np.all(got["scale"][got["rank"]:] == 0)
        if name == "zero":
            assert got["rank"] == 0 and np.all(got["explained_variance_ratio"] == 0) and np.all(got["scale"] == 0)
        if name == "rank1":
            assert got["rank"] == 1
        if name == "planted":
            assert got["rank"] == h and abs(got["explained_variance_ratio"].sum() - 1) <= h * R.EPS
    assert M.pca_from_scatter(np.eye(3), None, 2)["scale"] is None
    for kw, msg in ((dict(rows=1), "at least 2 rows"), (dict(rows=5, k=0), r"k must be in 1\.\.3"), (dict(rows=5, k=4), r"k must be in 1\.\.3")):
        with pytest.raises(M.GcnHostError, match="pca_from_scatter: " + msg):
            M.pca_from_scatter(np.eye(3), np.zeros(3), **kw)
    with pytest.raises(M.GcnHostError, match="pca_from_scatter: the mean is not finite"):
        M.pca_from_scatter(np.eye(3), np.array([0, np.inf, 0]), 5)
    with pytest.raises(M.GcnHostError, match="pca_from_scatter: sym_eigen: the matrix is not symmetric"):
        M.pca_from_scatter(np.array([[1.0, 2.0], [3.0, 1.0]]), None, 5)


@pytest.mark.parametrize("h", [5, 41, 256])
def test_pca_from_scatter_against_scikit_learn(M, h):
    """PCA(svd_solver="full") on the float64 data the scatter matrix was formed from.  Both solvers' pairs are held against the
    same S: E = |S V - V L|_F of sym_eigen + |S U - U W|_F of scikit-learn's k pairs (W = explained_variance_ . (n - 1)).
    Eigenvalues agree within E (Weyl), a component, up to the stated sign, within the angle E / gap, and it is compared only where
    the eigengap is above 8e-4 lambda_1.  The ratios divide by the total variance, which either side forms as a float64 sum of
    h column sums of n terms: |ratio - ratio'| <= E / trace(S) + 2 (n + h) 2^-53 ratio."""
    decomposition = pytest.importorskip("sklearn.decomposition")
    n = 1000
    x = R.planted(n, h, 7 + h).astype(np.float64)
    c = x - x.mean(0)
    s = c.T @ c
    s = (s + s.T) / 2
    k = min(h, 8)
    got = M.pca_from_scatter(s, x.mean(0), n, k=k)
    sk = decomposition.PCA(n_components=k, svd_solver="full").fit(x)
    lam, v = M.sym_eigen(s)
    w, u = sk.explained_variance_ * (n - 1), sk.components_.T
    E = np.linalg.norm(s @ v - v * lam) + np.linalg.norm(s @ u - u * w)
    print(f"h={h}: the two residual norms {E:.3g}; eigenvalue difference {np.abs(got['eigenvalues'][:k] - w).max():.3g}")
    assert np.abs(got["eigenvalues"][:k] - w).max() <= E
    assert np.abs(got["explained_variance"][:k] - sk.explained_variance_).max() <= E / (n - 1)
    ratio_tol = E / np.trace(s) + 2 * (n + h) * R.U * sk.explained_variance_ratio_
    assert np.all(np.abs(got["explained_variance_ratio"][:k] - sk.explained_variance_ratio_) <= ratio_tol)
    assert np.abs(got["singular_values"][:k] ** 2 - sk.singular_values_ ** 2).max() <= E
    d = np.r_[np.inf, np.abs(np.diff(lam)), np.inf]              # the distance of eigenvalue j to its neighbours on both sides
    gaps = np.minimum(d[:-1], d[1:])
    checked = 0
    for j in range(k):
        if gaps[j] > 8e-4 * lam[0]:
            theirs = sk.components_[j] * np.sign(sk.components_[j][np.argmax(np.abs(sk.components_[j]))])
            angle = np.linalg.norm(got["components"][j] - theirs)
            print(f"h={h} component {j}: angle {angle:.3g}, allowed {E / gaps[j]:.3g}")
            assert angle <= E / gaps[j], j
            checked += 1
    assert checked >= min(k, 5)


def test_pca_plan_follows_the_documented_formula():
    from cuda_gcn_amd import _lib
    lib = _lib.gcnhip()
    for dim in (1, 5, 16, 17, 41, 128, 256):
        t = -(-dim // 16)
        per = t * (t + 1) // 2 * 256 * 8
        for n in (0, 1, R.PART - 1, R.PART, R.PART + 1, 2 * R.PART + 3, 232965):
            a, b = C.c_size_t(), C.c_size_t()
            assert lib.gcnhip_pca_plan(n, dim, C.byref(a), C.byref(b)) == 0
            assert a.value == max(-(-n // R.PART), 1) * per and b.value == per, (n, dim)
    for n, dim in ((-1, 4), (4, 0), (4, 257)):
        assert lib.gcnhip_pca_plan(n, dim, None, None) == -1 and b"gcnhip_pca_plan" in lib.gcnhip_last_error()
