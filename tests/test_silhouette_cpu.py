"""What of the silhouette query needs no GPU: the float64 reference of tests/silhouette_ref.py against scikit-learn, the scratch
plan's byte counts and refusals, read_silhouette on a written file, the refusals that are made before the library is reached,
and the ABI tables."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from tests import silhouette_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("dim", [1, 5, 16, 41, 128, 256])
def test_reference_matches_sklearn(dim):
    SK = pytest.importorskip("sklearn.metrics")
    n = 1000
    for k in (2, 7, 64, 65, 200, 256):
        x, lab = R.blobs(n, dim, k, 1000 * dim + k)
        if k >= 200:
            lab[lab == 3] = 4                                     # an empty label
            lab[11] = 3                                           # and a singleton
        sums, sizes = R.sums64(x, lab, k)
        w = R.widths(sums, lab, sizes)
        assert w["defined"] and np.array_equal(sizes, np.bincount(lab, minlength=k))
        want = SK.silhouette_samples(x.astype(np.float64), lab, metric="euclidean")
        assert np.abs(w["s"] - want).max() <= 1e-12, (dim, k, float(np.abs(w["s"] - want).max()))
        assert abs(w["s"].mean() - SK.silhouette_score(x.astype(np.float64), lab, metric="euclidean")) <= 1e-12
        assert np.all(w["s"][sizes[lab] == 1] == 0)
        # a row list with repeats and ids outside the table, labels outside [0, k): the points alone, as scikit-learn sees them
        rows = np.random.default_rng(k).integers(-1, n + 1, 300)
        l2 = np.random.default_rng(k + 1).integers(-1, k + 1, 300).astype(np.int32)
        lp, sz = R.points_of(l2, k, n, rows)
        pts = lp >= 0
        if np.unique(lp[pts]).size >= 2:
            s2, z2 = R.sums64(x, l2, k, rows=rows)
            w2 = R.widths(s2, l2, z2, (rows >= 0) & (rows < n))
            assert np.array_equal(z2, sz) and np.all(np.isnan(w2["s"][~pts])) and np.all(w2["neighbor"][~pts] == -1) and np.all(s2[~pts] == 0)
            want2 = SK.silhouette_samples(x[rows[pts]].astype(np.float64), lp[pts], metric="euclidean")
            assert np.abs(w2["s"][pts] - want2).max() <= 1e-7      # a repeated row: sqrt of the float64 rounding of a zero d^2


def test_reference_edge_cases():
    x, lab = R.blobs(50, 3, 4, 1)
    one = np.zeros(50, np.int32)
    sums, sizes = R.sums64(x, one, 4)
    w = R.widths(sums, one, sizes)
    assert not w["defined"] and np.all(w["s"] == 0) and np.all(w["b"] == 0) and np.all(w["neighbor"] == -1) and np.all(w["a"] > 0)
    same = np.ones((6, 2), np.float32)                            # every distance 0: max(a, b) = 0
    l = np.array([0, 0, 0, 1, 1, 1], np.int32)
    sums, sizes = R.sums64(same, l, 2)
    w = R.widths(sums, l, sizes)
    assert w["defined"] and np.all(w["s"] == 0) and np.array_equal(w["neighbor"], 1 - l)
    # equal means: the lowest label
    pts = np.array([[0.0], [1.0], [-1.0], [5.0]], np.float32)
    l = np.array([0, 2, 1, 0], np.int32)
    sums, sizes = R.sums64(pts, l, 3)
    assert R.widths(sums, l, sizes)["neighbor"][0] == 1
    # the exact variant: integer tables give integers under the root, the f32 root is the float64 one rounded
    t = np.random.default_rng(2).integers(-3, 4, (40, 7)).astype(np.float32)
    l = np.random.default_rng(3).integers(-1, 5, 40).astype(np.int32)
    exact, _ = R.sums64(t, l, 5, f32_sqrt=True)
    plain, _, E = R.sums64(t, l, 5, bounds=True)
    assert np.all(np.abs(exact - plain) <= E) and np.all(exact[l < 0] == 0)


def up256(b):
    return (b + 255) // 256 * 256


@pytest.mark.parametrize("n,k,dim", [(0, 1, 1), (1000, 7, 5), (1000, 256, 256), (232965, 41, 128), (5000, 2, 16), (1025, 64, 17)])
def test_plan_byte_counts(n, k, dim):
    """{histograms [chunks of 1024 x k] | two start tables [k + 1] | the member list [n] | chunk sums} each rounded up to 256
    bytes, then the (segment, position) partials: n // 512 + k segments at most, by every position rounded up to 64 (at least
    64), or by 64 positions at the least"""
    from cuda_gcn_amd import _lib
    lib = _lib.gcnhip()
    a, b = C.c_size_t(), C.c_size_t()
    assert lib.gcnhip_silhouette_plan(n, k, dim, C.byref(a), C.byref(b)) == 0
    chunks = max(-(-n // 1024), 1)
    fixed = up256(chunks * k * 4) + up256(2 * (k + 1) * 4) + up256(max(n, 1) * 4) + up256(chunks * 8)
    segs = n // 512 + k
    assert a.value == fixed + 8 * segs * max(-(-n // 64), 1) * 64
    assert b.value == fixed + 8 * segs * 64
    assert a.value >= b.value
    assert lib.gcnhip_silhouette_plan(n, k, dim, None, None) == 0
    for bad in ((-1, 4, 4), (10, 0, 4), (10, 257, 4), (10, 4, 0), (10, 4, 257)):
        assert lib.gcnhip_silhouette_plan(*bad, C.byref(a), C.byref(b)) == -1
        assert b"gcnhip_silhouette_plan" in lib.gcnhip_last_error()


def test_read_silhouette(tmp_path):
    from cuda_gcn_amd.model import read_silhouette, GcnHostError
    rng = np.random.default_rng(5)
    n = 37
    s = rng.uniform(-1, 1, n)
    s[4] = np.nan
    cl, nb = rng.integers(0, 5, n), rng.integers(-1, 5, n)
    cl[4] = -1
    p = tmp_path / "s.txt"
    p.write_text("".join("%d %d %.9g %d\n" % (i, cl[i], s[i], nb[i]) for i in range(n)))
    got = read_silhouette(str(p))
    assert np.array_equal(got["node"], np.arange(n)) and np.array_equal(got["cluster"], cl) and np.array_equal(got["neighbor"], nb)
    assert got["s"].dtype == np.float64 and np.isnan(got["s"][4])
    keep = ~np.isnan(s)
    assert np.all(np.abs(got["s"][keep] - s[keep]) <= 1e-9)
    assert got["node"].dtype == got["cluster"].dtype == got["neighbor"].dtype == np.int32
    empty = tmp_path / "e.txt"
    empty.write_text("")
    assert read_silhouette(str(empty))["s"].size == 0
    for bad in ("0 1 0.5\n", "0 1 x 2\n", "0 1 0.5 2 9\n"):
        p.write_text("0 0 0.25 1\n" + bad)
        with pytest.raises(GcnHostError, match=r"read_silhouette: .*:2: expected `node cluster s neighbor`"):
            read_silhouette(str(p))


def bare_model(num_nodes=10, hidden=16):
    from cuda_gcn_amd.model import HipGCNModel
    m = HipGCNModel.__new__(HipGCNModel)
    m.params = types.SimpleNamespace(num_nodes=num_nodes, output_dim=4, hidden_dim=hidden)
    m.multilabel = False
    m.lib = None                                                  # any call into the library would fail loudly
    m.h = None
    return m


def test_refusals_that_need_no_gpu():
    from cuda_gcn_amd import _lib
    from cuda_gcn_amd.model import GcnHostError
    m = bare_model()
    lab = np.zeros(10, np.int32)
    for k in (0, 257, "ten", 2.5, True):
        with pytest.raises(GcnHostError, match=r"silhouette: k must be an integer in 1\.\.256"):
            m.silhouette(lab, k=k)
    with pytest.raises(GcnHostError, match=r"silhouette: k must be an integer in 1\.\.256"):
        m.silhouette(np.full(10, 300))                            # k = labels.max() + 1
    with pytest.raises(GcnHostError, match="silhouette: the query lists 10 rows, the labels are 9"):
        m.silhouette(lab[:9], k=2)
    with pytest.raises(GcnHostError, match="silhouette: the query lists 3 rows, the labels are 10"):
        m.silhouette(lab, k=2, nodes=[1, 2, 3])
    for bad in (np.zeros(10), np.zeros((5, 2), np.int32), "labels"):
        with pytest.raises(GcnHostError, match="silhouette: labels must be a one-dimensional integer array"):
            m.silhouette(bad, k=2)
    with pytest.raises(GcnHostError, match="silhouette: give a split or a node query"):
        m.silhouette(lab, k=2, split=1, nodes=[0])
    with pytest.raises(GcnHostError, match="silhouette: split is 1"):
        m.silhouette(lab, k=2, split=4)
    with pytest.raises(GcnHostError, match="silhouette: a hidden width of at most 256"):
        bare_model(hidden=512).silhouette(lab, k=2)
    host = _lib.gcnhost()
    assert host.gcnhost_model_silhouette(None, 0, None, 0, None, 2, 1, 0, 0, None, None, None, None, None, None, None, None) == -1
    assert b"gcnhost_model_silhouette: invalid argument" in host.gcnhost_last_error()


def test_abi_tables_hold_the_new_entry_points():
    from cuda_gcn_amd import _lib
    hip, host = _lib.gcnhip(), _lib.gcnhost()
    drv = open(os.path.join(ROOT, "include", "gcnhip_driver.h")).read()
    hst = open(os.path.join(ROOT, "include", "gcnhost.h")).read()
    for n in ("gcnhip_silhouette_plan", "gcnhip_silhouette_sums", "gcnhip_silhouette_rows"):
        assert n in _lib.GCNHIP_SYMBOLS and hasattr(hip, n) and re.search(rf"\bint {n}\(", drv), n
    assert "gcnhost_model_silhouette" in _lib.GCNHOST_SYMBOLS and hasattr(host, "gcnhost_model_silhouette")
    assert re.search(r"\bint gcnhost_model_silhouette\(", hst)
