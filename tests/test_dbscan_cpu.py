"""The DBSCAN reference and the host-only pieces: dbscan_ref against hand answers and scikit-learn's brute-force DBSCAN, read_dbscan,
the refusals that need no GPU."""
import numpy as np
import pytest

from tests import dbscan_ref as R


def run(t, eps2, min_samples, rows=None):
    xs, ok = R.scaled_rows(t, rows)
    return R.dbscan(R.dist2(xs, ok), eps2, min_samples)


def test_reference_on_hand_answers():
    t = np.array([0, 1, 2, 3, 10, 20, 21, 22], np.float32)[:, None]
    r = run(t, 2.25, 3, rows=np.r_[np.arange(8), -1, 8, 4])      # two positions without a row, the row at 10 twice
    assert r["labels"].tolist() == [0, 0, 0, 0, -1, 1, 1, 1, -1, -1, -1] and r["counts"].tolist() == [2, 3, 3, 2, 2, 2, 3, 2, 0, 0, 2]
    assert r["core"].tolist() == [False, True, True, False, False, False, True, False, False, False, False]
    assert (r["n_clusters"], r["n_core"], r["n_border"], r["n_noise"], r["points"]) == (2, 3, 4, 2, 9) and r["sizes"].tolist() == [4, 3]
    b = run(np.array([0, 1, 2, 3, 4, 6, 8, 9, 10, 11, 12, 50], np.float32)[::-1, None].copy(), 4.5, 4)
    # reversed: the cluster of 8..11 holds the smaller positions and is number 0; the point at 6 has core neighbours in both
    assert b["labels"].tolist() == [-1, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1] and b["ambiguous"] == 1 and b["n_border"] == 3
    assert R.counts(R.dist2(*R.scaled_rows(t)), [0.5, 1.0, 64.0]).tolist() == [[1] * 8, [2, 3, 3, 2, 1, 2, 3, 2], [4, 4, 5, 5, 3, 3, 3, 3]]


@pytest.mark.parametrize("dim", [1, 41])
def test_reference_labels_are_scikit_learns(dim):
    cluster = pytest.importorskip("sklearn.cluster")
    for t, eps2, ms in ((R.bridges(dim), 4.5, 4), (R.intblobs(193, 16, 4, 193), 19.5, 5)):
        want = cluster.DBSCAN(eps=np.sqrt(eps2), min_samples=ms, algorithm="brute").fit(t.astype(np.float64))
        got = run(t, eps2, ms)
        assert np.array_equal(got["labels"], want.labels_) and np.array_equal(np.flatnonzero(got["core"]), want.core_sample_indices_)


def test_read_dbscan(tmp_path):
    from cuda_gcn_amd.model import GcnHostError, read_dbscan
    p = tmp_path / "d.txt"
    p.write_text("3 0 1 7\n\n9 -1 0 1\n")
    got = read_dbscan(str(p))
    assert got["node"].tolist() == [3, 9] and got["label"].tolist() == [0, -1] and got["core"].tolist() == [True, False]
    assert got["count"].tolist() == [7, 1]
    for bad in ("3 0 1\n", "3 0 2 7\n", "3 -2 0 7\n", "3 0 1 x\n"):
        p.write_text("1 0 1 5\n" + bad)
        with pytest.raises(GcnHostError, match=r"read_dbscan: .*:2: expected `node label core count`"):
            read_dbscan(str(p))


def test_refusals_that_need_no_gpu():
    """the argument checks of HipGCNModel.dbscan / neighbor_counts come before any library call"""
    from cuda_gcn_amd.model import GcnHostError, HipGCNModel
    m = object.__new__(HipGCNModel)                               # no model behind it: a check that reached the library would fail
    for kwargs, msg in ((dict(eps=0.0), "eps must be finite"), (dict(eps=np.inf), "eps must be finite"), (dict(eps=-1.0), "eps must be finite"),
                        (dict(eps=1.0, min_samples=0), "min_samples must be at least 1"), (dict(eps=1.0, min_samples=2.5), "min_samples")):
        with pytest.raises(GcnHostError, match="dbscan: " + msg):
            m.dbscan(**kwargs)
    for e, msg in (([], "between 1 and 8 radii"), ([1.0] * 9, "between 1 and 8 radii"), ([1.0, 0.0], "eps must be finite"), ([np.nan], "eps must be")):
        with pytest.raises(GcnHostError, match="neighbor_counts: " + msg):
            m.neighbor_counts(e)
    with pytest.raises(GcnHostError, match="dbscan: data must be a float"):
        m.dbscan(1.0, data=np.zeros((4, 300)))
    with pytest.raises(GcnHostError, match="dbscan: with data the rows are the data's"):
        m.dbscan(1.0, data=np.zeros((4, 3)), split=3)
