"""HDBSCAN without a GPU: tests/hdbscan_ref.py AND model.hdbscan_tree against scikit-learn and scipy, a hand-sized answer, the reader, refusals"""
import numpy as np
import pytest

from cuda_gcn_amd import model as M
from tests import dbscan_ref as D
from tests import hdbscan_ref as R
from tests.silhouette_ref import blobs


@pytest.mark.parametrize("n,dim,k,mcs,ms,method,single", [(300, 4, 5, 5, 2, "eom", False), (257, 3, 3, 10, 2, "leaf", False),
                                                          (120, 2, 1, 8, 1, "eom", True), (400, 8, 6, 15, 2, "eom", False)])
def test_scikit_learns_answer(n, dim, k, mcs, ms, method, single):
    """float blobs whose tree weights are distinct (asserted; a larger min_samples repeats core distances in the tree): the same labels
    with the same numbering, probabilities to 1e-12, and the DBSCAN* labels at three radii of the tree"""
    cluster = pytest.importorskip("sklearn.cluster")
    x = blobs(n, dim, k, n)[0].astype(np.float64)
    d2 = D.dist2(x, np.ones(n, bool))
    want = cluster.HDBSCAN(min_cluster_size=mcs, min_samples=ms, algorithm="brute", cluster_selection_method=method, allow_single_cluster=single,
                           copy=True).fit(x)
    ref = R.run(d2, mcs, ms, method=method, allow_single_cluster=single)
    assert np.unique(ref["w"]).size == n - 1
    got = M.hdbscan_tree(ref["lo"], ref["hi"], ref["w"], n, mcs, method, single)
    for a in (ref, got):
        assert np.array_equal(a["labels"], want.labels_) and np.abs(a["probabilities"] - want.probabilities_).max() <= 1e-12
    assert np.array_equal(got["linkage"][:, [0, 1, 3]], ref["linkage"][:, [0, 1, 3]]) and got["n_clusters"] == want.labels_.max() + 1
    for q in (0.2, 0.5, 0.8):
        cut = float(np.sqrt(np.quantile(ref["w"], q)))
        assert np.array_equal(M.hdbscan_cut(got, cut, mcs), want.dbscan_clustering(cut, mcs)), q


def test_linkage_is_scipys_single_linkage():
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    x = blobs(200, 3, 4, 7)[0].astype(np.float64)
    ref = R.run(D.dist2(x, np.ones(200, bool)), 5, 1)
    got = M.hdbscan_tree(ref["lo"], ref["hi"], ref["w"], 200, 5)
    want = hierarchy.linkage(x, method="single")
    for z in (ref["linkage"], got["linkage"]):
        assert np.array_equal(z[:, [0, 1, 3]], want[:, [0, 1, 3]]) and np.abs(z[:, 2] - want[:, 2]).max() <= 1e-6 * want[:, 2].max()


def test_a_hand_sized_answer():
    """two groups of five on a line, steps of 1 inside and a gap of 10 between, plus a point 100 away; position 3 is no point"""
    x = np.array([0, 1, 2, -1, 3, 4, 14, 15, 16, 17, 18, 118], np.float64)[:, None]
    ok = np.arange(12) != 3
    ref = R.run(D.dist2(x, ok), 4, 1)
    assert np.array_equal(ref["lo"][-2:], [5, 10]) and np.array_equal(ref["hi"][-2:], [6, 11]) and np.array_equal(ref["w"][-2:], [100.0, 10000.0])
    got = M.hdbscan_tree(ref["lo"], ref["hi"], ref["w"], 12, 4)
    for a in (ref, got):
        assert a["labels"].tolist() == [0, 0, 0, -1, 0, 0, 1, 1, 1, 1, 1, -1] and np.array_equal(a["probabilities"], a["labels"] >= 0)
    assert (got["n_clusters"], got["n_noise"], got["points"]) == (2, 1, 11) and got["linkage"][-1].tolist() == [10.0, 19.0, 100.0, 11.0]
    assert M.hdbscan_cut(got, 10.5, 4).tolist() == [0] * 3 + [-1] + [0] * 7 + [-1] and M.hdbscan_cut(got, 5.0, 6).max() == -1


def test_read_hdbscan_and_refusals(tmp_path):
    p = tmp_path / "h.txt"
    p.write_text("4 0 1\n7 -1 0\n\n9 1 0.25\n")
    got = M.read_hdbscan(str(p))
    assert got["node"].tolist() == [4, 7, 9] and got["label"].tolist() == [0, -1, 1] and got["probability"].tolist() == [1.0, 0.0, 0.25]
    for bad in ("4 0\n", "4 -2 0.5\n", "4 0 1.5\n", "x 0 1\n"):
        p.write_text(bad)
        with pytest.raises(M.GcnHostError, match="h.txt:1: expected `node label probability`"):
            M.read_hdbscan(str(p))
    lo, hi, w = [0, 1], [1, 2], [1.0, 2.0]
    for args, msg in (((lo, hi, w, 3, 1), "min_cluster_size must be at least 2"), ((lo, hi, [2.0, 1.0], 3), "non-negative and ascending"),
                      ((lo, [1, 3], w, 3), "an end outside the list"), (([0, 0], [1, 1], w, 3), "do not form one tree"),
                      (([0, 2], [1, 3], w, 4), "do not form one tree"), ((lo, hi, w[:1], 3), "of one length")):
        with pytest.raises(M.GcnHostError, match="hdbscan_tree: .*" + msg):
            M.hdbscan_tree(*args)
    with pytest.raises(M.GcnHostError, match="'eom' or 'leaf'"):
        M.hdbscan_tree(lo, hi, w, 3, cluster_selection_method="best")
