"""The map-quality reference and the host-only pieces: mapq_ref against scikit-learn's trustworthiness, map_quality_metrics on hand
tables, the plan, the refusals that need no GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import mapq_ref as R
from tests.silhouette_ref import blobs


@pytest.mark.parametrize("n,dim", [(193, 2), (300, 16), (193, 41), (1024, 128)])
def test_reference_trustworthiness_is_scikit_learns(n, dim):
    """tie-free float rows, the map = the first two columns plus noise: the rank definition is scikit-learn's"""
    manifold = pytest.importorskip("sklearn.manifold")
    x = blobs(n, dim, 4, n)[0]
    y = (x[:, :2] + 0.3 * np.random.default_rng(dim).standard_normal((n, 2))).astype(np.float32)
    ok = np.ones(n, bool)
    dx, dy = R.candidates(x, ok), R.candidates(y, ok)
    for k in (1, 5, 32):
        kx, ky = R.knn(dx, k), R.knn(dy, k)
        t, c, _ = R.scores(kx, ky, R.ranks(dx, ky), R.ranks(dy, kx), ok, k)[2]
        assert abs(t - manifold.trustworthiness(x.astype(np.float64), y.astype(np.float64), n_neighbors=k)) <= 1e-12
        assert abs(c - manifold.trustworthiness(y.astype(np.float64), x.astype(np.float64), n_neighbors=k)) <= 1e-12


def test_reference_orders_ties_by_position():
    x = np.array([0, 1, 1, 2, 5], np.float32)[:, None]
    xs, ok = R.scaled_rows(x, np.r_[np.arange(5), -1, 1])        # a position without a row; the row at 1 a third time
    d = R.candidates(xs, ok)
    assert R.knn(d, 3).tolist() == [[1, 2, 6], [2, 6, 0], [1, 6, 0], [1, 2, 6], [3, 1, 2], [-1, -1, -1], [1, 2, 0]]
    assert R.ranks(d, np.array([[6, 4, 5]] * 7, np.int32)).tolist() == [[3, 5, 0], [2, 5, 0], [2, 5, 0], [3, 5, 0], [4, 0, 0], [0, 0, 0], [0, 5, 0]]


def test_metrics_on_hand_tables():
    from cuda_gcn_amd.model import GcnHostError, map_quality_metrics
    assert map_quality_metrics([0, 0, 100 * 5], 100, 5) == dict(trustworthiness=1.0, continuity=1.0, knn_overlap=1.0)
    worst = 100 * 5 * (200 - 15 - 1) // 2
    got = map_quality_metrics([worst, worst // 4, 125], 100, 5)
    assert got == dict(trustworthiness=0.0, continuity=0.75, knn_overlap=0.25)
    for args, msg in ((([0, 0, 0], 100, 0), "k must be in 1..32"), (([0, 0, 0], 100, 33), "k must be in 1..32"),
                      (([0, 0, 0], 10, 5), "below half the points"), (([-1, 0, 0], 100, 5), "outside their range"),
                      (([worst + 1, 0, 0], 100, 5), "outside their range"), (([0, 0, 501], 100, 5), "outside their range")):
        with pytest.raises(GcnHostError, match=msg):
            map_quality_metrics(*args)


def test_plan_and_its_refusals_need_no_gpu():
    from cuda_gcn_amd import _lib
    lib = _lib.gcnhip()
    p, s, q = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert lib.gcnhip_mapq_plan(193, 41, 10, C.byref(p), C.byref(s)) == 0 and lib.gcnhip_dbscan_plan(193, 41, C.byref(q), None) == 0
    assert p.value == q.value == 256 + 256 * (64 * 4 + 16 + 4) and s.value == 0
    for args, msg in (((64, 257, 5), b"1 <= dim <= 256"), ((64, 16, 0), b"1 <= k <= 32"), ((64, 16, 33), b"1 <= k <= 32")):
        assert lib.gcnhip_mapq_plan(*args, None, None) == -1 and msg in lib.gcnhip_last_error()
    for name in ("gcnhip_knn_rows", "gcnhip_nbr_ranks"):        # a launch is refused before anything touches a device
        assert getattr(lib, name)(None, None, 64, 16, 5, None, None) == -1 and b"invalid argument" in lib.gcnhip_last_error()
