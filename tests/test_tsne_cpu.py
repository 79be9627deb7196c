"""The t-SNE reference and the host-only pieces: tsne_ref's P against scikit-learn's, read_tsne, the "auto" learning rate."""
import numpy as np
import pytest

from tests import tsne_ref as R
from tests.silhouette_ref import blobs


def test_reference_p_is_scikit_learns():
    pytest.importorskip("sklearn")
    from sklearn.manifold import _t_sne
    from scipy.spatial.distance import squareform
    x = blobs(150, 8, 4, 2)[0]
    xs, ok = R.scaled_rows(x)
    d2 = R.dist2(xs, ok)
    P = R.joint(d2, R.bandwidths(d2, 20.0)[0])
    d = np.where(np.isfinite(d2), d2, 0.0).astype(np.float32)
    want = squareform(_t_sne._joint_probabilities(d, 20.0, 0))
    # both searches stop within 1e-5 of the entropy; scikit-learn's runs on f32 distances and stores f32 conditionals
    assert np.abs(P - want).max() <= 1e-4 * want.max() and abs(P.sum() - 1.0) <= 1e-12


def test_read_tsne(tmp_path):
    from cuda_gcn_amd.model import GcnHostError, read_tsne
    p = tmp_path / "t.txt"
    p.write_text("3 0.5 -1.25\n\n7 1e-3 2\n")
    got = read_tsne(str(p))
    assert np.array_equal(got["node"], [3, 7]) and np.array_equal(got["coords"], [[0.5, -1.25], [1e-3, 2.0]])
    p.write_text("3 0.5 -1.25\n7 1 2 3\n")
    with pytest.raises(GcnHostError, match=r"read_tsne: .*:2: expected `node y1 \.\. yk`"):
        read_tsne(str(p))


def test_auto_learning_rate_and_the_update_rule():
    assert R.auto_learning_rate(193) == 50.0 and R.auto_learning_rate(48000) == 1000.0
    x = blobs(40, 3, 2, 0)[0]
    xs, ok = R.scaled_rows(x, rows=np.r_[np.arange(40), -1])
    d2 = R.dist2(xs, ok)
    beta, conv = R.bandwidths(d2, 5.0)
    P = R.joint(d2, beta)
    assert conv[:40].all() and abs(P.sum() - 1.0) <= 1e-12 and not P[40].any()
    y = np.random.default_rng(0).standard_normal((41, 2))
    one = R.run(P, y, 1, learning_rate=10.0)                      # update = 0, gain = 1: the first step shrinks the gain to 0.8
    assert np.allclose(one[:40], y[:40] - 10.0 * 0.8 * R.gradient(P, y, 12.0)[0][:40], rtol=1e-12, atol=0) and np.all(np.isnan(one[40]))
