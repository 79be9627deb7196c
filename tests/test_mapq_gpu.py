"""Map quality on the GPU (csrc/mapq.hip through ops.py and the model) against the float64 reference of tests/mapq_ref.py.  On
integer tables every d2 is exact in f32 and every output is asserted EQUAL; on float tables the rank walk is held to its own kNN
lists exactly, and to the reference within the number of candidates the f32 error bound cannot tell apart."""
import os
import subprocess

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import mapq_ref as R
from tests.dbscan_ref import intblobs
from tests.silhouette_ref import blobs
from tests.test_kmeans_gpu import dev, same_bits                                        # noqa: F401 (dev: the Device fixture)
from tests.test_silhouette_gpu import trained_planted                                    # noqa: F401 (the planted-communities model)

pytestmark = pytest.mark.gpu
HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cuda_gcn_amd", "bin", "gcn-hip")


def reference(x, y, k, rows=None):
    (xs, ok), (ys, _) = R.scaled_rows(x, rows), R.scaled_rows(y, rows)
    dx, dy = R.candidates(xs, ok), R.candidates(ys, ok)
    kx, ky = R.knn(dx, k), R.knn(dy, k)
    rx, ry = R.ranks(dx, ky), R.ranks(dy, kx)
    per, tot, sc = R.scores(kx, ky, rx, ry, ok, k)
    return dict(knn_x=kx, knn_y=ky, rank_x=rx, rank_y=ry, per_position=per, totals=tot, scores=sc, xs=xs, dx=dx)


def unit_blobs(n, dim):
    x = blobs(n, dim, 8, 1)[0].astype(np.float64)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("dim", [1, 16, 41, 128, 256])
@pytest.mark.parametrize("n", [63, 64, 65, 129, 193])
def test_exact_tables(dev, n, dim):
    """integer blobs against an integer lattice: ties everywhere, so the position rule decides; one tile, a full tile, a one-row last
    tile, three and four tiles; every padded width; then a row list that repeats rows (d2 = 0 between distinct positions) and names
    rows outside the table"""
    x = intblobs(n, dim, 4, n + dim)
    y = np.random.default_rng(n * dim).integers(0, 6, (n, 2 + dim % 2)).astype(np.float32)
    rows = np.random.default_rng(n).integers(0, n, n + 7).astype(np.int32)
    rows[[5, 11]], rows[-3:] = (-1, n + 1), rows[:3]
    for k in (1, 5, 32):
        for r in (None, rows):
            points = n if r is None else n + 5
            if not k < points / 2:
                continue
            want, got = reference(x, y, k, r), dev.map_quality_run(x, y, k, rows=r)
            for key in ("knn_x", "knn_y", "rank_x", "rank_y", "per_position", "totals"):
                assert np.array_equal(got[key], want[key]), (k, r is not None, key)
            assert (got["trustworthiness"], got["continuity"], got["knn_overlap"]) == want["scores"] and got["totals"][3] == points
            nn = dev.knn_rows(x, k, rows=r)
            assert np.array_equal(nn["pos"], want["knn_x"]) and nn["points"] == points
            d_want = np.where(want["knn_x"] >= 0, np.take_along_axis(want["dx"], np.maximum(want["knn_x"], 0), 1), np.inf)
            assert np.array_equal(nn["d2"], d_want.astype(np.float32))


@pytest.mark.parametrize("n,dim", [(193, 16), (300, 41), (193, 128), (257, 256)])
def test_the_rank_walk_sees_the_selection_walks_bits(dev, n, dim):
    """the rank of the t-th nearest neighbour is t + 1 in every row: the threshold phase, the rank walk and the selection walk form
    the same d2 bits.  No tolerance can stand in for this."""
    x = unit_blobs(n, dim)
    for k in (5, 32):
        nn = dev.knn_rows(x, k)
        assert np.array_equal(dev.nbr_ranks(x, nn["pos"]), np.tile(np.arange(1, k + 1, dtype=np.int32), (n, 1))), k
        assert same_bits(dev.nbr_d2(x, nn["pos"]), nn["d2"]), k


@pytest.mark.parametrize("n,dim", [(193, 16), (300, 41), (193, 128)])
def test_float_rows_against_the_reference(dev, n, dim):
    """unit rows against a lattice map whose kNN lists are exact: a rank may differ from the float64 one by at most the candidates
    within the f32 bound of the target's distance (few entries have any: a condition on the input), the kNN sets agree in the rows
    whose k-th gap is decided, and trustworthiness lies within the summed slack"""
    x, k = unit_blobs(n, dim), 10
    y = (np.round(64.0 * x[:, :2].astype(np.float64)) / 8.0).astype(np.float32)
    want, got = reference(x, y, k), dev.map_quality_run(x, y, k)
    assert np.array_equal(got["knn_y"], want["knn_y"])
    slack = R.slack(want["xs"], want["dx"], want["knn_y"])
    flagged = R.boundary_rows(want["xs"], want["dx"], k)
    print(f"entries with slack {np.mean(slack > 0):.4f}, rows with an undecided k-th gap {flagged.mean():.4f}")
    assert np.mean(slack > 0) <= 0.05 and flagged.mean() <= 0.05
    assert np.all(np.abs(got["rank_x"].astype(np.int64) - want["rank_x"]) <= slack)
    assert all(set(a) == set(b) for a, b in zip(got["knn_x"][~flagged], want["knn_x"][~flagged]))
    assert abs(got["trustworthiness"] - want["scores"][0]) <= slack.sum() * 2.0 / (n * k * (2 * n - 3 * k - 1))


def test_the_model_is_the_ops_path_on_its_rows(dev, trained_planted):
    ds, m = trained_planted
    table = m.embed()
    inv = dev.embed_inv_norms(table)
    q = np.random.default_rng(3).integers(0, table.shape[0], 500).astype(np.int32)
    lattice = np.round(4.0 * table[:, :3] * inv[:, None]).astype(np.float32)          # a crude map of every node; coords: of the listed ones
    coords = lattice[q]
    before = m.predict(logp=True)
    got, nn = m.map_quality(coords, k=7, nodes=q), m.knn(k=7, nodes=q)
    assert all(same_bits(a, b) for a, b in zip(before, m.predict(logp=True)))
    px = dev.knn_rows(table, 7, rows=q, inv_norm=inv)
    assert np.array_equal(nn["positions"], px["pos"]) and nn["points"] == 500
    assert np.array_equal(nn["ids"], q[px["pos"]])
    want = dev.map_quality_run(table, lattice, 7, rows=q, inv_norm=inv)
    assert np.array_equal(np.stack([got["trust_penalty"], got["cont_penalty"], got["shared"]], 1), want["per_position"])
    assert (got["trustworthiness"], got["continuity"], got["knn_overlap"], got["points"], got["k"]) == (
        want["trustworthiness"], want["continuity"], want["knn_overlap"], 500, 7)
    xs = R.scaled_rows(table, q, inv)[0]
    same = m.map_quality(xs, k=7, data=xs)                        # the map is the space itself
    assert (same["trustworthiness"], same["continuity"], same["knn_overlap"]) == (1.0, 1.0, 1.0)
    assert not same["trust_penalty"].any() and not same["cont_penalty"].any() and np.all(same["shared"] == 7)
    split3 = np.flatnonzero(np.asarray(ds["split"]) == 3)
    assert np.array_equal(m.knn(k=3, split=3)["ids"], split3[dev.knn_rows(table, 3, rows=split3, inv_norm=inv)["pos"]])
    assert "shared" not in m.map_quality(coords, k=7, nodes=q, per_node=False)


def test_a_map_quality_call_between_epochs_changes_nothing():
    from cuda_gcn_amd import model as M
    ds = datagen.make_dataset("cora-syn")
    a = M.HipGCNModel(ds, seed=6, hidden_dim=16, dropout=0.5)
    b = M.HipGCNModel(ds, seed=6, hidden_dim=16, dropout=0.5)
    ta, tb = [a.run_epochs(3)], [b.run_epochs(3)]
    b.map_quality(b.embed()[np.asarray(ds["split"]) == 3][:, :2], k=5, split=3)
    b.knn(k=4, split=2)
    ta.append(a.run_epochs(2))
    tb.append(b.run_epochs(2))
    ta, tb = np.concatenate(ta), np.concatenate(tb)
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32)), (ta, tb)
    assert a.eval(3) == b.eval(3) and all(same_bits(a.var(v), b.var(v)) for v in (2, 3, 5, 6))
    a.close()
    b.close()


def test_refusals(dev):
    from cuda_gcn_amd import model as M
    from cuda_gcn_amd.model import HipGCNModel, GcnHostError
    from cuda_gcn_amd.ops import GcnHipError
    x = blobs(64, 4, 2, 0)[0]
    for k in (0, 33):
        with pytest.raises(GcnHipError, match="1 <= k <= 32"):
            dev.knn_rows(x, k)
    with pytest.raises(GcnHipError, match="targets must be"):
        dev.nbr_ranks(x, np.zeros((63, 3), np.int32))
    with pytest.raises(GcnHostError, match="below half the points"):
        dev.map_quality_run(x, x[:, :2], 32)
    ds = datagen.make_dataset("tiny-syn")
    plain = HipGCNModel(ds, seed=1, hidden_dim=16)
    n = plain.params.num_nodes
    y = np.zeros((n, 2), np.float32)
    for call, msg in ((lambda: plain.knn(k=33), "knn: k must be an integer in 1..32"),
                      (lambda: plain.map_quality(y, k=0), "map_quality: k must be an integer in 1..32"),
                      (lambda: plain.map_quality(np.zeros((n, 300), np.float32)), "map_quality: coords must be a float"),
                      (lambda: plain.map_quality(y[:-1]), f"map_quality: the query lists {n} rows, coords has {n - 1}"),
                      (lambda: plain.knn(k=5, nodes=np.arange(10)), "knn: at least 2 k \\+ 1 = 11 rows"),
                      (lambda: plain.knn(data=np.zeros((40, 300), np.float32)), "knn: data must be a float"),
                      (lambda: plain.knn(split=3, nodes=[1, 2]), "knn: give a split or a node query, not both")):
        with pytest.raises(GcnHostError, match=msg):
            call()
    with pytest.raises(GcnHostError, match="map_quality: coords of a width in 1..256, got 300"):     # the library's own refusal, past Python's
        M._ck(plain.lib, plain.lib.gcnhost_model_map_quality(plain.h, y.ctypes.data, n, 300, 5, 0, None, 0, None, 0, 1, None, None, None), "map_quality")
    plain.close()
    bf = HipGCNModel(ds, seed=1, flags=M.BF16_TABLES, hidden_dim=16)
    for call in (lambda: bf.knn(k=3), lambda: bf.map_quality(y, k=3)):
        with pytest.raises(GcnHostError, match="not with bf16 tables"):
            call()
    bf.close()


def test_cli_tsne_quality(tmp_path):
    """GCN_TSNE_QUALITY prints, after the tsne_rows= line, what m.map_quality gives for m.tsne's map of the test split, and writes
    the per-node table; without GCN_TSNE it is refused"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.make_dataset("cora-syn")
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "cora-syn.gcnbin"))
    m = HipGCNModel(ds, seed=3, hidden_dim=16, dropout=0.5)
    m.run_epochs(6, want_trace=False)
    w = str(tmp_path / "w.gcnw")
    m.save_weights(w)
    want = m.map_quality(m.tsne(split=3, perplexity=20.0, iters=25)["coords"], k=5, split=3)
    m.close()
    args = ["timeout", "-k", "10", "50", HIP, "cora-syn", "-", "-", "16", "-", "0.5", "-", "-", "0"]
    out = str(tmp_path / "q.txt")
    env = dict(os.environ, GCN_SEED="3", GCN_LOAD_WEIGHTS=w, GCN_TSNE_QUALITY=out, GCN_TSNE_QUALITY_K="5")
    env.pop("GCN_TSNE", None)
    r0 = subprocess.run(args, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r0.returncode != 0 and "GCN_TSNE_QUALITY needs GCN_TSNE" in r0.stderr
    r1 = subprocess.run(args, cwd=str(tmp_path), env=dict(env, GCN_TSNE=str(tmp_path / "t.txt"), GCN_TSNE_ITERS="25", GCN_TSNE_PERPLEXITY="20"),
                        capture_output=True, text=True)
    assert r1.returncode == 0, r1.stderr[-1000:]
    lines = r1.stdout.strip().splitlines()
    assert lines[-2].startswith("tsne_rows=")
    fields = dict(p.split("=") for p in lines[-1].split())
    assert list(fields) == ["tsne_quality_k", "tsne_trustworthiness", "tsne_continuity", "tsne_knn_overlap"] and fields["tsne_quality_k"] == "5"
    assert [float(v) for v in list(fields.values())[1:]] == [float("%.9g" % want[key]) for key in ("trustworthiness", "continuity", "knn_overlap")]
    got = np.loadtxt(out, dtype=np.int64)
    assert np.array_equal(got[:, 0], np.flatnonzero(np.asarray(ds["split"]) == 3))
    assert np.array_equal(got[:, 1:], np.stack([want["trust_penalty"], want["cont_penalty"], want["shared"]], 1))
