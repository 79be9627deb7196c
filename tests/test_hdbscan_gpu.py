"""HDBSCAN on the GPU (csrc/hdbscan.hip through ops.py and the model) against tests/hdbscan_ref.py.  On integer tables every d2 is exact
in f32 and ties are everywhere: only the order (w, lo, hi), honoured from both ends of an edge, makes the tree unique: asserted EQUAL."""
import os
import subprocess
import threading

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import dbscan_ref as D
from tests import hdbscan_ref as R
from tests.silhouette_ref import blobs
from tests.test_kmeans_gpu import dev, same_bits, strides                               # noqa: F401 (dev: the Device fixture)
from tests.test_silhouette_gpu import trained_planted                                    # noqa: F401 (the planted-communities model)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")


def equal_tree(dev, t, min_samples, rows=None, ld=None):
    """hdbscan_mst against Kruskal on the same rows: every edge, its weight's bits and the core distances"""
    xs, ok = D.scaled_rows(t, rows)
    d2 = D.dist2(xs, ok)
    c2 = R.core2(d2, min_samples)
    lo, hi, w = R.mst(d2, c2)
    got = dev.hdbscan_mst(t, min_samples, rows=rows, ld=ld)
    assert got["points"] == ok.sum() and got["lo"].size == max(got["points"] - 1, 0)
    assert np.array_equal(got["core2"][ok], c2[ok].astype(np.float32))
    assert np.array_equal(got["lo"], lo) and np.array_equal(got["hi"], hi) and same_bits(got["d2"], w.astype(np.float32))
    return got


@pytest.mark.parametrize("n", [63, 64, 65, 129, 193])
def test_the_tile_seams(dev, n):
    """one tile, the diagonal alone, a one-row last tile, an odd pairing; then repeats (w = 0 edges) and ids outside the table (in no edge)"""
    t = D.intblobs(n, 16, 4, n)
    equal_tree(dev, t, 5)
    rows = np.random.default_rng(n).integers(-2, n + 2, n + 7).astype(np.int32)
    rows[-3:] = rows[:3]
    got = equal_tree(dev, t, 1, rows=rows, ld=strides(16, 1))
    assert got["points"] < rows.size and (got["d2"] == 0).any()


@pytest.mark.parametrize("dim,min_samples", [(1, 4), (5, 4), (16, 4), (41, 4), (128, 4), (256, 4), (5, 1), (5, 2), (5, 5), (5, 33)])
def test_every_width_and_core_distance(dev, dim, min_samples):
    equal_tree(dev, D.bridges(dim), min_samples, ld=strides(dim, dim & 1))


def test_a_chain(dev):
    """300 points in a row in permuted positions: a component grows by a few points a round"""
    t = np.zeros((300, 5), np.float32)
    t[:, 0] = np.random.default_rng(300).permutation(300)
    got = equal_tree(dev, t, 1)
    assert 2 <= got["rounds"] <= int(np.ceil(np.log2(300)))


@pytest.mark.parametrize("n,dim,k", [(1024, 16, 8), (193, 128, 4)])
def test_float_rows(dev, n, dim, k):
    """unit float rows: a spanning tree whose sorted float64 weights lie within 2 (dim + 4) 2^-24 (xn_i + xn_j) of the reference
    tree's — the sorted weights of a minimum spanning tree move by at most the largest change of an edge weight, once for the
    kernel's f32 and once for the recomputation: twice the bound dbscan_ref.gap_eps2 uses, derived and not measured"""
    t = blobs(n, dim, k, 1)[0]
    inv = dev.embed_inv_norms(t)
    xs, ok = D.scaled_rows(t, inv=inv)
    d2 = D.dist2(xs, ok)
    c2 = R.core2(d2, 5)
    lo, hi, want = R.mst(d2, c2)
    w = np.maximum(d2, np.maximum(c2[:, None], c2[None, :]))
    got = dev.hdbscan_mst(t, 5, inv_norm=inv)
    from cuda_gcn_amd.model import hdbscan_tree                   # it refuses rows that are not one sorted tree
    assert got["lo"].size == n - 1 and (got["lo"] < got["hi"]).all() and hdbscan_tree(got["lo"], got["hi"], got["d2"], n)["points"] == n
    xn = (xs.astype(np.float64) ** 2).sum(axis=1)
    bound = 2 * (dim + 4) * 2.0 ** -24 * (xn[lo] + xn[hi])
    err = np.abs(np.sort(w[got["lo"], got["hi"]]) - want)
    print("largest error over its bound", float((err / bound).max()), "rounds", got["rounds"])
    assert (err <= bound).all()


def test_the_model_is_the_ops_path_on_its_rows(dev, trained_planted):
    ds, m = trained_planted
    table = m.embed()
    inv = dev.embed_inv_norms(table)
    q = np.random.default_rng(2).integers(0, table.shape[0], 700).astype(np.int32)
    before = m.predict(logp=True)
    got = m.hdbscan(min_cluster_size=8, nodes=q)
    assert all(same_bits(a, b) for a, b in zip(before, m.predict(logp=True)))
    from cuda_gcn_amd.model import hdbscan_tree
    t = dev.hdbscan_mst(table, 8, rows=q, inv_norm=inv)
    want = hdbscan_tree(t["lo"], t["hi"], t["d2"], 700, 8)
    assert np.array_equal(got["labels"], want["labels"]) and same_bits(got["probabilities"], want["probabilities"])
    assert same_bits(got["linkage"], want["linkage"]) and got["rounds"] == t["rounds"] and got["points"] == 700
    assert np.array_equal(got["mst"]["lo"], t["lo"]) and np.array_equal(got["mst"]["hi"], t["hi"])
    assert same_bits(got["mst"]["distance"], np.sqrt(t["d2"].astype(np.float64))) and same_bits(got["core_distance"], np.sqrt(t["core2"].astype(np.float64)))
    k, lab, c = got["n_clusters"], np.asarray(ds["label"])[q], m.params.output_dim
    assert k >= 2 and got["n_noise"] == (got["labels"] < 0).sum() and np.array_equal(got["sizes"], np.bincount(got["labels"][got["labels"] >= 0]))
    assert np.array_equal(got["contingency"], np.histogram2d(got["labels"][got["labels"] >= 0], lab[got["labels"] >= 0], bins=(k, c),
                                                             range=((0, k), (0, c)))[0])
    assert 0.0 <= got["nmi"] <= 1.0 and "contingency" not in m.hdbscan(min_cluster_size=8, nodes=q, report=False)
    again = m.hdbscan(min_cluster_size=8, nodes=q)
    assert all(same_bits(got[key], again[key]) for key in ("labels", "probabilities", "linkage", "core_distance", "contingency"))
    assert all(same_bits(got["mst"][key], again["mst"][key]) for key in got["mst"])
    leaf, t3 = m.hdbscan(8, 3, nodes=q, cluster_selection_method="leaf"), dev.hdbscan_mst(table, 3, rows=q, inv_norm=inv)
    assert np.array_equal(leaf["labels"], hdbscan_tree(t3["lo"], t3["hi"], t3["d2"], 700, 8, cluster_selection_method="leaf")["labels"])
    xs = D.scaled_rows(table, q, inv)[0]
    raw = m.hdbscan(min_cluster_size=8, data=xs)                  # the same rows as data: no scaling, no report
    t = dev.hdbscan_mst(xs, 8)
    assert np.array_equal(raw["labels"], hdbscan_tree(t["lo"], t["hi"], t["d2"], 700, 8)["labels"]) and "contingency" not in raw


def test_a_hdbscan_call_between_epochs_changes_nothing():
    from cuda_gcn_amd import model as M
    ds = datagen.make_dataset("cora-syn")
    a = M.HipGCNModel(ds, seed=6, hidden_dim=16, dropout=0.5)
    b = M.HipGCNModel(ds, seed=6, hidden_dim=16, dropout=0.5)
    ta, tb = [a.run_epochs(3)], [b.run_epochs(3)]
    b.hdbscan(split=3)
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
    from tests.mr_threads import ThreadWorld
    x = blobs(64, 4, 2, 0)[0]
    for call, msg in ((lambda: dev.hdbscan_mst(x, 0), "min_samples must be in 1..33"), (lambda: dev.hdbscan_mst(x, 34), "min_samples must be in 1..33"),
                      (lambda: dev.hdbscan_mst(x, 33), "at least 2 .min_samples - 1. . 1 = 65 points"),
                      (lambda: dev.hdbscan_plan(64, 257), "1 <= dim <= 256"), (lambda: dev.hdbscan_plan(65537, 16), "at most 65536 positions")):
        with pytest.raises(GcnHipError, match=msg):
            call()
    ds = datagen.make_dataset("tiny-syn")
    plain, wide = HipGCNModel(ds, seed=1, hidden_dim=16), np.zeros((4, 300), np.float32)
    with pytest.raises(GcnHostError, match="hdbscan: data of a width in 1..256, got 300"):   # the library's own refusal, past Python's
        M._ck(plain.lib, plain.lib.gcnhost_model_hdbscan(plain.h, 5, 5, 0, None, 4, wide.ctypes.data, 300, 1, 0, 0, 4, *[None] * 10), "hdbscan")
    for kwargs, msg in ((dict(min_cluster_size=1), "min_cluster_size must be at least 2"), (dict(min_samples=0), "min_samples must be in 1..33"),
                        (dict(min_samples=34), "min_samples must be in 1..33"), (dict(nodes=np.arange(9), min_samples=6), "at least 2 .min_samples"),
                        (dict(data=np.zeros((65537, 2), np.float32)), "at most 65536 rows")):
        with pytest.raises(GcnHostError, match="hdbscan: " + msg):
            plain.hdbscan(**kwargs)
    plain.close()
    bf = HipGCNModel(ds, seed=1, flags=M.BF16_TABLES, hidden_dim=16)
    with pytest.raises(GcnHostError, match="not with bf16 tables"):
        bf.hdbscan()
    bf.close()
    tw = ThreadWorld(2)
    seen, errors = [None, None], []

    def body(rank):
        try:
            ag, ar = tw.callbacks(rank)
            r = HipGCNModel(ds, seed=4, device=0, rank=rank, world=2, host_allgather=ag, host_allreduce=ar, hidden_dim=16, dropout=0.5)
            try:
                r.hdbscan()
                seen[rank] = "no error"
            except GcnHostError as e:
                seen[rank] = str(e)
            r.close()
        except BaseException as e:                                # a failed rank must not leave the other at a barrier forever
            errors.append((rank, e))
            tw.barrier.abort()
    threads = [threading.Thread(target=body, args=(r,)) for r in range(2)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errors, errors
    assert all("hdbscan: one rank only" in s for s in seen), seen


def test_cli_hdbscan(tmp_path):
    """GCN_HDBSCAN writes what m.hdbscan gives for the test split; a run without the variable prints what it printed before"""
    from cuda_gcn_amd.model import HipGCNModel, read_hdbscan
    ds = datagen.make_dataset("cora-syn")
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "cora-syn.gcnbin"))
    m = HipGCNModel(ds, seed=3, hidden_dim=16, dropout=0.5)
    m.run_epochs(6, want_trace=False)
    w = str(tmp_path / "w.gcnw")
    m.save_weights(w)
    want = m.hdbscan(min_cluster_size=6, min_samples=4, split=3)
    m.close()
    args = ["timeout", "-k", "10", "50", HIP, "cora-syn", "-", "-", "16", "-", "0.5", "-", "-", "0"]
    env = dict(os.environ, GCN_SEED="3", GCN_LOAD_WEIGHTS=w)
    [env.pop(key, None) for key in ("GCN_HDBSCAN", "GCN_HDBSCAN_MIN_CLUSTER_SIZE", "GCN_HDBSCAN_MIN_SAMPLES")]
    out = str(tmp_path / "h.txt")
    r0 = subprocess.run(args, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    r1 = subprocess.run(args, cwd=str(tmp_path), env=dict(env, GCN_HDBSCAN=out, GCN_HDBSCAN_MIN_CLUSTER_SIZE="6", GCN_HDBSCAN_MIN_SAMPLES="4"),
                        capture_output=True, text=True)
    assert r0.returncode == 0 and r1.returncode == 0, (r0.stderr[-1000:], r1.stderr[-1000:])
    l0, l1 = r0.stdout.strip().splitlines(), r1.stdout.strip().splitlines()
    assert len(l1) == len(l0) + 1 and "hdbscan" not in r0.stdout
    fields = dict(p.split("=") for p in l1[-1].split())
    assert list(fields) == ["hdbscan_min_cluster_size", "hdbscan_min_samples", "hdbscan_clusters", "hdbscan_noise", "hdbscan_rounds"]
    assert [int(v) for v in fields.values()] == [6, 4, want["n_clusters"], want["n_noise"], want["rounds"]]
    got = read_hdbscan(out)
    assert np.array_equal(got["node"], np.flatnonzero(np.asarray(ds["split"]) == 3)) and np.array_equal(got["label"], want["labels"])
    assert np.array_equal(got["probability"], want["probabilities"])
