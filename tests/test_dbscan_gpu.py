"""DBSCAN on the GPU (csrc/dbscan.hip through ops.py and the model) against the float64 reference of tests/dbscan_ref.py: every
output is an integer and is asserted EQUAL.  The integer tables make d2 exact in f32; the float tables are checked to hold no pair
within the f32 error bound of eps^2 before equality is asked for."""
import os
import subprocess
import threading

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import dbscan_ref as R
from tests.silhouette_ref import blobs
from tests.test_kmeans_gpu import dev, same_bits, strides                               # noqa: F401 (dev: the Device fixture)
from tests.test_silhouette_gpu import trained_planted                                    # noqa: F401 (the planted-communities model)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")


def check(dev, t, eps2, min_samples, rows=None, inv=None, ld=None):
    """dbscan_run against the reference on the same rows; returns (got, want)"""
    xs, ok = R.scaled_rows(t, rows, inv)
    want = R.dbscan(R.dist2(xs, ok), eps2, min_samples)
    got = dev.dbscan_run(t, np.sqrt(eps2), min_samples, rows=rows, inv_norm=inv, ld=ld)
    print({k: got[k] for k in R.KEYS[4:] + ("rounds",)}, "ambiguous borders", want["ambiguous"])
    assert not R.same(got, want), R.same(got, want)
    return got, want


@pytest.mark.parametrize("dim", [1, 5, 16, 41, 128, 256])
def test_bridges(dev, dim):
    """18 blocks of two clusters joined by a border point that has core neighbours in both, plus a far point: 36 clusters, 144 core,
    54 border, 18 noise; every padded width and a width that pays for padding"""
    got, want = check(dev, R.bridges(dim), 4.5, 4, ld=strides(dim, dim & 1))
    assert want["ambiguous"] >= 1 and (got["n_clusters"], got["n_core"], got["n_border"], got["n_noise"]) == (36, 144, 54, 18)


def test_a_chain(dev):
    """300 points in a row, each linked to the next only: one cluster however the positions are permuted"""
    t = np.zeros((300, 5), np.float32)
    t[:, 0] = np.random.default_rng(300).permutation(300)
    got, _ = check(dev, t, 1.5, 3)
    assert (got["n_clusters"], got["n_core"], got["n_border"]) == (1, 298, 2) and got["rounds"] >= 2


@pytest.mark.parametrize("n", [63, 64, 65, 129, 193])
def test_the_tile_seams(dev, n):
    """one tile, the diagonal tile alone, a one-row last tile, three tiles with an odd pairing of the triangle; then a row list
    with repeats and ids outside the table; then 1, 3 and 8 radii that straddle the distinct integer distances"""
    t = R.intblobs(n, 16, 4, n)
    xs, ok = R.scaled_rows(t)
    d2 = R.dist2(xs, ok)
    eps2 = round(float(np.quantile(d2[np.triu_indices(n, 1)], 0.08))) + 0.5
    check(dev, t, eps2, 5)
    rows = np.random.default_rng(n).integers(-2, n + 2, n + 7).astype(np.int32)
    rows[-3:] = rows[:3]
    got, _ = check(dev, t, eps2, 5, rows=rows, ld=strides(16, 1))
    assert got["points"] < rows.size
    xs, ok = R.scaled_rows(t, rows)
    d2 = R.dist2(xs, ok)
    radii2 = np.unique(d2[np.isfinite(d2)])[1:9] + 0.5           # between two distinct integer distances each
    for e in (1, 3, 8):
        assert np.array_equal(dev.dbscan_counts(t, np.sqrt(radii2[:e]), rows=rows), R.counts(d2, radii2[:e])), e


@pytest.mark.parametrize("n,dim,k,normalize", [(1024, 16, 8, False), (193, 128, 4, True)])
def test_float_rows(dev, n, dim, k, normalize):
    """eps^2 sits in the widest gap of the 3 %..6 % quantile window of the float64 d2; the input is checked to hold no pair within
    the f32 bound (dim + 4) 2^-24 (xn_i + xn_j) of it, a condition on the input and no tolerance: then equality"""
    t = blobs(n, dim, k, 1)[0]
    inv = dev.embed_inv_norms(t) if normalize else None
    xs, ok = R.scaled_rows(t, inv=inv)
    eps2, margin = R.gap_eps2(R.dist2(xs, ok), xs)
    print(f"eps2 {eps2:.6g}: the nearest pair is {margin:.2f} bounds away")
    assert margin > 1.0
    got, _ = check(dev, t, eps2, 5, inv=inv)
    assert got["n_clusters"] >= k // 2 and got["n_border"] > 0 and got["n_noise"] > 0


def test_the_model_is_the_ops_path_on_its_rows(dev, trained_planted):
    ds, m = trained_planted
    table = m.embed()
    inv = dev.embed_inv_norms(table)
    q = np.random.default_rng(2).integers(0, table.shape[0], 700).astype(np.int32)
    xs, ok = R.scaled_rows(table, q, inv)
    eps = float(np.sqrt(np.quantile(R.dist2(xs, ok), 0.05)))
    before = m.predict(logp=True)
    got = m.dbscan(eps, nodes=q)
    assert all(same_bits(a, b) for a, b in zip(before, m.predict(logp=True)))
    want = dev.dbscan_run(table, eps, 5, rows=q, inv_norm=inv)
    assert not R.same(got, want) and got["rounds"] == want["rounds"] and 1 <= got["n_clusters"] <= 256
    lab = np.asarray(ds["label"])[q]
    assert got["contingency"].shape == (got["n_clusters"], m.params.output_dim) and got["skipped"] == got["n_noise"]
    assert np.array_equal(got["contingency"], np.histogram2d(got["labels"][got["labels"] >= 0], lab[got["labels"] >= 0],
                                                             bins=(got["n_clusters"], m.params.output_dim),
                                                             range=((0, got["n_clusters"]), (0, m.params.output_dim)))[0])
    assert 0.0 <= got["nmi"] <= 1.0 and "contingency" not in m.dbscan(eps, nodes=q, report=False)
    sweep = [0.5 * eps, eps, 2 * eps]
    assert np.array_equal(m.neighbor_counts(sweep, split=3),
                          dev.dbscan_counts(table, sweep, rows=np.flatnonzero(np.asarray(ds["split"]) == 3), inv_norm=inv))
    raw = m.dbscan(1.0, data=xs, min_samples=3)                   # the same rows as data: no scaling, no report
    assert not R.same(raw, dev.dbscan_run(xs, 1.0, 3)) and "contingency" not in raw


def test_a_dbscan_call_between_epochs_changes_nothing():
    from cuda_gcn_amd import model as M
    ds = datagen.make_dataset("cora-syn")
    a = M.HipGCNModel(ds, seed=6, hidden_dim=16, dropout=0.5)
    b = M.HipGCNModel(ds, seed=6, hidden_dim=16, dropout=0.5)
    ta, tb = [a.run_epochs(3)], [b.run_epochs(3)]
    b.dbscan(0.3, split=3)
    b.neighbor_counts([0.1, 0.3], split=2)
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
    for e in ([], [1.0] * 9):
        with pytest.raises(GcnHipError, match="1 <= E <= 8 radii"):
            dev.dbscan_counts(x, e)
    for e in (0.0, -1.0, np.inf):
        with pytest.raises(GcnHipError, match="eps must be finite and above 0"):
            dev.dbscan_counts(x, [1.0, e])
    with pytest.raises(GcnHipError, match="min_samples must be at least 1"):
        dev.dbscan_run(x, 1.0, 0)
    with pytest.raises(GcnHipError, match="1 <= dim <= 256"):
        dev.dbscan_plan(64, 257)
    ds = datagen.make_dataset("tiny-syn")
    plain, wide = HipGCNModel(ds, seed=1, hidden_dim=16), np.zeros((4, 300), np.float32)
    with pytest.raises(GcnHostError, match="dbscan: data must be a float"):
        plain.dbscan(1.0, data=wide)
    with pytest.raises(GcnHostError, match="dbscan: data of a width in 1..256, got 300"):    # the library's own refusal, past Python's
        M._ck(plain.lib, plain.lib.gcnhost_model_dbscan(plain.h, 1.0, 5, 0, None, 4, wide.ctypes.data, 300, 1, 4, *[None] * 6), "dbscan")
    for kwargs, msg in ((dict(eps=0.0), "eps must be finite"), (dict(eps=1.0, min_samples=0), "min_samples must be at least 1")):
        with pytest.raises(GcnHostError, match="dbscan: " + msg):
            plain.dbscan(**kwargs)
    plain.close()
    bf = HipGCNModel(ds, seed=1, flags=M.BF16_TABLES, hidden_dim=16)
    for call in (lambda: bf.dbscan(1.0), lambda: bf.neighbor_counts([1.0])):
        with pytest.raises(GcnHostError, match="not with bf16 tables"):
            call()
    bf.close()
    tw = ThreadWorld(2)
    seen, errors = [None, None], []

    def body(rank):
        try:
            ag, ar = tw.callbacks(rank)
            r = HipGCNModel(ds, seed=4, device=0, rank=rank, world=2, host_allgather=ag, host_allreduce=ar, hidden_dim=16, dropout=0.5)
            try:
                r.dbscan(1.0)
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
    assert all("dbscan: one rank only" in s for s in seen), seen


def test_cli_dbscan(tmp_path):
    """GCN_DBSCAN writes what m.dbscan gives for the test split; a run without the variable prints what it printed before"""
    from cuda_gcn_amd.model import HipGCNModel, read_dbscan
    ds = datagen.make_dataset("cora-syn")
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "cora-syn.gcnbin"))
    m = HipGCNModel(ds, seed=3, hidden_dim=16, dropout=0.5)
    m.run_epochs(6, want_trace=False)
    w = str(tmp_path / "w.gcnw")
    m.save_weights(w)
    want = m.dbscan(0.25, min_samples=4, split=3)
    m.close()
    args = ["timeout", "-k", "10", "50", HIP, "cora-syn", "-", "-", "16", "-", "0.5", "-", "-", "0"]
    env = dict(os.environ, GCN_SEED="3", GCN_LOAD_WEIGHTS=w)
    [env.pop(key, None) for key in ("GCN_DBSCAN", "GCN_DBSCAN_EPS", "GCN_DBSCAN_MIN_SAMPLES")]
    out = str(tmp_path / "d.txt")
    r0 = subprocess.run(args, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    r1 = subprocess.run(args, cwd=str(tmp_path), env=dict(env, GCN_DBSCAN=out, GCN_DBSCAN_EPS="0.25", GCN_DBSCAN_MIN_SAMPLES="4"), capture_output=True,
                        text=True)
    assert r0.returncode == 0 and r1.returncode == 0, (r0.stderr[-1000:], r1.stderr[-1000:])
    l0, l1 = r0.stdout.strip().splitlines(), r1.stdout.strip().splitlines()
    assert len(l1) == len(l0) + 1 and "dbscan" not in r0.stdout
    fields = dict(p.split("=") for p in l1[-1].split())
    assert list(fields) == ["dbscan_eps", "dbscan_min_samples", "dbscan_clusters", "dbscan_core", "dbscan_border", "dbscan_noise"]
    assert [int(fields[k]) for k in list(fields)[1:]] == [4, want["n_clusters"], want["n_core"], want["n_border"], want["n_noise"]]
    got = read_dbscan(out)
    assert np.array_equal(got["node"], np.flatnonzero(np.asarray(ds["split"]) == 3)) and np.array_equal(got["label"], want["labels"])
    assert np.array_equal(got["core"], want["core"]) and np.array_equal(got["count"], want["counts"]) and float(fields["dbscan_eps"]) == 0.25
