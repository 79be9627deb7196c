"""k-means on the GPU: the kernels of csrc/kmeans.hip through ops.py — exactly, on small-integer tables whose every distance is an
integer, and within the derived bounds of tests/kmeans_ref.py on real-valued ones — a Lloyd loop checked step by step against the
reference on the GPU's own inputs, then the model's cluster() against the ops loop on its own rows, its row queries, its table
against the labels, no side effects on training, refusals, and the command line (GCN_CLUSTER)."""
import os
import subprocess
import threading

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import kmeans_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")
N = 1000
DIMS = [1, 5, 16, 41, 128, 256]
KS = [1, 2, 7, 64, 65, 200, 256]
AMBIGUOUS_CAP = 0.03


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def dev():
    from cuda_gcn_amd.ops import Device
    d = Device(0)
    yield d
    d.close()


def integer_table(n, dim, seed):
    """entries in {-3..3}; at least 30 % of the rows are copies of other rows (test_embed_gpu.integer_table)"""
    rng = np.random.default_rng(seed)
    t = rng.integers(-3, 4, (n, dim)).astype(np.float32)
    where = rng.choice(n, (3 * n + 9) // 10, replace=False)
    t[where] = t[rng.integers(0, n, where.size)]
    return t


def integer_centres(t, k, seed):
    """integer centres: copies of table rows, fresh rows, and exact duplicates of each other"""
    rng = np.random.default_rng(seed)
    m = rng.integers(-3, 4, (k, t.shape[1])).astype(np.float32)
    take = rng.random(k) < 0.5
    m[take] = t[rng.integers(0, t.shape[0], int(take.sum()))]
    if k > 1:
        dup = rng.choice(k, max(k // 4, 1), replace=False)
        m[dup] = m[rng.integers(0, k, dup.size)]
    return m


def strides(dim, which):
    return dim + 3 if which else (dim + 3) // 4 * 4 + 4


def row_list(n, seed):
    """a list with repeats, an id of -1 and an id of n"""
    q = np.random.default_rng(seed).integers(0, n, n - 90).astype(np.int32)
    q[5], q[17], q[-1] = -1, n, q[0]
    return q


# ---- assign -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", DIMS)
def test_assign_is_exact_on_integer_tables(dev, dim):
    t = integer_table(N, dim, dim)
    rng = np.random.default_rng(100 + dim)
    combo = 0
    for k in KS:
        m = integer_centres(t, k, 7 * k + dim)
        cn = R.cn_f32(m)
        assert np.all(cn == (m.astype(np.int64) ** 2).sum(axis=1))
        for rows in (None, row_list(N, k)):
            ld, ldm = strides(dim, combo % 2), strides(dim, (combo // 2) % 2)
            combo += 1
            want_a, want_d = R.assign_exact(t, m, cn, rows=rows)
            prev = np.where(rng.random(want_a.size) < 0.5, want_a, rng.integers(-1, k, want_a.size)).astype(np.int32)
            a, d, moved = dev.kmeans_assign(t, m, cn, rows=rows, prev=prev, ld=ld, ldm=ldm)
            assert np.array_equal(a, want_a) and same_bits(d, want_d), (k, rows is None, ld, ldm)
            assert moved == int((want_a != prev).sum())
            a2, d2, moved2 = dev.kmeans_assign(t, m, cn, rows=rows, ld=ld, ldm=ldm)
            assert same_bits(a, a2) and same_bits(d, d2) and moved2 == want_a.size
            if rows is not None:
                assert np.all(a[[5, 17]] == -1) and np.all(np.isnan(d[[5, 17]]))


@pytest.mark.parametrize("dim", DIMS)
def test_assign_on_real_tables_stays_inside_the_bound(dev, dim):
    """standard normal rows, centres = rows plus 0.25 noise; with and without inverse norms (the kernel's own)"""
    rng = np.random.default_rng(dim)
    x = rng.standard_normal((N, dim)).astype(np.float32)
    inv = dev.embed_inv_norms(x)
    for i, k in enumerate(KS):
        m = (x[rng.integers(0, N, k)] + 0.25 * rng.standard_normal((k, dim))).astype(np.float32)
        use_inv = inv if i % 2 else None
        rows = row_list(N, k) if i % 3 == 0 else None
        cn = R.cn_f32(m)
        a, d, _ = dev.kmeans_assign(x, m, cn, rows=rows, inv_norm=use_inv, ld=strides(dim, i % 2), ldm=strides(dim, 1 - i % 2))
        share = R.check_assign(x, m, cn, a, d, inv=use_inv, rows=rows)
        print(f"dim {dim} k {k}: ambiguous share {share:.4f}")
        assert share <= AMBIGUOUS_CAP, (dim, k, share)


# ---- update -----------------------------------------------------------------------------------------------------------------

def some_assignment(n, k, seed, leave_empty=True):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, k, n).astype(np.int32)
    if k > 1 and leave_empty:
        a[a == k - 1] = 0                                         # centre k - 1 stays empty
    a[rng.random(n) < 0.02] = -1
    return a


@pytest.mark.parametrize("dim", DIMS)
def test_update_is_exact_on_integer_tables(dev, dim):
    t = integer_table(N, dim, 50 + dim)
    for i, k in enumerate(KS):
        rows = row_list(N, 3 * k) if i % 2 else None
        n = N if rows is None else rows.size
        a = some_assignment(n, k, k + dim)
        prev = np.random.default_rng(k).integers(-9, 10, (k, dim)).astype(np.float32) + 0.5      # sentinel rows, NaN-free
        plan = dev.kmeans_plan(n, k, dim)
        got = dev.kmeans_update(t, a, prev, rows=rows, ld=strides(dim, i % 2), ldm=strides(dim, 1 - i % 2))
        R.check_update(t, a, prev, got, rows=rows, exact=True)
        if k > 1:
            assert got["sizes"][k - 1] == 0 and same_bits(got["centers"][k - 1], prev[k - 1])
        small = dev.kmeans_update(t, a, prev, rows=rows, ld=strides(dim, i % 2), ldm=strides(dim, 1 - i % 2), scratch_bytes=plan["update_bytes_min"])
        for key in ("centers", "sizes", "cn"):
            assert same_bits(got[key], small[key]), (k, key)
        assert got["inertia"] == 0.0 == small["inertia"]


@pytest.mark.parametrize("dim", [1, 41, 256])
def test_update_on_real_tables_is_within_an_ulp(dev, dim):
    rng = np.random.default_rng(dim + 1)
    x = rng.standard_normal((N, dim)).astype(np.float32)
    inv = dev.embed_inv_norms(x)
    for i, k in enumerate([1, 7, 65, 256]):
        use_inv = inv if i % 2 == 0 else None
        rows = row_list(N, k + 1) if i % 2 else None
        n = N if rows is None else rows.size
        a = some_assignment(n, k, k)
        dist2 = np.where(a >= 0, rng.random(n) * 3, np.nan).astype(np.float32)
        if rows is not None:
            dist2[(rows < 0) | (rows >= N)] = np.nan
        prev = rng.standard_normal((k, dim)).astype(np.float32)
        plan = dev.kmeans_plan(n, k, dim)
        got = dev.kmeans_update(x, a, prev, dist2=dist2, rows=rows, inv_norm=use_inv)
        R.check_update(x, a, prev, got, inv=use_inv, rows=rows)
        small = dev.kmeans_update(x, a, prev, dist2=dist2, rows=rows, inv_norm=use_inv, scratch_bytes=plan["update_bytes_min"])
        assert all(same_bits(got[key], small[key]) for key in ("centers", "sizes", "cn")) and got["inertia"] == small["inertia"]
        member = np.isfinite(dist2)
        total = float(dist2[member].astype(np.float64).sum())
        assert abs(got["inertia"] - total) <= n * 2.0 ** -52 * total
        # position order is part of the definition: a permuted list gives other bits, inside the same bound
        order = rng.permutation(n)
        base = np.arange(N, dtype=np.int32) if rows is None else rows
        perm = dev.kmeans_update(x, a[order], prev, dist2=dist2[order], rows=base[order], inv_norm=use_inv)
        R.check_update(x, a[order], prev, perm, inv=use_inv, rows=base[order])
        assert np.array_equal(perm["sizes"], got["sizes"])
        assert abs(perm["inertia"] - total) <= n * 2.0 ** -52 * total


def test_contingency_counts(dev):
    rng = np.random.default_rng(3)
    for k, c in ((1, 1), (7, 5), (41, 41), (256, 64)):
        truth = rng.integers(-1, c + 1, N).astype(np.int32)
        for rows in (None, row_list(N, k)):
            n = N if rows is None else rows.size
            a = rng.integers(-1, k, n).astype(np.int32)
            got, skipped = dev.contingency_rows(a, truth, k, c, rows=rows)
            want, want_skipped = R.contingency(a, truth, k, c, rows=rows)
            assert np.array_equal(got, want) and skipped == want_skipped and got.sum() + skipped == n


# ---- seeding ----------------------------------------------------------------------------------------------------------------

def test_seeding_follows_the_float64_race(dev):
    k = 64
    for dim, seed in ((5, 1), (41, 2 ** 63 + 12345), (128, 77)):
        s = seed ^ R.KEY_KMEANS
        t = integer_table(N, dim, dim + 9)
        for rows in (None, row_list(N, dim)):
            want, leads = R.seed64(t, k, s, rows=rows)
            assert np.all(leads > 1e-9), "the test's own inputs: a step of the reference race is too close to call"
            pos, m = dev.kmeans_seed(t, k, s, rows=rows, ld=strides(dim, 1), ldm=strides(dim, 0))
            n = N if rows is None else rows.size
            assert pos[0] == (int(R.seed_word(0, 0, s)) * n) >> 32
            assert np.array_equal(pos, want), (dim, rows is None)
            r = pos if rows is None else rows[pos]
            assert same_bits(m, t[r])
            pos2, m2 = dev.kmeans_seed(t, k, s, rows=rows)
            assert same_bits(pos, pos2) and same_bits(m, m2)
            other, _ = dev.kmeans_seed(t, k, (seed + 1) ^ R.KEY_KMEANS, rows=rows)
            assert not np.array_equal(other, pos)
    # real rows, scaled by the kernel's own inverse norms
    rng = np.random.default_rng(8)
    for dim in (16, 41):
        x = rng.standard_normal((N, dim)).astype(np.float32)
        inv = dev.embed_inv_norms(x)
        s = 99 ^ R.KEY_KMEANS
        want, leads = R.seed64(x, k, s, inv=inv)
        assert np.all(leads > 4 * (dim + 2) * R.U)
        pos, m = dev.kmeans_seed(x, k, s, inv_norm=inv)
        assert np.array_equal(pos, want)
        assert same_bits(m, R.scaled_f32(x, inv, pos))


def test_seeding_edge_cases(dev):
    rng = np.random.default_rng(4)
    five = rng.integers(-3, 4, (5, 9)).astype(np.float32)
    assert np.unique(five, axis=0).shape[0] == 5
    t = five[rng.integers(0, 5, N)]
    pos, m = dev.kmeans_seed(t, 8, 5 ^ R.KEY_KMEANS)
    assert np.unique(m[:5], axis=0).shape[0] == 5                 # five distinct rows first
    assert np.all(pos[5:] == 0) and np.unique(m, axis=0).shape[0] == 5      # then every weight is zero: the lowest position, thrice
    assert np.array_equal(pos, R.seed64(t, 8, 5 ^ R.KEY_KMEANS)[0])
    # two far-apart groups: the second seed lies in the other one
    group = rng.integers(0, 2, N)
    x = (rng.standard_normal((N, 6)) + 1000.0 * group[:, None]).astype(np.float32)
    for seed in range(20):
        pos, _ = dev.kmeans_seed(x, 2, seed ^ R.KEY_KMEANS)
        assert group[pos[0]] != group[pos[1]], seed


# ---- Lloyd, step by step ----------------------------------------------------------------------------------------------------

def planted_table(n, dim, groups, seed):
    rng = np.random.default_rng(seed)
    centres = 3.0 * rng.standard_normal((groups, dim))
    g = rng.integers(0, groups, n)
    return (centres[g] + rng.standard_normal((n, dim))).astype(np.float32), g


def test_lloyd_in_lockstep_with_the_reference(dev):
    dim, k = 24, 9
    x, _ = planted_table(N, dim, k, 21)
    _, m = dev.kmeans_seed(x, k, 3 ^ R.KEY_KMEANS)
    cn = R.cn_f32(m)
    prev, history = None, []
    for it in range(10):
        a, d, moved = dev.kmeans_assign(x, m, cn, prev=prev)
        assert R.check_assign(x, m, cn, a, d) <= AMBIGUOUS_CAP
        assert moved == (N if prev is None else int((a != prev).sum()))
        d64, E, xn, _ = R.assign64(x, m, cn)
        slack = float((E[np.arange(N), a] + (dim + 3) * R.U * xn).sum())
        got = dev.kmeans_update(x, a, m, dist2=d)
        R.check_update(x, a, m, got)
        total = float(d.astype(np.float64).sum())
        assert abs(got["inertia"] - total) <= N * 2.0 ** -52 * total
        history.append((got["inertia"], slack))
        m, cn, prev = got["centers"], got["cn"], a
    for (a0, s0), (a1, s1) in zip(history, history[1:]):
        assert a1 <= a0 + s0 + s1, history                          # Lloyd never raises the inertia; each side carries its f32 error
    assert history[-1][0] < 0.9 * history[0][0]


# ---- the model --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def trained_planted():
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.planted_communities(n_comm=8, size=128, p_in=0.5, feats=8)
    m = HipGCNModel(ds, seed=5, hidden_dim=16, dropout=0.0)
    m.run_epochs(10, want_trace=False)
    yield ds, m
    m.close()


def ops_loop(dev, table, inv, centres, iters, rows=None):
    m = np.ascontiguousarray(centres, np.float32)
    cn = dev.kmeans_update(table, np.zeros(0, np.int32), m, rows=np.zeros(0, np.int32), inv_norm=inv)["cn"]
    prev, hist = None, []
    for _ in range(iters):
        a, d, moved = dev.kmeans_assign(table, m, cn, rows=rows, inv_norm=inv, prev=prev)
        got = dev.kmeans_update(table, a, m, dist2=d, rows=rows, inv_norm=inv)
        m, cn, prev = got["centers"], got["cn"], a
        hist.append((moved, got["inertia"]))
        if moved == 0:
            break
    return dict(assign=a, dist2=d, centers=m, sizes=got["sizes"], history=np.array(hist, np.float64))


def test_cluster_is_the_ops_loop_on_the_models_rows(dev, trained_planted):
    ds, m = trained_planted
    n, k = ds["num_nodes"], 8
    table = m.embed()
    inv = dev.embed_inv_norms(table)
    assert same_bits(m.embed(normalize=True), dev.embed_rows(table, inv_norm=inv))
    start = np.ascontiguousarray(m.embed(nodes=np.arange(0, n, n // k)[:k], normalize=True))
    for normalize, f in ((True, inv), (False, None)):
        got = m.cluster(k=k, init=start, iters=25, normalize=normalize)
        want = ops_loop(dev, table, f, start, 25)
        for key in ("assign", "dist2", "centers", "sizes", "history"):
            assert same_bits(got[key], want[key]), (normalize, key)
        assert got["iters_run"] == len(want["history"]) and got["converged"] == (want["history"][-1, 0] == 0)
        assert got["inertia"] == want["history"][-1, 1] and got["seed_pos"] is None
    # the table against the labels, counted on the GPU; the scores are cluster_report's
    from cuda_gcn_amd.model import cluster_report
    full = m.cluster(k=k, iters=50)
    cont = np.zeros((k, ds["output_dim"]), np.int64)
    np.add.at(cont, (full["assign"], np.asarray(ds["label"])), 1)
    assert np.array_equal(full["contingency"], cont) and full["skipped"] == 0
    rep = cluster_report(cont)
    assert all(full[key] == rep[key] for key in rep)
    assert np.array_equal(full["sizes"], np.bincount(full["assign"], minlength=k))
    again = m.cluster(k=k, iters=50)
    assert all(same_bits(full[key], again[key]) for key in ("assign", "dist2", "centers", "seed_pos", "history"))
    assert not np.array_equal(m.cluster(k=k, iters=1, seed=123)["seed_pos"], full["seed_pos"])
    # a converged run is a fixed point: one more reference assignment moves only rows inside the margin
    assert full["converged"], full["history"]
    R.check_assign(table, full["centers"], R.cn_f32(full["centers"]), full["assign"], full["dist2"], inv=inv)
    # the small-scratch path gives the same bits
    small = m.cluster(k=k, iters=50, scratch_bytes=1)
    assert all(same_bits(full[key], small[key]) for key in ("assign", "dist2", "centers", "history"))


def test_split_and_node_queries_agree(trained_planted):
    ds, m = trained_planted
    test_nodes = np.flatnonzero(np.asarray(ds["split"]) == 3).astype(np.int32)
    a = m.cluster(k=5, split=3, iters=20, seed=9)
    b = m.cluster(k=5, nodes=test_nodes, iters=20, seed=9)
    assert a["assign"].size == test_nodes.size
    for key in ("assign", "dist2", "centers", "sizes", "seed_pos", "history", "contingency"):
        assert same_bits(a[key], b[key]), key
    pos = np.array([0, 3, 9, 4, 11], np.int32)
    c = m.cluster(k=5, nodes=test_nodes, init=pos, iters=3, report=False)
    d = m.cluster(k=5, nodes=test_nodes, init=m.embed(nodes=test_nodes[pos], normalize=True), iters=3, report=False)
    assert "contingency" not in c and all(same_bits(c[key], d[key]) for key in ("assign", "dist2", "centers"))
    rep = m.cluster(k=3, nodes=[7, 7, 7, 2, 2, 9], iters=5, report=False)      # repeats are rows of their own
    assert rep["assign"][0] == rep["assign"][1] == rep["assign"][2] and rep["assign"][3] == rep["assign"][4]


def test_a_cluster_call_between_epochs_changes_nothing():
    from cuda_gcn_amd import model as M
    ds = datagen.make_dataset("cora-syn")
    a = M.HipGCNModel(ds, seed=6, hidden_dim=16, dropout=0.5)
    b = M.HipGCNModel(ds, seed=6, hidden_dim=16, dropout=0.5)
    ta, tb = [a.run_epochs(3)], [b.run_epochs(3)]
    before = b.predict(logp=True)
    b.cluster(iters=5)
    b.cluster(k=3, split=2, normalize=False, iters=2)
    assert all(same_bits(x, y) for x, y in zip(before, b.predict(logp=True)))
    ta.append(a.run_epochs(2))
    tb.append(b.run_epochs(2))
    ta, tb = np.concatenate(ta), np.concatenate(tb)
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32)), (ta, tb)
    for v in (2, 5):
        assert same_bits(a.var(v), b.var(v)), v
    assert a.eval(3) == b.eval(3) and same_bits(a.var(6), b.var(6)) and same_bits(a.var(3), b.var(3))
    a.close()
    b.close()


def test_refusals():
    from cuda_gcn_amd.model import HipGCNModel, GcnHostError, _ck
    from tests.mr_threads import ThreadWorld
    ds = datagen.make_dataset("tiny-syn")
    n = ds["num_nodes"]
    m = HipGCNModel(ds, seed=1, hidden_dim=16)
    for k in (0, 257, "ten", 2.5):
        with pytest.raises(GcnHostError, match="cluster: k must be"):
            m.cluster(k=k)
    buf = np.zeros(n, np.int32)

    def raw(k=2, nodes=None, count=0, init=0, iters=5):
        return m.lib.gcnhost_model_kmeans(m.h, k, 0, nodes, count, iters, 1, init, None, None, None, 0, n, buf.ctypes.data, None, None, None, None, None,
                                          None, None, None, None)
    for k in (0, 257):
        with pytest.raises(GcnHostError, match=r"kmeans: k must be in 1\.\.256"):
            _ck(m.lib, raw(k=k), "call")
    with pytest.raises(GcnHostError, match="kmeans: k = 4 is above the 3 rows listed"):
        m.cluster(k=4, nodes=[0, 1, 2])
    with pytest.raises(GcnHostError, match="kmeans: iters must be at least 1"):
        _ck(m.lib, raw(iters=0), "call")
    with pytest.raises(GcnHostError, match="kmeans: .*not a node of the dataset"):
        m.cluster(k=1, nodes=[0, n])
    for bad in (np.zeros((2, 15), np.float32), np.zeros((3, 16), np.float32), np.zeros(3, np.int32), "random"):
        with pytest.raises(GcnHostError, match="cluster: init"):
            m.cluster(k=2, init=bad)
    with pytest.raises(GcnHostError, match="kmeans: initial position"):
        m.cluster(k=2, nodes=[0, 1, 2], init=np.array([0, 3]))
    with pytest.raises(GcnHostError, match="cluster: give a split or a node query"):
        m.cluster(split=1, nodes=[0])
    m.close()
    tw = ThreadWorld(2)
    seen, errors = [None, None], []

    def body(rank):
        try:
            ag, ar = tw.callbacks(rank)
            r = HipGCNModel(ds, seed=4, device=0, rank=rank, world=2, host_allgather=ag, host_allreduce=ar, hidden_dim=16, dropout=0.5)
            try:
                r.cluster(k=2)
                seen[rank] = "no error"
            except GcnHostError as e:
                seen[rank] = str(e)
            r.close()
        except BaseException as e:                                # a failed rank must not leave the other at a barrier forever
            errors.append((rank, e))
            tw.barrier.abort()
    threads = [threading.Thread(target=body, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert all("kmeans: one rank only" in s for s in seen), seen


# ---- the command line -------------------------------------------------------------------------------------------------------

def test_cli_cluster(tmp_path):
    """gcn-hip cora-syn with GCN_CLUSTER: stdout keeps its lines and gains one; the file parses to the Python call on the same
    weights (handed over through a weights file, 0 epochs); the file's clusters reproduce the printed scores"""
    from cuda_gcn_amd.model import HipGCNModel, cluster_report
    ds = datagen.make_dataset("cora-syn")
    n, c = ds["num_nodes"], ds["output_dim"]
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "cora-syn.gcnbin"))
    m = HipGCNModel(ds, seed=3, hidden_dim=16, dropout=0.5)
    m.run_epochs(6, want_trace=False)
    w = str(tmp_path / "w.gcnw")
    m.save_weights(w)
    want = m.cluster(k=5, iters=30, seed=11)
    m.close()
    args = ["cora-syn", "-", "-", "16", "-", "0.5", "-", "-", "0"]
    out = str(tmp_path / "c.txt")
    env = dict(os.environ, GCN_SEED="3", GCN_LOAD_WEIGHTS=w, GCN_CLUSTER=out, GCN_CLUSTER_K="5", GCN_CLUSTER_ITERS="30", GCN_CLUSTER_SEED="11")
    r = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-2].startswith("test_loss=") and lines[-1].startswith("clusters=5 ")
    fields = dict(p.split("=") for p in lines[-1].split())
    assert list(fields) == ["clusters", "cluster_iters", "cluster_inertia", "cluster_nmi", "cluster_ari", "cluster_purity"]
    rows = np.loadtxt(out, ndmin=2)
    assert rows.shape == (n, 3) and np.array_equal(rows[:, 0], np.arange(n))
    assert np.array_equal(rows[:, 1].astype(np.int32), want["assign"]) and same_bits(rows[:, 2].astype(np.float32), want["dist2"])
    assert int(fields["cluster_iters"]) == want["iters_run"] and abs(float(fields["cluster_inertia"]) - want["inertia"]) <= 1e-6 * want["inertia"]
    test = np.asarray(ds["split"]) == 3
    cont = np.zeros((5, c), np.int64)
    np.add.at(cont, (rows[test, 1].astype(np.int64), np.asarray(ds["label"])[test]), 1)
    rep = cluster_report(cont)
    for name in ("nmi", "ari", "purity"):
        assert abs(float(fields["cluster_" + name]) - rep[name]) <= 5e-7, (name, fields, rep)
    bad = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=dict(env, GCN_GPUS="2"), capture_output=True, text=True)
    assert bad.returncode != 0 and "GCN_CLUSTER runs on one GPU" in bad.stderr, bad.stderr[-500:]
