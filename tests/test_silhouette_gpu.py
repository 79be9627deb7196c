"""Silhouette widths on the GPU: the kernels of csrc/silhouette.hip through ops.py — bit for bit on small-integer tables, whose every
squared distance is an integer, and within the derived bounds of tests/silhouette_ref.py on real-valued ones — several segments and
row batches, the totals, then the model's silhouette() against the ops path on its own rows, no side effects on training,
refusals, and the command line (GCN_CLUSTER_SILHOUETTE).

The share of points whose neighbour the bound leaves open is a condition on the INPUTS (it is computed from the float64 reference
alone) and is held to test_kmeans_gpu's AMBIGUOUS_CAP on every (dim, k, scaled or not) but one family: dim = 1 with inverse norms.
There every scaled row is +1 or -1, every label whose points share a sign lies at distance 0 from all of them, and the reference
itself cannot tell those labels apart: its open share is 0 at k = 2, 0.23 at k = 7 and 1.0 from k = 64 on, whatever computes the
sums.  Those cases keep every other check (S, a, b, s inside their bounds, the neighbour wherever it is decided); their share
is printed and not capped."""
import os
import subprocess
import threading

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import silhouette_ref as R
from tests.test_kmeans_gpu import AMBIGUOUS_CAP, integer_table, row_list, same_bits, strides

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")
N = 1000
DIMS = [1, 5, 16, 41, 128, 256]
KS = [1, 2, 7, 64, 65, 200, 256]


@pytest.fixture(scope="module")
def dev():
    from cuda_gcn_amd.ops import Device
    d = Device(0)
    yield d
    d.close()


def same_values(a, b):
    """the same bits, NaN matching NaN"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and same_bits(np.where(nan, 0, a), np.where(nan, 0, b).astype(a.dtype))


def valid_rows(rows, n_table):
    return None if rows is None else (rows >= 0) & (rows < n_table)


def check_rows_exact(dev, sums, lab, sizes, rows, n_table):
    """the rows launch against widths() of the SAME sums, bit for bit; returns the launch's dict"""
    got = dev.silhouette_rows(sums, lab, sizes, n_table, rows=rows)
    want = R.widths(sums, lab, sizes, valid_rows(rows, n_table))
    for key in ("s", "a", "b"):
        assert same_values(got[key], want[key]), key
    assert np.array_equal(got["neighbor"], want["neighbor"])
    pts = ~np.isnan(want["s"])
    assert got["points"] == int(pts.sum()) == int(np.sum(sizes)) and got["excluded"] == int((~pts).sum())
    assert got["nonempty"] == int(np.sum(np.asarray(sizes) > 0)) and (got["nonempty"] >= 2) == want["defined"]
    assert np.all(np.isfinite(got["s"][pts])) and np.all(np.abs(got["s"][pts]) <= 1.0)
    return got


# ---- exact ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", DIMS)
def test_sums_and_widths_are_exact_on_integer_tables(dev, dim):
    """every d^2 is an integer below 2^24, sqrtf is correctly rounded, and a float64 sum of fewer than 2^17 such values is exact
    in any order: sums, sizes, and everything derived from them have the reference's bits"""
    t = integer_table(N, dim, 300 + dim)
    combo = 0
    for k in KS:
        for rows in (None, row_list(N, k + dim)):
            n = N if rows is None else rows.size
            lab = np.random.default_rng(31 * k + dim + combo).integers(-1, k, n).astype(np.int32)
            if k >= 200:                                          # by construction: an empty label, a singleton, a label of -1
                lab[lab >= k - 2] = 0
                lab[3], lab[7] = k - 2, -1
            ld = strides(dim, combo % 2)
            combo += 1
            sums, sizes = dev.silhouette_sums(t, lab, k, rows=rows, ld=ld)
            want, want_sizes = R.sums64(t, lab, k, rows=rows, f32_sqrt=True)
            assert np.array_equal(sizes, want_sizes), (k, rows is None)
            assert same_bits(sums, want), (k, rows is None, ld, float(np.abs(sums - want).max()))
            got = check_rows_exact(dev, sums, lab, sizes, rows, N)
            if rows is not None:
                assert np.all(np.isnan(got["s"][[5, 17]])) and np.all(got["neighbor"][[5, 17]] == -1) and np.all(sums[[5, 17]] == 0)
            if k >= 200:
                assert np.any(sizes == 0) and np.any(sizes == 1) and np.any(lab == -1)
                single = np.flatnonzero((lab >= 0) & (sizes[np.maximum(lab, 0)] == 1) & ~np.isnan(got["s"]))
                assert single.size and np.all(got["s"][single] == 0) and np.all(got["a"][single] == 0)
    # every point in one label: nothing to compare with
    lab = np.zeros(N, np.int32)
    sums, sizes = dev.silhouette_sums(t, lab, 7)
    got = check_rows_exact(dev, sums, lab, sizes, None, N)
    assert got["nonempty"] == 1 and np.all(got["s"] == 0) and np.all(got["neighbor"] == -1) and got["total"] == 0.0


# ---- real tables ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", DIMS)
def test_real_tables_stay_inside_the_bound(dev, dim):
    for i, k in enumerate(KS):
        x, l = R.blobs(N, dim, k, 1000 * dim + k)
        inv = dev.embed_inv_norms(x)
        rows = row_list(N, k) if i % 3 == 0 else None
        lab = l if rows is None else l[np.clip(rows, 0, N - 1)]
        for use_inv in (None, inv):
            sums, sizes = dev.silhouette_sums(x, lab, k, rows=rows, inv_norm=use_inv, ld=strides(dim, i % 2))
            ref, ref_sizes, E = R.sums64(x, lab, k, inv=use_inv, rows=rows, bounds=True)
            assert np.array_equal(sizes, ref_sizes)
            over = np.abs(sums - ref) - E
            assert np.all(over <= 0), f"dim {dim} k {k}: a sum is {float(over.max()):.3e} beyond its bound"
            got = check_rows_exact(dev, sums, lab, sizes, rows, N)
            w = R.widths(ref, lab, ref_sizes, valid_rows(rows, N))
            B = R.width_bounds(ref, E, lab, ref_sizes, valid_rows(rows, N))
            pts = ~np.isnan(w["s"])
            for key in ("a", "b", "s"):
                over = np.abs(got[key][pts] - w[key][pts]) - B[key][pts]
                assert np.all(over <= 0), f"dim {dim} k {k}: {key} is {float(over.max()):.3e} beyond its bound"
            decided = B["decided"] & pts
            assert np.array_equal(got["neighbor"][decided], w["neighbor"][decided]), (dim, k)
            share = float(1.0 - B["decided"][pts].mean()) if pts.any() else 0.0
            print(f"dim {dim} k {k} scaled {use_inv is not None}: undecided share {share:.4f}")
            if not (dim == 1 and use_inv is not None):             # the module docstring: unit rows in one dimension
                assert share <= AMBIGUOUS_CAP, (dim, k, share)


# ---- several segments, several batches ----------------------------------------------------------------------------------------

def test_segments_and_batches_give_the_same_bits(dev):
    """n = 5000, k = 2: each label spans five segments of 512 members; the plan's bytes, its minimum and a size between them"""
    n, k, dim = 5000, 2, 16
    t = integer_table(n, dim, 77)
    lab = R.blobs(n, dim, k, 5)[1]
    plan = dev.silhouette_plan(n, k, dim)
    assert plan["bytes_min"] < plan["bytes"]
    want, want_sizes = R.sums64(t, lab, k, f32_sqrt=True)
    assert want_sizes.min() >= 3 * 512
    runs = []
    for sbytes in (plan["bytes"], plan["bytes_min"], (plan["bytes"] + plan["bytes_min"]) // 2, plan["bytes"]):
        sums, sizes = dev.silhouette_sums(t, lab, k, scratch_bytes=sbytes)
        assert np.array_equal(sizes, want_sizes) and same_bits(sums, want), sbytes
        runs.append(sums)
    # real rows: no reference has these bits, every scratch size has the same
    x = R.blobs(n, dim, k, 5)[0]
    inv = dev.embed_inv_norms(x)
    real = [dev.silhouette_sums(x, lab, k, inv_norm=inv, scratch_bytes=b)[0]
            for b in (plan["bytes"], plan["bytes_min"], (plan["bytes"] + plan["bytes_min"]) // 2, plan["bytes"])]
    assert all(same_bits(real[0], r) for r in real[1:])
    from cuda_gcn_amd.ops import GcnHipError
    with pytest.raises(GcnHipError, match="gcnhip_silhouette_sums: the scratch is below the minimum"):
        dev.silhouette_sums(t, lab, k, scratch_bytes=plan["bytes_min"] - 256)


# ---- totals -----------------------------------------------------------------------------------------------------------------

def test_totals_are_the_sums_of_the_returned_widths(dev):
    for dim, k in ((5, 7), (41, 65), (16, 256)):
        x, l = R.blobs(N, dim, k, dim + k)
        rows = row_list(N, dim)
        lab = l[np.clip(rows, 0, N - 1)]
        sums, sizes = dev.silhouette_sums(x, lab, k, rows=rows)
        got = dev.silhouette_rows(sums, lab, sizes, N, rows=rows)
        again = dev.silhouette_rows(sums, lab, sizes, N, rows=rows)
        assert same_bits(got["cluster_sum"], again["cluster_sum"]) and got["total"] == again["total"]
        s = got["s"]
        pts = ~np.isnan(s)
        n = rows.size
        for c in range(k):
            mine = s[pts & (lab == c)]
            assert abs(got["cluster_sum"][c] - mine.sum()) <= n * 2.0 ** -52 * np.abs(mine).sum(), c
            if sizes[c] == 0:
                assert got["cluster_sum"][c] == 0.0
        assert abs(got["total"] - s[pts].sum()) <= n * 2.0 ** -52 * np.abs(s[pts]).sum()


# ---- the model --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def trained_planted():
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.planted_communities(n_comm=8, size=128, p_in=0.5, feats=8)
    m = HipGCNModel(ds, seed=5, hidden_dim=16, dropout=0.0)
    m.run_epochs(10, want_trace=False)
    yield ds, m
    m.close()


def ops_path(dev, table, inv, lab, k, rows=None):
    sums, sizes = dev.silhouette_sums(table, lab, k, rows=rows, inv_norm=inv)
    out = dev.silhouette_rows(sums, lab, sizes, table.shape[0], rows=rows)
    with np.errstate(divide="ignore", invalid="ignore"):
        out.update(sizes=sizes, cluster_mean=np.where(sizes > 0, out["cluster_sum"] / sizes.astype(np.float64), 0.0),
                   score=out["total"] / out["points"] if out["points"] else 0.0)
    return out


def test_silhouette_is_the_ops_path_on_the_models_rows(dev, trained_planted):
    ds, m = trained_planted
    table = m.embed()
    inv = dev.embed_inv_norms(table)
    test_nodes = np.flatnonzero(np.asarray(ds["split"]) == 3).astype(np.int32)
    repeats = np.array([7, 7, 7, 2, 2, 9] + list(range(100, 160)) + [7, 300, 301, 2], np.int32)
    for k, split, nodes, rows in ((8, None, None, None), (5, 3, None, test_nodes), (3, None, repeats, repeats)):
        lab = m.cluster(k=k, split=split, nodes=nodes, iters=30, report=False)["assign"]
        for normalize, f in ((True, inv), (False, None)):
            got = m.silhouette(lab, k=k, split=split, nodes=nodes, normalize=normalize)
            want = ops_path(dev, table, f, lab, k, rows=rows)
            for key in ("s", "a", "b", "cluster_mean"):
                assert same_values(got[key], want[key]), (k, normalize, key)
            assert np.array_equal(got["neighbor"], want["neighbor"]) and np.array_equal(got["sizes"], want["sizes"])
            assert got["score"] == want["score"] and got["points"] == want["points"] == lab.size and got["excluded"] == 0 and got["defined"]
            assert np.array_equal(got["sizes"], np.bincount(lab, minlength=k))
        brief = m.silhouette(lab, split=split, nodes=nodes, per_node=False, scratch_bytes=1)      # k = labels.max() + 1; the least scratch
        assert "s" not in brief and brief["score"] == m.silhouette(lab, k=int(lab.max()) + 1, split=split, nodes=nodes)["score"]
    # a label outside [0, k) takes its position out; the labels of the clustering sit better than the same labels with 30 % shuffled
    lab = m.cluster(k=8, iters=50, report=False)["assign"]
    good = m.silhouette(lab, k=8)
    out = lab.copy()
    out[[3, 500]] = [-1, 8]
    part = m.silhouette(out, k=8)
    assert part["excluded"] == 2 and part["points"] == lab.size - 2 and np.all(np.isnan(part["s"][[3, 500]])) and np.all(part["neighbor"][[3, 500]] == -1)
    assert same_values(part["s"], ops_path(dev, table, inv, out, 8)["s"])
    rng = np.random.default_rng(1)
    mixed = lab.copy()
    pick = np.flatnonzero(rng.random(lab.size) < 0.3)
    mixed[pick] = lab[rng.permutation(pick)]
    worse = m.silhouette(mixed, k=8)
    print(f"score {good['score']:.4f}, with 30 % of the labels shuffled {worse['score']:.4f}")
    assert good["score"] > worse["score"] and -1.0 <= worse["score"] and good["score"] <= 1.0
    one = m.silhouette(np.zeros(lab.size, np.int32), k=4)
    assert not one["defined"] and one["score"] == 0.0 and np.all(one["s"] == 0) and np.all(one["neighbor"] == -1)


def test_a_silhouette_call_between_epochs_changes_nothing():
    from cuda_gcn_amd import model as M
    ds = datagen.make_dataset("cora-syn")
    a = M.HipGCNModel(ds, seed=6, hidden_dim=16, dropout=0.5)
    b = M.HipGCNModel(ds, seed=6, hidden_dim=16, dropout=0.5)
    ta, tb = [a.run_epochs(3)], [b.run_epochs(3)]
    before = b.predict(logp=True)
    lab = np.asarray(ds["label"]).astype(np.int32)
    b.silhouette(lab)
    test = np.asarray(ds["split"]) == 2
    b.silhouette(lab[test], k=ds["output_dim"], split=2, normalize=False, per_node=False)
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
    from cuda_gcn_amd import model as M
    from cuda_gcn_amd.model import HipGCNModel, GcnHostError, _ck
    from tests.mr_threads import ThreadWorld
    ds = datagen.make_dataset("tiny-syn")
    n = ds["num_nodes"]
    m = HipGCNModel(ds, seed=1, hidden_dim=16)
    lab = np.zeros(n, np.int32)

    def raw(k=2, split=0, nodes=None, count=0, capacity=n):
        return m.lib.gcnhost_model_silhouette(m.h, split, nodes, count, lab.ctypes.data, k, 1, 0, capacity, None, None, None, None, None, None, None, None)
    for k in (0, 257):
        with pytest.raises(GcnHostError, match=r"silhouette: k must be in 1\.\.256"):
            _ck(m.lib, raw(k=k), "call")
    with pytest.raises(GcnHostError, match=f"silhouette: the query lists {n} rows, the labels are {n - 1}"):
        _ck(m.lib, raw(capacity=n - 1), "call")
    with pytest.raises(GcnHostError, match="silhouette: invalid argument"):
        _ck(m.lib, raw(split=4), "call")
    with pytest.raises(GcnHostError, match="silhouette: .*not a node of the dataset"):
        m.silhouette(np.zeros(2, np.int32), k=1, nodes=[0, n])
    n_test = int((np.asarray(ds["split"]) == 3).sum())
    with pytest.raises(GcnHostError, match=f"silhouette: the query lists {n_test} rows, the labels are {n}"):
        m.silhouette(lab, k=2, split=3)
    assert m.silhouette(np.zeros(0, np.int32), k=2, nodes=[])["points"] == 0
    m.close()
    bf = HipGCNModel(ds, seed=1, flags=M.BF16_TABLES, hidden_dim=16)
    with pytest.raises(GcnHostError, match="silhouette: not with bf16 tables"):
        bf.silhouette(lab, k=2)
    bf.close()
    tw = ThreadWorld(2)
    seen, errors = [None, None], []

    def body(rank):
        try:
            ag, ar = tw.callbacks(rank)
            r = HipGCNModel(ds, seed=4, device=0, rank=rank, world=2, host_allgather=ag, host_allreduce=ar, hidden_dim=16, dropout=0.5)
            try:
                r.silhouette(lab, k=2)
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
    assert all("silhouette: one rank only" in s for s in seen), seen


# ---- the command line -------------------------------------------------------------------------------------------------------

def test_cli_cluster_silhouette(tmp_path):
    """gcn-hip cora-syn with GCN_CLUSTER and GCN_CLUSTER_SILHOUETTE: one further line whose score is the mean of the file's column;
    the GCN_CLUSTER line and file are those of a run without the new variable, byte for byte; the variable alone is refused"""
    from cuda_gcn_amd.model import HipGCNModel, read_silhouette
    ds = datagen.make_dataset("cora-syn")
    n = ds["num_nodes"]
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "cora-syn.gcnbin"))
    m = HipGCNModel(ds, seed=3, hidden_dim=16, dropout=0.5)
    m.run_epochs(6, want_trace=False)
    w = str(tmp_path / "w.gcnw")
    m.save_weights(w)
    lab = m.cluster(k=5, iters=30, seed=11, report=False)["assign"]
    want = m.silhouette(lab, k=5)
    m.close()
    args = ["cora-syn", "-", "-", "16", "-", "0.5", "-", "-", "0"]
    plain, out, sil = str(tmp_path / "c0.txt"), str(tmp_path / "c1.txt"), str(tmp_path / "s.txt")
    env = dict(os.environ, GCN_SEED="3", GCN_LOAD_WEIGHTS=w, GCN_CLUSTER=plain, GCN_CLUSTER_K="5", GCN_CLUSTER_ITERS="30", GCN_CLUSTER_SEED="11")
    env.pop("GCN_CLUSTER_SILHOUETTE", None)
    r0 = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r0.returncode == 0, r0.stderr[-2000:]
    r1 = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=dict(env, GCN_CLUSTER=out, GCN_CLUSTER_SILHOUETTE=sil),
                        capture_output=True, text=True)
    assert r1.returncode == 0, r1.stderr[-2000:]
    l0, l1 = r0.stdout.strip().splitlines(), r1.stdout.strip().splitlines()
    assert len(l1) == len(l0) + 1                                 # the lines before the clustering's carry timings
    assert l1[-2] == l0[-1] and l0[-1].startswith("clusters=5 ") and open(plain, "rb").read() == open(out, "rb").read()
    fields = dict(p.split("=") for p in l1[-1].split())
    assert list(fields) == ["silhouette", "silhouette_min_cluster", "silhouette_negative"]
    got = read_silhouette(sil)
    assert np.array_equal(got["node"], np.arange(n)) and np.array_equal(got["cluster"], lab) and np.array_equal(got["neighbor"], want["neighbor"])
    assert abs(float(fields["silhouette"]) - got["s"].mean()) <= 1e-6
    assert np.all(np.abs(got["s"] - want["s"]) <= 1e-8) and abs(float(fields["silhouette"]) - want["score"]) <= 1e-8
    assert abs(float(fields["silhouette_min_cluster"]) - want["cluster_mean"].min()) <= 1e-8
    assert abs(float(fields["silhouette_negative"]) - float((want["s"] < 0).mean())) <= 1e-6
    env.pop("GCN_CLUSTER")
    bad = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=dict(env, GCN_CLUSTER_SILHOUETTE=sil), capture_output=True,
                         text=True)
    assert bad.returncode != 0 and "GCN_CLUSTER_SILHOUETTE needs GCN_CLUSTER" in bad.stderr, bad.stderr[-500:]
