"""Neighbourhood overlap on the GPU (csrc/overlap.hip through ops.py, the model and the command line) against the Python sets of
tests/overlap_ref.py: every integer is asserted EQUAL, on every lane group, cut, slice and lookup."""
import os
import subprocess

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from cuda_gcn_amd import model as M
from tests import overlap_ref as R
from tests.irregular_inputs import gpu_graph
from tests.test_kmeans_gpu import dev                                                   # noqa: F401 (the Device fixture)

pytestmark = pytest.mark.gpu
HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cuda_gcn_amd", "bin", "gcn-hip")
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1025, 4097)       # stored entries of rows 0 .. 10: each side of every cut
HUB = 10


def handmade(n=6000):
    """rows 0 .. 10 with the stored lengths above, each (from 63 on) holding the self entry twice, a repeated entry, the entry
    n_rows and the hub; the other rows a few drawn entries, one-way, some of them naming the special rows"""
    rng = np.random.default_rng(77)
    rows = []
    for v in range(n):
        if v >= len(LENGTHS):
            r = rng.integers(0, n, int(rng.integers(0, 7)))
            r[rng.random(r.size) < 0.2] = rng.integers(0, len(LENGTHS))
        elif LENGTHS[v] < 3:
            r = np.array([v, HUB][:LENGTHS[v]])
        else:
            base = rng.choice(np.setdiff1d(np.arange(n), [v, HUB]), LENGTHS[v] - 5, replace=False)
            r = rng.permutation(np.concatenate([base, [v, v, base[0], n, HUB if v != HUB else base[1]]]))
        rows.append(np.asarray(r, np.int64))
    indptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
    assert tuple(np.diff(indptr)[:len(LENGTHS)]) == LENGTHS
    return indptr, np.concatenate(rows).astype(np.int32), n + 1


def planted(n=600, k=6):
    rng = np.random.default_rng(78)
    c = rng.integers(0, k, n)
    a = np.triu(rng.random((n, n)) < np.where(c[:, None] == c[None, :], 0.12, 0.004), 1)
    a = a | a.T
    indptr = np.concatenate([[0], np.cumsum(a.sum(1))]).astype(np.int32)
    return indptr, np.nonzero(a)[1].astype(np.int32), n


@pytest.fixture(scope="module")
def graphs(dev):
    out = {}
    for name, (indptr, indices, n_cols) in dict(handmade=handmade(), irregular=gpu_graph() + (1500,), planted=planted()).items():
        g = dev.graph(indptr, indices, n_cols=n_cols, col_deg=np.ones(n_cols, np.int32))
        out[name] = dict(indptr=indptr, n=indptr.size - 1, S=R.sets(indptr, indices), g=g, sets=dev.overlap_sets(g), ref={})
    return out


def listed(case, kind):
    n = case["n"]
    hub = int(np.argmax(np.diff(case["indptr"])))
    if kind == "list":
        r = np.random.default_rng(5).integers(0, n, 300)
        return np.concatenate([r, r[:40], [-1, n, hub, hub], np.arange(min(n, 12))]).astype(np.int32)
    return None if kind == "all" else np.zeros(0, np.int32)


def reference(case, kind):
    if kind not in case["ref"]:
        case["ref"][kind] = R.rows(case["S"], listed(case, kind))
    return case["ref"][kind]


@pytest.mark.parametrize("name", ["handmade", "irregular", "planted"])
def test_the_canonical_pass_gives_the_sorted_sets(graphs, name):
    case = graphs[name]
    idx, length = case["sets"][0].download(), case["sets"][1].download()
    assert np.array_equal(length[:case["n"]], [len(s) for s in case["S"]])
    for v, s in enumerate(case["S"]):
        assert np.array_equal(idx[case["indptr"][v]:case["indptr"][v] + len(s)], sorted(s)), v


@pytest.mark.parametrize("path", [dict(), dict(bitmap=0), dict(slice=64), dict(slice=64, bitmap=0), dict(slice=64, wg_cut=1 << 20)], ids=str)
@pytest.mark.parametrize("group", [0, 4, 16, 64])
@pytest.mark.parametrize("name", ["handmade", "irregular", "planted"])
def test_rows_equal_the_reference_on_every_path(dev, graphs, name, group, path):
    """the defaults, no bitmap (LDS list), a slice of 64 entries (the global and the swapped search behind the groups, the pool
    too small for the hub behind the workgroup), and no workgroup rows at all"""
    case = graphs[name]
    for kind in ("all", "list", "empty"):
        t2, deg, tot, skipped = reference(case, kind)
        got = dev.overlap_rows(case["g"], case["sets"], rows=listed(case, kind), group=group, **path)
        assert np.array_equal(got["t2"], t2) and np.array_equal(got["deg"], deg), kind
        assert got["totals"].tolist() == tot and got["skipped"] == skipped, kind
        assert int(got["t2"].sum()) == got["totals"][4]
    t2, _, tot, _ = reference(case, "all")
    if name == "planted":                                      # symmetric: every closed wedge is seen from both ends, every triangle six times
        assert not (np.asarray(t2) % 2).any() and tot[4] % 6 == 0 and tot[4] > 0
    for want in (("t2",), ("deg",), ()):
        got = dev.overlap_rows(case["g"], case["sets"], want=want, group=group, **path)
        assert got["totals"].tolist() == reference(case, "all")[2] and (got["t2"] is None) == ("t2" not in want)


@pytest.mark.parametrize("path", [dict(), dict(bitmap=0), dict(slice=64, bitmap=0), dict(slice=64, wg_cut=1 << 20)], ids=str)
@pytest.mark.parametrize("group", [0, 4, 16, 64])
@pytest.mark.parametrize("name", ["handmade", "irregular"])
def test_pairs_equal_the_reference_on_every_path(dev, graphs, name, group, path):
    case = graphs[name]
    n, rng = case["n"], np.random.default_rng(9)
    hub = int(np.argmax(np.diff(case["indptr"])))
    big = np.argsort(np.diff(case["indptr"]))[-3:]
    src = np.concatenate([rng.integers(0, n, 300), [hub, hub, 3, -1, 5, big[0], big[1]], rng.integers(0, 12, 40)]).astype(np.int32)
    dst = np.concatenate([rng.integers(0, n, 300), [hub, 7, 3, 4, n, big[1], hub], rng.integers(0, 12, 40)]).astype(np.int32)
    wt = rng.integers(0, 1 << 40, case["g"].n_cols).astype(np.int64)
    if "pairs" not in case["ref"]:
        case["ref"]["pairs"] = R.pairs(case["S"], src.tolist(), dst.tolist(), wt)
    cn, un, ws, skipped = case["ref"]["pairs"]
    got = dev.overlap_pairs(case["g"], case["sets"], src, dst, wt=wt, group=group, **path)
    assert np.array_equal(got["cn"], cn) and np.array_equal(got["un"], un) and np.array_equal(got["wsum"], ws) and got["skipped"] == skipped == 2
    got = dev.overlap_pairs(case["g"], case["sets"], src, dst, want=("cn", "wsum"), group=group, **path)
    assert np.array_equal(got["cn"], cn) and not got["wsum"].any() and got["un"] is None


def test_ops_refusals(dev, graphs):
    case = graphs["planted"]
    for kw, text in ((dict(group=8), "lane group"), (dict(slice=-1), "slice"), (dict(bitmap=2), "bitmap"), (dict(group=4, slice=1 << 20), "LDS")):
        with pytest.raises(Exception, match=text):
            dev.overlap_rows(case["g"], case["sets"], **kw)
    rect = dev.graph(np.array([0, 1, 2, 3], np.int32), np.array([0, 1, 0], np.int32), n_cols=2, col_deg=np.ones(2, np.int32))
    with pytest.raises(Exception, match="fewer columns than rows"):
        dev.overlap_sets(rect)


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def trained():
    ds = datagen.make_dataset("tiny-syn")
    m = M.HipGCNModel(ds, seed=3, hidden_dim=16, dropout=0.5)
    m.run_epochs(3, want_trace=False)
    yield ds, m, R.sets(ds["g_indptr"], ds["g_indices"])
    m.close()


@pytest.mark.parametrize("query", ["all", "split", "nodes"])
def test_clustering_equals_the_reference(trained, query):
    ds, m, S = trained
    n = len(S)
    nodes = np.random.default_rng(1).integers(0, n, 50).astype(np.int32)
    rows, kw = {"all": (range(n), {}), "split": (np.flatnonzero(np.asarray(ds["split"]) == 3).tolist(), dict(split=3)),
                "nodes": (nodes.tolist(), dict(nodes=nodes))}[query]
    t2, deg, tot, _ = R.rows(S, rows)
    got = m.clustering(**kw)
    assert np.array_equal(got["t2"], t2) and np.array_equal(got["deg"], deg) and got["totals"].tolist() == tot and got["rows"] == len(t2)
    assert (got["triangles"], got["transitivity"], got["avg_clustering"]) == R.metrics(tot)
    want_c = [t / (d * (d - 1)) if d >= 2 else 0.0 for t, d in zip(t2, deg)]
    assert np.array_equal(got["clustering"], np.asarray(want_c, np.float64))
    assert "t2" not in m.clustering(per_node=False, **kw)


def test_link_overlap_equals_the_reference(trained):
    ds, m, S = trained
    n, rng = len(S), np.random.default_rng(2)
    src, dst = rng.integers(0, n, 400).astype(np.int32), rng.integers(0, n, 400).astype(np.int32)
    dst[:20] = src[:20]
    deg = [len(s) for s in S]
    got = m.link_overlap(src, dst)
    cn, un, _, _ = R.pairs(S, src.tolist(), dst.tolist())
    assert np.array_equal(got["common"], cn)
    assert np.array_equal(got["jaccard"], [c / u if u else 0.0 for c, u in zip(cn, un)])
    assert np.array_equal(got["preferential_attachment"], [deg[a] * deg[b] for a, b in zip(src, dst)])
    for kind, f in (("adamic_adar", lambda d: 1.0 / np.log(d) if d >= 2 else 0.0), ("resource_allocation", lambda d: 1.0 / d if d >= 1 else 0.0)):
        ws = R.pairs(S, src.tolist(), dst.tolist(), R.weight_table(deg, kind))[2]
        assert np.array_equal(got[kind], np.asarray(ws, np.float64) / 2.0 ** 32), kind
        exact = np.array([sum(f(deg[w]) for w in S[a] & S[b]) for a, b in zip(src, dst)])
        assert np.all(np.abs(got[kind] - exact) <= np.asarray(cn) * 2.0 ** -33 + 1e-12), kind
    assert set(m.link_overlap(src, dst, weights=("adamic_adar",))) == {"common", "jaccard", "preferential_attachment", "adamic_adar"}
    with pytest.raises(Exception, match="weights"):
        m.link_overlap(src, dst, weights=("katz",))


def test_a_multilabel_model_takes_the_queries():
    ds = datagen.make_dataset("tiny-syn")
    y = np.zeros((ds["num_nodes"], ds["output_dim"]), bool)
    y[np.arange(ds["num_nodes"]), np.asarray(ds["label"])] = True
    m = M.HipGCNModel(ds, seed=1, hidden_dim=16, multilabel=y)
    S = R.sets(ds["g_indptr"], ds["g_indices"])
    assert m.clustering(per_node=False)["totals"].tolist() == R.rows(S)[2]
    assert np.array_equal(m.link_overlap([0, 1, 2], [3, 4, 2], weights=())["common"], R.pairs(S, [0, 1, 2], [3, 4, 2])[0])
    m.close()


def test_the_queries_between_epochs_change_nothing():
    ds = datagen.make_dataset("cora-syn")
    a = M.HipGCNModel(ds, seed=6, hidden_dim=16, dropout=0.5)
    b = M.HipGCNModel(ds, seed=6, hidden_dim=16, dropout=0.5)
    ta, tb = [a.run_epochs(3)], [b.run_epochs(3)]
    b.clustering(split=3)
    b.link_overlap([0, 1, 2], [3, 4, 5])
    ta.append(a.run_epochs(3)), tb.append(b.run_epochs(3))
    assert np.concatenate(ta).tobytes() == np.concatenate(tb).tobytes()
    a.close(), b.close()


def test_cli_triangles(tmp_path, trained):
    """gcn-hip tiny-syn with GCN_TRIANGLES: stdout gains one line behind the test line; the file holds clustering(split=3)"""
    ds, m, _ = trained
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "tiny-syn.gcnbin"))
    w, out = str(tmp_path / "w.gcnw"), str(tmp_path / "tri.txt")
    m.save_weights(w)
    env = dict(os.environ, GCN_SEED="3", GCN_LOAD_WEIGHTS=w, GCN_TRIANGLES=out)
    r = subprocess.run(["timeout", "-k", "10", "50", HIP, "tiny-syn", "-", "-", "16", "-", "0.5", "-", "-", "0"], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    want = m.clustering(split=3)
    lines = r.stdout.strip().splitlines()
    assert lines[-2].startswith("test_loss=")
    assert lines[-1] == "triangles=%d transitivity=%.6f avg_clustering=%.6f" % (want["triangles"], want["transitivity"], want["avg_clustering"])
    got = M.read_triangles(out)
    assert np.array_equal(got["node"], np.flatnonzero(np.asarray(ds["split"]) == 3))
    assert np.array_equal(got["deg"], want["deg"]) and np.array_equal(got["t2"], want["t2"]) and got["totals"].tolist() == want["totals"].tolist()
    assert np.array_equal(got["clustering"], want["clustering"]) and got["triangles"] == want["triangles"]
