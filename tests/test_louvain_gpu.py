"""Louvain communities on the GPU (csrc/louvain.hip through ops.py and the model) against the Python integers of
tests/louvain_ref.py: every integer is asserted EQUAL, on every lane group, cut and table size."""
import os
import subprocess

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from cuda_gcn_amd import model as M
from tests import louvain_ref as L
from tests import overlap_ref as R
from tests.irregular_inputs import gpu_graph
from tests.test_kmeans_gpu import dev                                                   # noqa: F401 (the Device fixture)
from tests.test_overlap_gpu import handmade, planted

pytestmark = pytest.mark.gpu
HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cuda_gcn_amd", "bin", "gcn-hip")
# the defaults, the three lane groups, a cut that leaves row 4097 (and every row above 8 entries) to a workgroup, a table of 256
# slots: rows above 128 entries take the global-memory table, coarse rows with more room the dense array
VARIANTS = [dict(), dict(group=4), dict(group=16), dict(group=64), dict(group=64, wg_cut=8), dict(table=256)]
CLIQUE = (np.arange(0, 8 * 7 + 1, 7), np.concatenate([np.delete(np.arange(8), v) for v in range(8)]), 8)
EDGELESS = (np.array([0, 0, 1, 1, 3], np.int64), np.array([1, 3, 9]), 10)       # only the self entry and entries outside the rows


@pytest.fixture(scope="module")
def graphs(dev):
    out = {}
    for name, (indptr, indices, n_cols) in dict(handmade=handmade(), irregular=gpu_graph() + (1500,), planted=planted(), clique=CLIQUE,
                                                edgeless=EDGELESS).items():
        indptr, indices = np.asarray(indptr, np.int32), np.asarray(indices, np.int32)
        g = dev.graph(indptr, indices, n_cols=n_cols, col_deg=np.ones(n_cols, np.int32))
        rows, self_w = L.level0(R.sets(indptr, indices))
        comm, tot, num, sweeps, moved = L.level(rows, self_w)
        out[name] = dict(indptr=indptr, indices=indices, g=g, lv=dev.louvain_level0(g, dev.overlap_sets(g)), rows=rows, self_w=self_w,
                         level=(comm, tot, num, sweeps, moved), coarse=L.coarsen(rows, self_w, comm))
    return out


def level_equals(got, want, n):
    comm, tot, num, sweeps, moved = want
    assert (got["num"], got["sweeps"], got["moved"]) == (num, sweeps, moved)
    assert np.array_equal(got["comm"].download()[:n], comm) and np.array_equal(got["tot"].download()[:n], tot)


@pytest.mark.parametrize("variant", VARIANTS, ids=str)
@pytest.mark.parametrize("name", ["handmade", "irregular", "planted"])
def test_one_level_equals_the_reference_on_every_path(dev, graphs, name, variant):
    case = graphs[name]
    got = dev.louvain_level(case["lv"], **variant)
    level_equals(got, case["level"], case["lv"]["n"])
    assert got["m2"] == sum(len(r) for r in case["rows"]) and case["level"][4]
    if name == "handmade" and "wg_cut" in variant:
        assert got["wg_rows"] + got["long_rows"] == sum(len(r) > 8 for r in case["rows"]) >= 8 and got["wg_rows"] > 0
    if "table" in variant:
        assert got["long_rows"] == sum(len(r) > 128 for r in case["rows"]) and (got["long_rows"] >= 2 or name != "handmade")
    short = dev.louvain_level(case["lv"], max_sweeps=3, **variant)
    level_equals(short, L.level(case["rows"], case["self_w"], max_sweeps=3), case["lv"]["n"])


@pytest.mark.parametrize("table", [0, 256])
@pytest.mark.parametrize("name", ["handmade", "irregular", "planted"])
def test_coarsening_equals_the_reference_and_the_next_level_too(dev, graphs, name, table):
    case = graphs[name]
    label, rows, self_w, ptr = case["coarse"]
    got_label, lv = dev.louvain_coarsen(case["lv"], dev.louvain_level(case["lv"])["comm"], table=table)
    nc = len(rows)
    if name == "handmade":                                         # with table=256 the hub's coarse row takes the dense array
        assert max(np.diff(ptr)) > 128 > min(np.diff(ptr))
    assert lv["n"] == nc and lv["entries"] == ptr[-1] and np.array_equal(got_label.download()[:len(label)], label)
    got_ptr, got_len, idx, w = lv["ptr"].download(), lv["len"].download(), lv["idx"].download(), lv["w"].download()
    assert np.array_equal(got_ptr[:nc + 1], ptr) and np.array_equal(got_len[:nc], [len(r) for r in rows])
    assert np.array_equal(lv["self_w"].download()[:nc], self_w)
    for C, row in enumerate(rows):
        span = slice(ptr[C], ptr[C] + len(row))
        assert np.array_equal(idx[span], [u for u, _ in row]) and np.array_equal(w[span], [x for _, x in row]), C
    for variant in (dict(), dict(group=64, wg_cut=8), dict(table=256)):            # weights, self weights and ragged rows in the move
        level_equals(dev.louvain_level(lv, **variant), L.level(rows, self_w), nc)


def test_an_edgeless_graph_and_a_clique(dev, graphs):
    got = dev.louvain_level(graphs["edgeless"]["lv"])
    assert (got["m2"], got["num"], got["sweeps"], got["moved"]) == (0, 0, 0, False) and np.array_equal(got["comm"].download()[:4], np.arange(4))
    case = graphs["clique"]
    got = dev.louvain_level(case["lv"])
    level_equals(got, case["level"], 8)
    label, lv = dev.louvain_coarsen(case["lv"], got["comm"])
    assert lv["n"] == 1 and not label.download()[:8].any() and got["num"] == 0 and lv["self_w"].download()[0] == 56


def test_ops_refusals(dev, graphs):
    lv = graphs["planted"]["lv"]
    for kw, text in ((dict(group=8), "lane group"), (dict(wg_cut=-1), "cut"), (dict(table=300), "power of two"), (dict(table=1 << 20), "power of two")):
        with pytest.raises(Exception, match=text):
            dev.louvain_level(lv, **kw)


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("dataset", ["tiny-syn", "cora-syn"])
def test_communities_equal_the_chained_calls_and_the_reference(dev, dataset):
    ds = datagen.make_dataset(dataset)
    m = M.HipGCNModel(ds, seed=3, hidden_dim=16, dropout=0.5)
    got = m.communities(levels=True)
    again = m.communities(report=False)                            # on warm buffers
    m.close()
    S = R.sets(ds["g_indptr"], ds["g_indices"])
    labels, records, num, m2 = L.louvain(S)
    assert np.array_equal(got["labels"], labels) and got["labels"].tobytes() == again["labels"].tobytes()
    assert (got["numerator"], got["m2"], got["communities"]) == (num, m2, len(set(labels)))
    assert got["level_records"] == [(v, s, M.modularity_from_sums(x, m2)) for v, s, x in records] and got["modularity"] == num / m2 ** 2
    assert len(got["level_labels"]) == len(records) - 1 and np.array_equal(got["level_labels"][-1], labels)
    # the same run from the op-level calls
    indptr, indices = np.asarray(ds["g_indptr"], np.int32), np.asarray(ds["g_indices"], np.int32)
    g = dev.graph(indptr, indices, n_cols=len(S), col_deg=np.ones(len(S), np.int32))
    lv, chained, n = dev.louvain_level0(g, dev.overlap_sets(g)), dev.buf(np.arange(len(S), dtype=np.int32)), []
    while True:
        one = dev.louvain_level(lv)
        n.append((lv["n"], one["sweeps"], one["num"]))
        if not one["moved"]:
            break
        label, nxt = dev.louvain_coarsen(lv, one["comm"])
        dev.louvain_compose(chained, len(S), label, lv["n"])
        lv = nxt
    assert n == records and chained.download().tobytes() == got["labels"].tobytes()
    if "contingency" in got:
        want = np.zeros_like(got["contingency"])
        known = np.asarray(ds["label"]) >= 0
        np.add.at(want, (np.asarray(labels)[known], np.asarray(ds["label"])[known]), 1)
        assert np.array_equal(got["contingency"], want) and got["ari"] == M.cluster_report(want)["ari"]


def test_communities_of_an_edgeless_model_and_its_refusals():
    ds = dict(datagen.make_dataset("tiny-syn"))
    n = ds["num_nodes"]
    ds["g_indptr"], ds["g_indices"] = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)     # only the self entries
    m = M.HipGCNModel(ds, seed=1, hidden_dim=16)
    got = m.communities(levels=True)
    assert np.array_equal(got["labels"], np.arange(n)) and (got["communities"], got["modularity"], got["numerator"], got["m2"]) == (n, 0.0, 0, 0)
    assert got["level_records"] == [(n, 0, 0.0)] and got["level_labels"] == [] and got["contingency"].sum(1).tolist() == [1] * n
    one = m.communities(max_levels=1, max_sweeps=0)
    assert one["communities"] == n
    with pytest.raises(M.GcnHostError, match="max_levels"):
        m.communities(max_levels=0)
    m.close()


def test_cli_communities(tmp_path):
    """gcn-hip tiny-syn with GCN_COMMUNITIES: stdout gains one line behind the test line; the file holds communities()"""
    ds = datagen.make_dataset("tiny-syn")
    m = M.HipGCNModel(ds, seed=3, hidden_dim=16, dropout=0.5)
    want = m.communities(report=False)
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "tiny-syn.gcnbin"))
    w, out = str(tmp_path / "w.gcnw"), str(tmp_path / "comm.txt")
    m.save_weights(w)
    m.close()
    env = dict(os.environ, GCN_SEED="3", GCN_LOAD_WEIGHTS=w, GCN_COMMUNITIES=out)
    r = subprocess.run(["timeout", "-k", "10", "50", HIP, "tiny-syn", "-", "-", "16", "-", "0.5", "-", "-", "0"], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-2].startswith("test_loss=")
    assert lines[-1] == "communities=%d modularity=%.6f louvain_levels=%d louvain_sweeps=%d" % (
        want["communities"], want["modularity"], len(want["level_records"]), sum(rec[1] for rec in want["level_records"]))
    got = M.read_communities(out)
    assert np.array_equal(got["node"], np.arange(ds["num_nodes"])) and got["labels"].tobytes() == want["labels"].tobytes()
    assert (got["communities"], got["modularity"], got["numerator"], got["m2"], got["levels"]) == (
        want["communities"], want["modularity"], want["numerator"], want["m2"], len(want["level_records"]))
