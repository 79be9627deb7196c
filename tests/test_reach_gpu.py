"""The reach report on the GPU: the kernels of csrc/reach.hip through ops.py — every integer equal to the Python-integer reference
of tests/reach_ref.py, for every lane grouping and every batching of the level launches — then the model's label_distance(),
components() and reach_report() against the reference fed with the dataset and predict()'s output, no side effects on training,
refusals, and the command line (GCN_REACH)."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import irregular_inputs as II
from tests import reach_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")
GROUPS = [0, 4, 16, 64]
SYNCS = [1, 3, 64]


@pytest.fixture(scope="module")
def dev():
    from cuda_gcn_amd.ops import Device
    d = Device(0)
    yield d
    d.close()


def self_loops_only(n=200):
    return R.csr(n, [], [])


def two_sources_graph():
    """row 5 stores 9 before 2 and both are seeds: the first entry found is not the winner; row 6 stores 5 and 7, at distances 1 and
    1 with nearest 2 and 8: the lower seed wins through the later entry again; 300 filler rows push the work past one wave"""
    n = 320
    src = [5, 5, 6, 6, 7, 10, 10, 11]
    dst = [9, 2, 7, 5, 8, 6, 11, 6]
    return R.csr(n, src, dst)


GRAPHS = {"path": lambda: R.path_graph(300), "permuted path": lambda: R.path_graph(300, np.random.default_rng(3).permutation(300)),
          "star": lambda: R.star_graph(700, 5000), "irregular": II.gpu_graph, "sparse": lambda: R.random_mutual_graph(3000, 2100, 11),
          "denser": lambda: R.random_mutual_graph(3000, 4500, 12), "self loops": self_loops_only, "two sources": two_sources_graph}


def seed_lists(name, n):
    if name == "path":
        return {"one end": np.array([0], np.int32)}
    if name == "star":                                         # from a leaf: the hub's 5 000 entries are walked while it has no distance
        return {"a leaf": np.array([700], np.int32), "the hub": np.array([0], np.int32)}
    if name == "permuted path":
        return {"one end": np.random.default_rng(3).permutation(300)[:1].astype(np.int32)}
    if name == "two sources":
        return {"three": np.array([9, 2, 8], np.int32)}
    out = {"2 %": R.random_seeds(n, 0.02, 1), "33 %": R.random_seeds(n, 0.33, 2)}
    if name in ("sparse", "denser"):
        out = {"5 %": R.random_seeds(n, 0.05, 2)}
    if name == "irregular":
        rep = np.concatenate([out["2 %"], out["2 %"][:7], [-1, n, n + 100, -2 ** 31, 2 ** 31 - 1]]).astype(np.int32)
        out.update({"none": np.zeros(0, np.int32), "every row": np.arange(n, dtype=np.int32), "repeats and strays": rep})
    return out


@pytest.fixture(scope="module")
def graphs(dev):
    out = {}
    for name, make in GRAPHS.items():
        gp, gi = make()
        out[name] = (gp, gi, dev.graph(gp, gi))
    return out


_refs = {}


def ref_for(name, which, gp, gi, seeds):
    if (name, which) not in _refs:
        _refs[(name, which)] = R.hop_distance(gp, gi, seeds)
    return _refs[(name, which)]


def assert_traversal(got, want, what, nearest=True):
    for key in ("dist", "nearest") if nearest else ("dist",):
        assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), (what, key, np.flatnonzero(got[key] != want[key])[:10])
    assert got["levels"] == want["levels"] and got["skipped"] == want["skipped"], (what, got["levels"], want["levels"], got["skipped"])
    assert got["level_counts"].dtype == np.int64 and np.array_equal(got["level_counts"], want["level_counts"]), (what, got["level_counts"])


# ---- the traversal -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_hop_distance_equals_the_reference(dev, graphs, name):
    gp, gi, g = graphs[name]
    for which, seeds in seed_lists(name, gp.size - 1).items():
        want = ref_for(name, which, gp, gi, seeds)
        got = dev.hop_distance(g, seeds)
        assert_traversal(got, want, (name, which))
        assert_traversal(dev.hop_distance(g, seeds, nearest=False), want, (name, which, "no nearest"), nearest=False)
        again = dev.hop_distance(g, seeds)
        assert all(again[k].tobytes() == got[k].tobytes() for k in ("dist", "nearest", "level_counts"))
        n = gp.size - 1
        assert got["level_counts"].sum() + int((got["dist"] < 0).sum()) == n
        assert np.array_equal((got["dist"] < 0), (got["nearest"] < 0))
        reached = got["dist"] >= 0
        assert np.all(np.isin(got["nearest"][reached], seeds)) and np.all(got["dist"][got["nearest"][reached]] == 0)


def test_the_cases_are_what_they_are_meant_to_be(dev, graphs):
    gp, gi, g = graphs["path"]
    got = dev.hop_distance(g, [0])
    assert got["levels"] == 299 and np.array_equal(got["dist"], np.arange(300)) and np.all(got["level_counts"] == 1)
    gp, gi, g = graphs["irregular"]
    n = gp.size - 1
    lists = seed_lists("irregular", n)
    none = dev.hop_distance(g, lists["none"])
    assert none["levels"] == 0 and np.all(none["dist"] == -1) and np.all(none["nearest"] == -1) and none["level_counts"].tolist() == [0]
    every = dev.hop_distance(g, lists["every row"])
    assert every["levels"] == 0 and not every["dist"].any() and np.array_equal(every["nearest"], np.arange(n)) and every["level_counts"].tolist() == [n]
    strays = dev.hop_distance(g, lists["repeats and strays"])
    assert strays["skipped"] == 5 and strays["level_counts"][0] == 30
    assert_traversal(strays, dict(ref_for("irregular", "2 %", gp, gi, lists["2 %"]), skipped=5), "strays")
    gp, gi, g = graphs["self loops"]
    alone = dev.hop_distance(g, [3, 150])
    assert alone["levels"] == 0 and alone["level_counts"].tolist() == [2] and np.flatnonzero(alone["dist"] == 0).tolist() == [3, 150]
    gp, gi, g = graphs["two sources"]
    two = dev.hop_distance(g, [9, 2, 8])
    assert two["dist"][[5, 6, 7, 10, 11]].tolist() == [1, 2, 1, 3, 3] and two["nearest"][[5, 6, 7, 10, 11]].tolist() == [2, 2, 8, 2, 2]
    assert gi[gp[5] + 1] == 9 and gi[gp[6] + 1] == 7             # the entry found first belongs to the higher seed


@pytest.mark.parametrize("name", ["path", "irregular", "denser"])
def test_a_hop_limit_truncates_the_full_answer(dev, graphs, name):
    gp, gi, g = graphs[name]
    which, seeds = next(iter(seed_lists(name, gp.size - 1).items()))
    full = ref_for(name, which, gp, gi, seeds)
    for max_hops in (1, 2, 3, 70, full["levels"], full["levels"] + 5):
        cut = dict(full, dist=np.where(full["dist"] > max_hops, -1, full["dist"]), nearest=np.where(full["dist"] > max_hops, -1, full["nearest"]),
                   levels=min(max_hops, full["levels"]), level_counts=full["level_counts"][:max_hops + 1])
        for sync in (1, 64):
            assert_traversal(dev.hop_distance(g, seeds, max_hops=max_hops, levels_per_sync=sync), cut, (name, max_hops, sync))
    short = dev.hop_distance(g, seeds, capacity=2)               # the capacity of the host array cuts the counts, nothing else
    assert np.array_equal(short["level_counts"], full["level_counts"][:2]) and short["levels"] == full["levels"]
    assert np.array_equal(short["dist"], full["dist"])
    assert dev.hop_distance(g, seeds, capacity=0)["levels"] == full["levels"]


@pytest.mark.parametrize("name", ["path", "permuted path", "star", "irregular", "sparse", "two sources"])
def test_every_lane_group_and_batching_gives_the_same_bits(dev, graphs, name):
    gp, gi, g = graphs[name]
    which, seeds = next(iter(seed_lists(name, gp.size - 1).items()))
    want = ref_for(name, which, gp, gi, seeds)
    for group in GROUPS:
        for sync in SYNCS:
            for nearest in (True, False):
                assert_traversal(dev.hop_distance(g, seeds, nearest=nearest, group=group, levels_per_sync=sync), want, (name, group, sync, nearest), nearest)


def test_propagate_reaches_exactly_the_rows_within_k_hops(dev, graphs):
    """an independent check through code that was there before: k iterations of propagate() from the indicator of the seeds, with
    positive coefficients and no clamp, leave a row non-zero exactly where 0 <= dist <= k"""
    from cuda_gcn_amd.model import HipGCNModel
    gp, gi, g = graphs["irregular"]
    n = gp.size - 1
    seeds = seed_lists("irregular", n)["2 %"]
    dist = dev.hop_distance(g, seeds, nearest=False)["dist"]
    rng = np.random.default_rng(1)
    ds = dict(name="reach", num_nodes=n, input_dim=4, output_dim=2, g_indptr=gp, g_indices=gi, f_indptr=np.arange(n + 1, dtype=np.int32),
              f_indices=rng.integers(0, 4, n).astype(np.int32), f_val=np.ones(n, np.float32), split=rng.integers(1, 4, n).astype(np.int32),
              label=rng.integers(0, 2, n).astype(np.int32))
    m = HipGCNModel(ds, seed=1, hidden_dim=8)
    y0 = np.zeros((n, 1), np.float32)
    y0[seeds] = 1.0
    for k in range(1, 6):
        y = m.propagate(y0, 0.5, k)
        assert np.all(y >= 0) and np.array_equal(y[:, 0] != 0, (dist >= 0) & (dist <= k)), k
    m.close()


# ---- the components ------------------------------------------------------------------------------------------------------------

def one_way_graph(n=500, seed=5):
    """every row but the first stores ONE entry, a lower row, and nobody stores it back: a random tree, one weak component"""
    rng = np.random.default_rng(seed)
    src = np.arange(1, n)
    return R.csr(n, src, (rng.random(n - 1) * src).astype(np.int64))


COMPONENT_GRAPHS = dict(GRAPHS, **{"long path": lambda: R.path_graph(4096, np.random.default_rng(7).permutation(4096)), "one way": one_way_graph})
COMPONENT_GRAPHS.pop("path")


@pytest.mark.parametrize("name", sorted(COMPONENT_GRAPHS))
def test_components_equal_the_reference(dev, graphs, name):
    gp, gi = COMPONENT_GRAPHS[name]()
    g = graphs[name][2] if name in graphs else dev.graph(gp, gi)
    n = gp.size - 1
    want = R.components(gp, gi)
    comp, rounds = dev.components(g)
    assert comp.dtype == np.int32 and np.array_equal(comp, want), (name, np.flatnonzero(comp != want)[:10])
    assert 1 <= rounds <= n, rounds
    print(f"components {name}: {np.unique(want).size} components of {n} rows in {rounds} rounds")
    again, _ = dev.components(g)
    assert again.tobytes() == comp.tobytes()
    if name == "self loops":
        assert np.array_equal(comp, np.arange(n)) and rounds == 1
    if name in ("long path", "one way", "irregular"):
        assert not comp.any()
    rng = np.random.default_rng(n)
    for mark in (None, (rng.random(n) < 0.05).astype(np.int32), np.where(rng.random(n) < 0.5, -3, 0).astype(np.int32)):
        size, marked, totals = dev.component_counts(comp, mark)
        ws, wm, wt = R.component_counts(want, mark)
        assert np.array_equal(size, ws) and np.array_equal(marked, wm) and totals.dtype == np.int64 and np.array_equal(totals, wt), (name, totals, wt)
        assert totals[0] == n and totals[1] == np.unique(want).size and totals[5] == (0 if mark is None else np.count_nonzero(mark))
        twice = dev.component_counts(comp, mark)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(twice, (size, marked, totals)))


def test_component_counts_pass_over_labels_outside_the_graph(dev):
    comp = np.array([0, 0, 9, -1, 4, 4, 4, 2 ** 31 - 1], np.int32)
    mark = np.array([1, 0, 1, 1, 0, 5, 0, 1], np.int32)
    got = dev.component_counts(comp, mark)
    want = R.component_counts(comp, mark)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and got[2].tolist() == [5, 2, 3, 0, 0, 2]
    empty = dev.component_counts(np.zeros(0, np.int32))
    assert empty[2].tolist() == [0] * 6


# ---- the strata ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hops", [1, 2, 8, 32])
def test_distance_strata_equal_the_reference(dev, hops):
    rng = np.random.default_rng(hops)
    n_rows, C = 777, 7
    dist = rng.integers(-1, hops + 3, n_rows).astype(np.int32)
    dist[:6] = [hops - 1, hops, hops + 1, -1, 0, 2 ** 31 - 1]   # the boundaries of the buckets
    truth = np.where(rng.random(n_rows) < 0.15, rng.choice([-1, C, -7, 2 ** 31 - 1], n_rows), rng.integers(0, C, n_rows)).astype(np.int32)
    pred = np.where(rng.random(n_rows) < 0.6, truth, rng.integers(0, C, n_rows)).astype(np.int32)
    nearest = np.where(dist < 0, -1, rng.integers(0, n_rows, n_rows)).astype(np.int32)
    nearest[10:14] = [n_rows, -5, 2 ** 31 - 1, 10]
    lists = (None, rng.integers(0, n_rows, 400).astype(np.int32), np.where(rng.random(500) < 0.1, [-1, n_rows][hops % 2], rng.integers(0, n_rows, 500)).astype(np.int32),
             np.zeros(0, np.int32), np.tile(np.arange(n_rows, dtype=np.int32), 100))      # the last: more positions than one pass of the grid
    for rows in lists:
        for kw in (dict(nearest=nearest, pred=pred), dict(pred=pred), dict(nearest=nearest), dict()):
            want, want_unl = R.strata(dist, truth, C, hops, rows=rows, **kw)
            got, unl = dev.distance_strata(dist, truth, C, hops, rows=rows, **kw)
            assert got.dtype == np.int64 and np.array_equal(got, want) and unl == want_unl, (hops, None if rows is None else rows.size, sorted(kw))
            if "pred" not in kw:
                assert not got[:, 2].any()
            if "nearest" not in kw:
                assert not got[:, 3].any()
        used = np.arange(n_rows) if rows is None else rows
        ok = (used >= 0) & (used < n_rows)
        assert got[:, 0].sum() == ok.sum() and got[:, 1].sum() + unl == ok.sum()
    again, _ = dev.distance_strata(dist, truth, C, hops, nearest=nearest, pred=pred)
    first, _ = dev.distance_strata(dist, truth, C, hops, nearest=nearest, pred=pred)
    assert again.tobytes() == first.tobytes()


def test_ops_refusals(dev, graphs):
    from cuda_gcn_amd.ops import GcnHipError
    import ctypes as C
    gp, gi, g = graphs["self loops"]
    n = gp.size - 1
    lib = dev.lib
    out = dev.buf(np.full(2 * n + 600, 123, np.int32))
    dist, near, scratch = out.ptr, out.ptr + 4 * n, out.ptr + 8 * n
    seeds = dev.buf(np.zeros(4, np.int32))
    levels, skipped = C.c_int(-5), C.c_int64(-5)
    counts = np.full(8, -5, np.int64)
    rect = dev.graph(np.array([0, 1, 2], np.int32), np.array([0, 2], np.int32), n_cols=3, col_deg=np.ones(3, np.int32))

    def refused(rc, text):
        assert rc == -1 and text in lib.gcnhip_last_error().decode(), (rc, lib.gcnhip_last_error())

    def hop(ctx=dev.ctx, gh=g.h, s=seeds.ptr, ns=4, mh=0, d=dist, sc=scratch, lv=C.byref(levels), lc=counts.ctypes.data, cap=8, sk=C.byref(skipped), ex=None):
        args = (ctx, gh, s, ns, mh, d, near, sc, lv, lc, cap, sk)
        return lib.gcnhip_hop_distance_ex(*args, *ex) if ex else lib.gcnhip_hop_distance(*args)
    for kw in (dict(ctx=None), dict(gh=None), dict(s=None), dict(ns=-1), dict(mh=-1), dict(d=None), dict(sc=None), dict(lv=None), dict(lc=None), dict(cap=-1),
               dict(sk=None)):
        refused(hop(**kw), "gcnhip_hop_distance: invalid argument")
    refused(hop(gh=rect.h), "gcnhip_hop_distance: a square adjacency object")
    for group in (1, 8, 32, -4):
        refused(hop(ex=(group, 8)), "the lane group is")
    for sync in (0, 65, -1):
        refused(hop(ex=(0, sync)), "1 <= levels_per_sync <= 64")
    rounds = C.c_int(-5)
    for args in ((None, g.h, dist, scratch, C.byref(rounds)), (dev.ctx, None, dist, scratch, C.byref(rounds)), (dev.ctx, g.h, None, scratch, C.byref(rounds)),
                 (dev.ctx, g.h, dist, None, C.byref(rounds)), (dev.ctx, g.h, dist, scratch, None)):
        refused(lib.gcnhip_components(*args), "gcnhip_components: invalid argument")
    refused(lib.gcnhip_components(dev.ctx, rect.h, dist, scratch, C.byref(rounds)), "gcnhip_components: a square adjacency object")
    for args in ((None, dist, None, n, dist, near, scratch), (dev.ctx, None, None, n, dist, near, scratch), (dev.ctx, dist, None, -1, dist, near, scratch),
                 (dev.ctx, dist, None, n, None, near, scratch), (dev.ctx, dist, None, n, dist, None, scratch), (dev.ctx, dist, None, n, dist, near, None)):
        refused(lib.gcnhip_component_counts(*args), "gcnhip_component_counts: invalid argument")

    def strata(ctx=dev.ctx, d=dist, t=near, nr=n, nn=n, c=3, hops=4, st=scratch, un=scratch + 8 * 150):
        return lib.gcnhip_distance_strata(ctx, d, None, None, t, nr, None, nn, c, hops, st, un)
    for kw in (dict(ctx=None), dict(d=None), dict(t=None), dict(nr=-1), dict(nn=-1), dict(st=None), dict(un=None)):
        refused(strata(**kw), "gcnhip_distance_strata: invalid argument")
    for hops in (0, 33, -1):
        refused(strata(hops=hops), "1 <= hops <= 32")
    refused(strata(c=0), "num_classes >= 1")
    with pytest.raises(GcnHipError, match="1 <= hops <= 32"):
        dev.distance_strata(np.zeros(3), np.zeros(3), 3, 33)
    with pytest.raises(GcnHipError, match="the lane group is"):
        dev.hop_distance(g, [0], group=5)
    assert np.all(out.download() == 123)                       # no refusal launched or wrote anything
    assert levels.value == -5 and skipped.value == -5 and rounds.value == -5 and np.all(counts == -5)


# ---- the model ---------------------------------------------------------------------------------------------------------------

def isolated_dataset():
    """tiny-syn with every 5th node cut off: its row keeps the self loop alone and no row lists it"""
    ds = dict(datagen.make_dataset("tiny-syn"))
    gp, gi = np.asarray(ds["g_indptr"]), np.asarray(ds["g_indices"])
    n = ds["num_nodes"]
    cut = np.zeros(n, bool)
    cut[::5] = True
    rows = []
    for v in range(n):
        r = gi[gp[v]:gp[v + 1]]
        rows.append(np.array([v], np.int32) if cut[v] else r[~cut[r] | (r == v)])
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum([r.size for r in rows])
    ds.update(g_indptr=indptr.astype(np.int32), g_indices=np.concatenate(rows).astype(np.int32))
    return ds


@pytest.fixture(scope="module")
def trained():
    from cuda_gcn_amd.model import HipGCNModel
    out = {}
    for name, ds, kw in (("irregular", II.irregular_dataset(), dict(hidden_dim=16, dropout=0.5)),
                         ("planted", datagen.planted_communities(n_comm=8, size=128, p_in=0.5, feats=8), dict(hidden_dim=16, dropout=0.0)),
                         ("isolated", isolated_dataset(), dict(hidden_dim=16, dropout=0.5))):
        m = HipGCNModel(ds, seed=5, **kw)
        m.run_epochs(6, want_trace=False)
        pred = m.predict(nodes=np.arange(ds["num_nodes"], dtype=np.int32))[0]
        out[name] = (ds, m, pred, {})
    yield out
    for _, m, _, _ in out.values():
        m.close()


def model_reference(entry, sources):
    """the traversal, the components and their counts of a dataset's graph from one source list, computed once"""
    ds, _, _, cache = entry
    key = tuple(np.asarray(sources).tolist())
    if key not in cache:
        gp, gi = ds["g_indptr"], ds["g_indices"]
        n = ds["num_nodes"]
        d = R.hop_distance(gp, gi, sources)
        if "comp" not in cache:
            cache["comp"] = R.components(gp, gi)
        mark = np.zeros(n, np.int32)
        mark[np.asarray(sources, np.int64)] = 1
        cache[key] = (d, cache["comp"], R.component_counts(cache["comp"], mark))
    return cache[key]


def check_reach(entry, hops, split=3, nodes=None, sources=(1,), source_nodes=None, predicted=True):
    ds, m, pred, _ = entry
    n = ds["num_nodes"]
    split_of = np.asarray(ds["split"])
    src = np.flatnonzero(np.isin(split_of, sources)) if source_nodes is None else np.asarray(source_nodes)
    rows = np.asarray(nodes) if nodes is not None else (np.flatnonzero(split_of == split) if split else np.arange(n))
    d, comp, (size, marked, totals) = model_reference(entry, src)
    want, unl = R.strata(d["dist"], ds["label"], ds["output_dim"], hops, nearest=d["nearest"], pred=pred if predicted else None, rows=rows)
    got = m.reach_report(split=split, nodes=nodes, sources=sources, source_nodes=source_nodes, hops=hops, predicted=predicted, per_node=True)
    assert got["strata"].dtype == np.int64 and np.array_equal(got["strata"], want), (got["strata"], want)
    assert np.array_equal(got["totals"], totals) and np.array_equal(got["level_counts"], d["level_counts"]) and got["levels"] == d["levels"]
    assert np.array_equal(got["dist"], d["dist"][rows]) and np.array_equal(got["nearest"], d["nearest"][rows]) and np.array_equal(got["component"], comp[rows])
    assert (got["rows"], got["unlabelled"], got["sources"]) == (rows.size, unl, np.unique(src).size)
    assert (got["n_components"], got["largest"], got["unmarked_components"], got["unmarked_nodes"]) == tuple(int(x) for x in totals[1:5])
    layers = min(2, hops - 1)
    R.assert_metrics_equal(got, R.metrics(want, hops, layers))
    assert got["unreachable"] == int((d["dist"][rows] < 0).sum())
    inside = (d["dist"][rows] >= 0) & (d["dist"][rows] <= layers)
    assert got["inside_receptive_field"]["rows"] == int(inside.sum()) and got["outside_receptive_field"]["rows"] == rows.size - int(inside.sum())
    if predicted:
        lab = np.asarray(ds["label"])[rows]
        assert got["inside_receptive_field"]["correct"] == int((pred[rows] == lab)[inside].sum()) and got["all"]["correct"] == int((pred[rows] == lab).sum())
    return got


@pytest.mark.parametrize("name", ["irregular", "planted", "isolated"])
def test_reach_report_equals_the_reference(trained, name):
    entry = trained[name]
    ds, m, pred, _ = entry
    n = ds["num_nodes"]
    full = check_reach(entry, 8)
    check_reach(entry, 1, split=2)
    check_reach(entry, 32, split=None, sources=(1, 2))
    check_reach(entry, 3, predicted=False)
    rng = np.random.default_rng(4)
    hub = int(np.argmax(np.diff(ds["g_indptr"])))
    q = np.concatenate([[hub, 5, 5, hub], rng.integers(0, n, 50)]).astype(np.int32)
    few = check_reach(entry, 2, nodes=q, source_nodes=[7, 7, 3, n - 1])
    assert few["rows"] == q.size and few["sources"] == 3
    none = m.reach_report(nodes=np.zeros(0, np.int32), source_nodes=[], hops=3)
    assert none["rows"] == 0 and not none["strata"].any() and none["levels"] == 0 and none["sources"] == 0 and none["unreachable_share"] == 0.0
    assert none["unmarked_components"] == none["n_components"] == full["n_components"] and none["unmarked_nodes"] == n
    if name == "isolated":                                     # a cut-off test node is its own component and no label reaches it
        cut = np.flatnonzero((np.arange(n) % 5 == 0) & (np.asarray(ds["split"]) == 3))
        assert cut.size and full["unreachable"] >= cut.size and full["unmarked_components"] >= cut.size and full["by_distance"][9]["rows"] == full["unreachable"]
    again = m.reach_report(per_node=True)
    assert all(again[k].tobytes() == full[k].tobytes() for k in ("strata", "totals", "level_counts", "dist", "nearest", "component"))


@pytest.mark.parametrize("name", ["irregular", "isolated"])
def test_label_distance_and_components_on_queries_and_splits(trained, name):
    entry = trained[name]
    ds, m, _, _ = entry
    n = ds["num_nodes"]
    split_of = np.asarray(ds["split"])
    train = np.flatnonzero(split_of == 1)
    d, comp, (size, marked, totals) = model_reference(entry, train)
    q = np.array([n - 1, 0, 0, 17, 3], np.int32)
    for kw, rows in ((dict(), np.arange(n)), (dict(split=3), np.flatnonzero(split_of == 3)), (dict(nodes=q), q)):
        got = m.label_distance(nearest=True, **kw)
        assert np.array_equal(got["dist"], d["dist"][rows]) and np.array_equal(got["nearest"], d["nearest"][rows]) and got["rows"] == rows.size
        assert got["levels"] == d["levels"] and np.array_equal(got["level_counts"], d["level_counts"]) and got["sources"] == train.size
        assert got["unreachable"] == int((d["dist"][rows] < 0).sum())
        slim = m.label_distance(**kw)
        assert slim["nearest"] is None and np.array_equal(slim["dist"], got["dist"])
        cut = m.label_distance(max_hops=1, nearest=True, **kw)
        assert np.array_equal(cut["dist"], np.where(d["dist"][rows] > 1, -1, d["dist"][rows])) and cut["levels"] == min(1, d["levels"])
        c = m.components(**kw)
        assert np.array_equal(c["component"], comp[rows]) and np.array_equal(c["size"], size[comp[rows]]) and np.array_equal(c["totals"], totals)
        assert (c["n_components"], c["largest"], c["unmarked_components"], c["unmarked_nodes"], c["marked_rows"]) == tuple(int(x) for x in totals[1:])
        assert 1 <= c["rounds"] <= n and c["rows"] == rows.size
    other = m.label_distance(source_nodes=[5, 900 % n, 5], nearest=True)
    want = R.hop_distance(ds["g_indptr"], ds["g_indices"], [5, 900 % n])
    assert np.array_equal(other["dist"], want["dist"]) and np.array_equal(other["nearest"], want["nearest"]) and other["sources"] == 2
    marked_by_nodes = m.components(marked_nodes=[5])
    assert marked_by_nodes["marked_rows"] == 1 and marked_by_nodes["unmarked_components"] == marked_by_nodes["n_components"] - 1


def test_a_multilabel_model_takes_the_queries_without_a_forward():
    from cuda_gcn_amd.model import HipGCNModel, GcnHostError
    ds = datagen.make_dataset("tiny-syn")
    n, C = ds["num_nodes"], ds["output_dim"]
    y = np.zeros((n, C), bool)
    y[np.arange(n), np.asarray(ds["label"])] = True
    m = HipGCNModel(ds, seed=1, hidden_dim=16, multilabel=y)
    train = np.flatnonzero(np.asarray(ds["split"]) == 1)
    d = R.hop_distance(ds["g_indptr"], ds["g_indices"], train)
    assert np.array_equal(m.label_distance()["dist"], d["dist"])
    assert np.array_equal(m.components()["component"], R.components(ds["g_indptr"], ds["g_indices"]))
    rep = m.reach_report(predicted=False, hops=4)
    rows = np.flatnonzero(np.asarray(ds["split"]) == 3)
    assert np.array_equal(rep["strata"], R.strata(d["dist"], ds["label"], C, 4, nearest=d["nearest"], rows=rows)[0])
    with pytest.raises(GcnHostError, match="reach_report: predicted=True takes a single-label model"):
        m.reach_report()
    m.close()


def test_the_queries_between_epochs_change_nothing():
    from cuda_gcn_amd import model as M
    ds = datagen.make_dataset("cora-syn")
    a = M.HipGCNModel(ds, seed=6, hidden_dim=16, dropout=0.5)
    b = M.HipGCNModel(ds, seed=6, hidden_dim=16, dropout=0.5)
    ta, tb = [a.run_epochs(3)], [b.run_epochs(3)]
    before = b.predict(logp=True)
    b.reach_report(per_node=True)
    b.reach_report(split=2, hops=3, predicted=False)
    b.label_distance(nodes=[1, 2, 3], nearest=True)
    b.components(split=3)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, b.predict(logp=True)))
    ta.append(a.run_epochs(2))
    tb.append(b.run_epochs(2))
    ta, tb = np.concatenate(ta), np.concatenate(tb)
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32)), (ta, tb)
    for v in (2, 5):
        assert a.var(v).tobytes() == b.var(v).tobytes(), v
    assert a.eval(3) == b.eval(3) and a.var(6).tobytes() == b.var(6).tobytes() and a.var(3).tobytes() == b.var(3).tobytes()
    a.close()
    b.close()


def test_model_refusals():
    from cuda_gcn_amd.model import HipGCNModel, GcnHostError, _ck
    from tests.mr_threads import ThreadWorld
    ds = datagen.make_dataset("tiny-syn")
    n = ds["num_nodes"]
    m = HipGCNModel(ds, seed=1, hidden_dim=16)
    for hops in (0, 33, 2.5, "eight", True):
        with pytest.raises(GcnHostError, match="reach_report: hops must be"):
            m.reach_report(hops=hops)
    for max_hops in (-1, 1.5, True):
        with pytest.raises(GcnHostError, match="label_distance: max_hops must be"):
            m.label_distance(max_hops=max_hops)
    for call in (m.reach_report, m.label_distance, m.components):
        with pytest.raises(GcnHostError, match="split is 1"):
            call(split=4)
        with pytest.raises(GcnHostError, match="not a node of the dataset"):
            call(nodes=[0, n])
        with pytest.raises(GcnHostError, match="not a node of the dataset"):
            call(nodes=[-1])
    for call in (m.label_distance, m.components):
        with pytest.raises(GcnHostError, match="give a split or a node query"):
            call(split=1, nodes=[0])
    with pytest.raises(GcnHostError, match="not a node of the dataset"):
        m.label_distance(source_nodes=[0, n])
    with pytest.raises(GcnHostError, match="not a node of the dataset"):
        m.reach_report(source_nodes=[-1])
    with pytest.raises(GcnHostError, match="not a node of the dataset"):
        m.components(marked_nodes=[n + 3])
    for bad in ((), (0,), (4,), (1, True), "train"):
        with pytest.raises(GcnHostError, match="the source splits are"):
            m.label_distance(sources=bad)
    # the host's own refusals, past the Python checks
    out = np.zeros(64, np.int64)
    o = out.ctypes.data

    def reach(hops=8, split=3, mask=2):
        return m.lib.gcnhost_model_reach(m.h, split, None, 0, mask, None, 0, hops, 1, n, None, None, None, o, o + 8 * 40, None, 0, o + 8 * 48)

    def distance(max_hops=0, split=0, mask=2, ns=0):
        return m.lib.gcnhost_model_label_distance(m.h, mask, None, ns, split, None, 0, max_hops, n, None, None, None, 0, o)
    for hops in (0, 33):
        with pytest.raises(GcnHostError, match=r"reach: hops must be in 1\.\.32"):
            _ck(m.lib, reach(hops=hops), "call")
    with pytest.raises(GcnHostError, match="reach: invalid argument \\(split"):
        _ck(m.lib, reach(split=-1), "call")
    with pytest.raises(GcnHostError, match="reach: invalid argument \\(the source splits"):
        _ck(m.lib, reach(mask=1), "call")
    with pytest.raises(GcnHostError, match="label_distance: max_hops must be at least 0"):
        _ck(m.lib, distance(max_hops=-1), "call")
    with pytest.raises(GcnHostError, match="label_distance: invalid argument"):
        _ck(m.lib, distance(mask=0, ns=3), "call")
    with pytest.raises(GcnHostError, match="components: invalid argument \\(split"):
        _ck(m.lib, m.lib.gcnhost_model_components(m.h, 7, None, 0, 2, None, 0, n, None, None, o, o + 8 * 8), "call")
    assert not out.any()
    m.close()
    tw = ThreadWorld(2)
    seen, errors = [None, None], []

    def body(rank):
        try:
            ag, ar = tw.callbacks(rank)
            r = HipGCNModel(ds, seed=4, device=0, rank=rank, world=2, host_allgather=ag, host_allreduce=ar, hidden_dim=16, dropout=0.5)
            got = []
            for call in (lambda: r.reach_report(), lambda: r.label_distance(), lambda: r.components()):
                try:
                    call()
                    got.append("no error")
                except GcnHostError as e:
                    got.append(str(e))
            seen[rank] = got
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
    assert all("reach: one rank only" in s[0] and "label_distance: one rank only" in s[1] and "components: one rank only" in s[2] for s in seen), seen


# ---- the command line -------------------------------------------------------------------------------------------------------

def test_cli_reach(tmp_path):
    """gcn-hip cora-syn with GCN_REACH: stdout keeps its lines and gains one; the file's integers are the Python call's on the same
    weights (handed over through a weights file, 0 epochs); without the variable stdout is what it was"""
    from cuda_gcn_amd.model import HipGCNModel, read_reach_report, reach_metrics
    ds = datagen.make_dataset("cora-syn")
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "cora-syn.gcnbin"))
    m = HipGCNModel(ds, seed=3, hidden_dim=16, dropout=0.5)
    m.run_epochs(6, want_trace=False)
    w = str(tmp_path / "w.gcnw")
    m.save_weights(w)
    want = m.reach_report(split=3, hops=5)
    m.close()
    args = ["cora-syn", "-", "-", "16", "-", "0.5", "-", "-", "0"]
    out = str(tmp_path / "r.txt")
    base = dict(os.environ, GCN_SEED="3", GCN_LOAD_WEIGHTS=w)
    base.pop("GCN_REACH", None)
    env = dict(base, GCN_REACH=out, GCN_REACH_HOPS="5")
    r = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-2].startswith("test_loss=") and lines[-1].startswith("reach_sources=")
    fields = dict(p.split("=") for p in lines[-1].split())
    assert list(fields) == ["reach_sources", "reach_levels", "reach_unreachable", "reach_outside_two_hops", "acc_inside_two_hops", "acc_outside_two_hops",
                            "nearest_label_acc", "components", "largest_component", "unseeded_components", "unseeded_nodes"]
    ints = dict(reach_sources=want["sources"], reach_levels=want["levels"], reach_unreachable=want["unreachable"],
                reach_outside_two_hops=want["outside_receptive_field"]["rows"], components=want["n_components"], largest_component=want["largest"],
                unseeded_components=want["unmarked_components"], unseeded_nodes=want["unmarked_nodes"])
    for name, value in ints.items():
        assert int(fields[name]) == value, (name, fields, value)
    floats = dict(acc_inside_two_hops=want["inside_receptive_field"]["accuracy"], acc_outside_two_hops=want["outside_receptive_field"]["accuracy"],
                  nearest_label_acc=want["nearest_label_accuracy"])
    for name, value in floats.items():
        assert abs(float(fields[name]) - value) <= 5e-7, (name, fields, value)
    back = read_reach_report(out)
    assert back["hops"] == 5 and back["layers"] == 2 and np.array_equal(back["strata"], want["strata"]) and np.array_equal(back["totals"], want["totals"])
    assert np.array_equal(back["level_counts"], want["level_counts"]) and back["sources"] == want["sources"] and back["unlabelled"] == want["unlabelled"]
    assert reach_metrics(back["strata"], 5, back["layers"])["by_distance"] == want["by_distance"]
    text = open(out).read().splitlines()
    at = next(i for i, l in enumerate(text) if l.startswith("# by_distance:"))
    for b, row in enumerate(want["by_distance"]):
        f = text[at + 1 + b].split()
        assert int(f[1]) == b and int(f[2]) == row["rows"] and int(f[4]) == row["correct"] and abs(float(f[6]) - row["accuracy"]) <= 5e-10
    plain = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=base, capture_output=True, text=True)
    clock = lambda text: re.sub(r"time=\S+", "time=", text)     # the wall-clock fields differ from run to run
    assert plain.returncode == 0 and clock(plain.stdout).splitlines() == clock(r.stdout).splitlines()[:-1]
    for extra, text in ((dict(GCN_GPUS="2"), "GCN_REACH runs on one GPU"), (dict(GCN_REACH_HOPS="33"), "GCN_REACH needs GCN_REACH_HOPS in 1..32")):
        bad = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=dict(env, **extra), capture_output=True, text=True)
        assert bad.returncode != 0 and text in bad.stderr, bad.stderr[-500:]
