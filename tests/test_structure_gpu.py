"""The structure report on the GPU: the kernels of csrc/structure.hip through ops.py — every integer equal to the Python-integer
reference of tests/structure_ref.py, for every lane grouping and flush interval — then the model's neighbor_agreement() and
structure_report() against the reference fed with the dataset and predict()'s output, against evaluate(), across row schedules, no
side effects on training, refusals, and the command line (GCN_STRUCTURE)."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import irregular_inputs as II
from tests import structure_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")
CLASSES = [1, 2, 5, 41, 64]
GROUPS = [0, 4, 16, 64]
PER_ROW = ("deg", "same", "known")
INT_KEYS = PER_ROW + ("mix", "class_rows", "totals")


@pytest.fixture(scope="module")
def dev():
    from cuda_gcn_amd.ops import Device
    d = Device(0)
    yield d
    d.close()


def handmade_graph():
    """rows of the stored lengths at which the walk changes path (no entry, the self loop alone, below / at / above one vector step
    of a 16-lane group and of a wave, a row longer than 64 x 64 entries), rows that hold the self entry twice, a row without it"""
    rng = np.random.default_rng(77)
    lengths = [0, 1, 2, 63, 64, 65, 127, 128, 129, 4097, 3, 7, 6, 0, 5, 1025, 257, 4, 9, 30]
    n = len(lengths)
    rows = []
    for v, k in enumerate(lengths):
        r = rng.integers(0, n, k)
        if k:
            r[0] = v                                           # the loader's self loop first
        if v in (10, 11, 6, 9):                                # the self entry twice (also in the middle of the long row)
            r[k // 2 + 1] = v
        if v == 14:
            r[r == v] = (v + 1) % n                            # a row without its self loop
        rows.append(r)
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum(lengths)
    return indptr.astype(np.int32), np.concatenate(rows).astype(np.int32)


def symmetric_graph(n=257, seed=3):
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n, 4 * n), rng.integers(0, n, 4 * n)
    keep = a != b
    a, b = a[keep], b[keep]
    src = np.concatenate([np.arange(n), a, b])                 # self loops, each pair both ways (repeated pairs twice both ways)
    dst = np.concatenate([np.arange(n), b, a])
    order = np.argsort(src, kind="stable")
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum(np.bincount(src, minlength=n))
    return indptr.astype(np.int32), dst[order].astype(np.int32)


GRAPHS = {"irregular": lambda: II.irregular_graph(np.random.default_rng(II.SEED_GRAPH), 300, hub_len=2500, rep_len=300), "handmade": handmade_graph}


@pytest.fixture(scope="module")
def graphs(dev):
    out = {}
    for name, make in GRAPHS.items():
        gp, gi = make()
        out[name] = (gp, gi, dev.graph(gp, gi))
    return out


def lists_for(gp):
    n = gp.size - 1
    rng = np.random.default_rng(n)
    hub = int(np.argmax(np.diff(gp)))
    rep = np.concatenate([[hub, -1, 3, 3, n, hub], rng.integers(0, n, 40), [n + 5, -7, 0]]).astype(np.int32)
    return {"all": None, "empty": np.zeros(0, np.int32), "repeats": rep}


_refs = {}


def ref_for(name, gp, gi, C, which, rows):
    key = (name, C, which)
    if key not in _refs:
        lab = R.random_labels(np.random.default_rng(1000 + C), gp.size - 1, C)
        _refs[key] = (lab, R.agreement(gp, gi, lab, C, rows))
    return _refs[key]


def assert_equal(got, want, keys=INT_KEYS, what=None):
    for key in keys:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (what, key, got[key], want[key])
    assert got["skipped"] == want["skipped"], (what, got["skipped"], want["skipped"])


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_agreement_equals_the_reference(dev, graphs, name, C):
    gp, gi, g = graphs[name]
    for which, rows in lists_for(gp).items():
        lab, want = ref_for(name, gp, gi, C, which, rows)
        if which == "repeats":
            assert want["skipped"] == 4
        for group in GROUPS:
            got = dev.nbr_agreement(g, lab, C, rows=rows, group=group)
            assert_equal(got, want, what=(which, group))
            # the identities of the definitions
            t = got["totals"]
            assert got["mix"].sum() == t[4] and np.trace(got["mix"]) == t[5] and got["class_rows"].sum() == t[1]
            assert t[0] == (gp.size - 1 if rows is None else rows.size) - got["skipped"]
        again = dev.nbr_agreement(g, lab, C, rows=rows)
        first = dev.nbr_agreement(g, lab, C, rows=rows)
        assert all(again[k].tobytes() == first[k].tobytes() for k in INT_KEYS)


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_a_small_flush_interval_changes_nothing(dev, graphs, name):
    """every wave empties the LDS histogram after 64 (or 1) walked entries: the path that the default interval of 2^26 entries
    reaches only on graphs of billions of stored entries"""
    gp, gi, g = graphs[name]
    rows = lists_for(gp)["repeats"]
    for C in (5, 64):
        lab, want = ref_for(name, gp, gi, C, "repeats", rows)
        for group in GROUPS:
            for every in (1, 64, 5000):
                assert_equal(dev.nbr_agreement(g, lab, C, rows=rows, group=group, flush_every=every), want, what=(C, group, every))


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_null_outputs_leave_the_others_unchanged(dev, graphs, name):
    gp, gi, g = graphs[name]
    rows = lists_for(gp)["repeats"]
    lab, want = ref_for(name, gp, gi, 5, "repeats", rows)
    for group in (0, 4):
        for leave_out in ("mix",) + PER_ROW:
            keep = tuple(k for k in ("mix",) + PER_ROW if k != leave_out)
            got = dev.nbr_agreement(g, lab, 5, rows=rows, want=keep, group=group)
            assert got[leave_out] is None
            assert_equal(got, want, keys=keep + ("class_rows", "totals"), what=leave_out)
        none = dev.nbr_agreement(g, lab, 5, rows=rows, want=(), group=group)
        assert_equal(none, want, keys=("class_rows", "totals"))


def test_many_positions_take_the_grid_stride_loop(dev, graphs):
    """more positions than one pass of the largest grid holds (two workgroups per CU x 256 positions with 4-lane groups, 131 072 on
    256 CUs): a list of 150 000 positions over the short rows, whose expected counts are sums of the rows' own"""
    gp, gi, g = graphs["irregular"]
    n, C = gp.size - 1, 5
    lab = R.random_labels(np.random.default_rng(8), n, C)
    short = np.flatnonzero(np.diff(gp) <= 12)
    rows = short[np.random.default_rng(9).integers(0, short.size, 150000)].astype(np.int32)
    per = {int(v): R.agreement(gp, gi, lab, C, [v]) for v in np.unique(rows)}
    want = dict(skipped=0)
    for k in PER_ROW:
        want[k] = np.array([per[int(v)][k][0] for v in rows], np.int32)
    times = np.bincount(rows, minlength=n)
    for k in ("mix", "class_rows", "totals"):                  # Python integers; 150 000 ratios of at most 2^32 stay below 2^63
        want[k] = np.asarray(sum(int(times[v]) * per[v][k].astype(object) for v in per), np.int64)
    for group in GROUPS:
        assert_equal(dev.nbr_agreement(g, lab, C, rows=rows, group=group), want, what=group)
    # without a list, more positions than rows: the positions past the last row are skipped
    got = dev.nbr_agreement(g, lab, C, n=n + 9)
    full = R.agreement(gp, gi, lab, C, None, n + 9)
    assert full["skipped"] == 9
    assert_equal(got, full)


def test_mix_is_symmetric_on_a_symmetric_graph(dev):
    gp, gi = symmetric_graph()
    g = dev.graph(gp, gi)
    for C in (2, 41):
        lab = R.random_labels(np.random.default_rng(C), gp.size - 1, C)
        got = dev.nbr_agreement(g, lab, C)
        assert_equal(got, R.agreement(gp, gi, lab, C))
        assert np.array_equal(got["mix"], got["mix"].T) and got["mix"].sum() > 0 and np.trace(got["mix"]) < got["mix"].sum()


# ---- strata -----------------------------------------------------------------------------------------------------------------

def boundary_rows(bins):
    """(deg, same, known): degrees at powers of two and one below, same . bins divisible by known, same == known, known == 0"""
    deg, same, known = [], [], []
    for d in [0, 1, 2, 3, 4, 7, 8, 15, 16, 1023, 1024, 1025, 2 ** 30 - 1, 2 ** 30, 2 ** 31 - 1]:
        for k in sorted({0, 1, 2, 3, bins, 2 * bins, 7 * bins + 1, min(d, 997)}):
            if k > d:
                continue
            ss = {0, k, k // 2, max(k - 1, 0)} | {k * a // bins for a in range(bins + 1)} | {min(k, k * a // bins + 1) for a in range(bins)}
            for s in sorted(ss):
                deg.append(d); known.append(k); same.append(s)
    return np.array(deg, np.int32), np.array(same, np.int32), np.array(known, np.int32)


@pytest.mark.parametrize("bins", [1, 2, 10, 32])
def test_strata_equal_the_reference(dev, bins):
    deg, same, known = boundary_rows(bins)
    n, C = deg.size, 7
    rng = np.random.default_rng(bins)
    n_truth = n + 11
    truth = R.random_labels(rng, n_truth, C)
    pred = np.where(rng.random(n_truth) < 0.6, truth, rng.integers(0, C, n_truth)).astype(np.int32)
    for rows in (None, rng.integers(0, n_truth, n).astype(np.int32), np.where(rng.random(n) < 0.1, [-1, n_truth][bins % 2], rng.integers(0, n_truth, n)).astype(np.int32)):
        want, want_unl = R.strata(deg, same, known, pred, truth, C, bins, rows)
        got, unl = dev.strata_counts(deg, same, known, pred, truth, C, bins, rows=rows)
        assert got.dtype == np.int64 and np.array_equal(got, want) and unl == want_unl, (bins, rows is None)
        used = np.arange(n) if rows is None else rows
        ok = (used >= 0) & (used < n_truth)
        labelled = int(((truth[used[ok]] >= 0) & (truth[used[ok]] < C)).sum())
        assert got[:, :, 0].sum() == labelled and labelled + unl == int(ok.sum()) and np.all(got[:, :, 1] <= got[:, :, 0])
        again, _ = dev.strata_counts(deg, same, known, pred, truth, C, bins, rows=rows)
        assert again.tobytes() == got.tobytes()
    empty, unl = dev.strata_counts(deg[:0], same[:0], known[:0], pred, truth, C, bins)
    assert not empty.any() and unl == 0
    # more positions than one pass of the grid holds (256 workgroups x 256): the list repeated, the counts multiplied
    reps = 70000 // n + 1
    big = np.tile(np.arange(n), reps)
    want, want_unl = R.strata(deg, same, known, pred, truth, C, bins)
    got, unl = dev.strata_counts(deg[big], same[big], known[big], pred, truth, C, bins, rows=big)
    assert np.array_equal(got, reps * want) and unl == reps * want_unl


def test_ops_refusals(dev, graphs):
    from cuda_gcn_amd.ops import GcnHipError
    gp, gi, g = graphs["handmade"]
    n = gp.size - 1
    lab = np.zeros(n, np.int32)
    lib = dev.lib
    out = dev.buf(np.full(64 * 64 + 64 + 8 + 1, 123, np.int64))
    lb = dev.buf(lab)
    mix, rows_c, totals, skipped = out.ptr, out.ptr + 8 * 4096, out.ptr + 8 * (4096 + 64), out.ptr + 8 * (4096 + 64 + 8)

    def refused(rc, text):
        assert rc == -1 and text in lib.gcnhip_last_error().decode(), (rc, lib.gcnhip_last_error())
    for C in (0, 65, -3):
        refused(lib.gcnhip_nbr_agreement(dev.ctx, g.h, lb.ptr, C, None, n, None, None, None, mix, rows_c, totals, skipped), "1 <= num_classes <= 64")
    refused(lib.gcnhip_nbr_agreement(dev.ctx, g.h, lb.ptr, 3, None, -1, None, None, None, mix, rows_c, totals, skipped), "gcnhip_nbr_agreement: invalid argument")
    for args in ((None, g.h, lb.ptr, mix, rows_c, totals, skipped), (dev.ctx, None, lb.ptr, mix, rows_c, totals, skipped),
                 (dev.ctx, g.h, None, mix, rows_c, totals, skipped), (dev.ctx, g.h, lb.ptr, mix, None, totals, skipped),
                 (dev.ctx, g.h, lb.ptr, mix, rows_c, None, skipped), (dev.ctx, g.h, lb.ptr, mix, rows_c, totals, None)):
        refused(lib.gcnhip_nbr_agreement(args[0], args[1], args[2], 3, None, n, None, None, None, *args[3:]), "gcnhip_nbr_agreement: invalid argument")
    refused(lib.gcnhip_nbr_agreement_ex(dev.ctx, g.h, lb.ptr, 3, None, n, None, None, None, mix, rows_c, totals, skipped, 8, 0), "the lane group is")
    refused(lib.gcnhip_nbr_agreement_ex(dev.ctx, g.h, lb.ptr, 3, None, n, None, None, None, mix, rows_c, totals, skipped, 0, (1 << 26) + 1), "the flush interval")
    with pytest.raises(GcnHipError, match="1 <= num_classes <= 64"):
        dev.nbr_agreement(g, lab, 65)
    z = dev.buf(np.zeros(8, np.int32))
    for bins in (0, 33, -1):
        refused(lib.gcnhip_strata_counts(dev.ctx, z.ptr, z.ptr, z.ptr, z.ptr, z.ptr, 8, None, 8, 3, bins, mix, skipped), "1 <= bins <= 32")
    for C in (0, 65):
        refused(lib.gcnhip_strata_counts(dev.ctx, z.ptr, z.ptr, z.ptr, z.ptr, z.ptr, 8, None, 8, C, 4, mix, skipped), "1 <= num_classes <= 64")
    refused(lib.gcnhip_strata_counts(dev.ctx, z.ptr, z.ptr, z.ptr, z.ptr, z.ptr, 8, None, -1, 3, 4, mix, skipped), "gcnhip_strata_counts: invalid argument")
    refused(lib.gcnhip_strata_counts(dev.ctx, None, z.ptr, z.ptr, z.ptr, z.ptr, 8, None, 8, 3, 4, mix, skipped), "gcnhip_strata_counts: invalid argument")
    refused(lib.gcnhip_strata_counts(dev.ctx, z.ptr, z.ptr, z.ptr, None, z.ptr, 8, None, 8, 3, 4, mix, skipped), "gcnhip_strata_counts: invalid argument")
    refused(lib.gcnhip_strata_counts(dev.ctx, z.ptr, z.ptr, z.ptr, z.ptr, z.ptr, 8, None, 8, 3, 4, None, skipped), "gcnhip_strata_counts: invalid argument")
    with pytest.raises(GcnHipError, match="1 <= bins <= 32"):
        dev.strata_counts(np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3), 3, 33)
    assert np.all(out.download() == 123)                       # no refusal launched or zeroed anything


# ---- the model --------------------------------------------------------------------------------------------------------------

def reference_report(ds, pred, rows, bins):
    """structure_report() from the definitions: the dataset's arrays, predict()'s classes (dataset order), the listed rows"""
    C = ds["output_dim"]
    label = np.asarray(ds["label"])
    t = R.agreement(ds["g_indptr"], ds["g_indices"], label, C, rows)
    p = R.agreement(ds["g_indptr"], ds["g_indices"], pred, C, rows)
    s, unl = R.strata(t["deg"], t["same"], t["known"], pred, label, C, bins, np.arange(ds["num_nodes"]) if rows is None else rows)
    return t, p, s, unl


def check_report(m, ds, bins, split=None, nodes=None):
    from cuda_gcn_amd.model import structure_metrics
    n = ds["num_nodes"]
    pred = m.predict(nodes=np.arange(n, dtype=np.int32))[0]
    rows = np.flatnonzero(np.asarray(ds["split"]) == split) if split else (None if nodes is None else np.asarray(nodes))
    t, p, s, unl = reference_report(ds, pred, rows, bins)
    got = m.structure_report(split=split, nodes=nodes, bins=bins, per_node=True)
    for side, want in (("truth", t), ("pred", p)):
        for key in ("mix", "class_rows", "totals"):
            assert got[side][key].dtype == np.int64 and np.array_equal(got[side][key], want[key]), (side, key, got[side][key], want[key])
        R.assert_metrics_close(got[side], R.metrics(want["mix"], want["class_rows"], want["totals"]))
    for key in PER_ROW:
        assert got[key].dtype == np.int32 and np.array_equal(got[key], t[key]), key
    assert np.array_equal(got["strata"], s) and got["unlabelled"] == unl and got["rows"] == t["deg"].size and got["bins"] == bins
    tables = R.metrics(t["mix"], t["class_rows"], t["totals"], s)
    R.assert_metrics_close(dict(by_degree=got["by_degree"], by_agreement=got["by_agreement"]), dict(by_degree=tables["by_degree"], by_agreement=tables["by_agreement"]))
    assert got["pred_vs_truth_edge_homophily"] == got["pred"]["edge_homophily"] - got["truth"]["edge_homophily"]
    assert got["truth"]["edge_homophily"] == structure_metrics(t["mix"], t["class_rows"])["edge_homophily"]
    # against evaluate() on the same rows: the strata hold its matrix's rows, and its trace of them is right
    ev = m.evaluate(split=split, nodes=nodes)
    assert s[:, :, 1].sum() == np.trace(ev["confusion"]) and s[:, :, 0].sum() == ev["rows"] and unl == ev["unlabelled"]
    return got


@pytest.fixture(scope="module")
def trained():
    from cuda_gcn_amd.model import HipGCNModel
    out = {}
    for name, ds, kw in (("tiny", datagen.make_dataset("tiny-syn"), dict(hidden_dim=16, dropout=0.5)),
                         ("irregular", II.irregular_dataset(), dict(hidden_dim=16, dropout=0.5)),
                         ("planted", datagen.planted_communities(n_comm=8, size=128, p_in=0.5, feats=8), dict(hidden_dim=16, dropout=0.0))):
        m = HipGCNModel(ds, seed=5, **kw)
        m.run_epochs(6, want_trace=False)
        out[name] = (ds, m)
    yield out
    for _, m in out.values():
        m.close()


@pytest.mark.parametrize("name", ["tiny", "irregular", "planted"])
def test_structure_report_equals_the_reference(trained, name):
    ds, m = trained[name]
    n = ds["num_nodes"]
    full = check_report(m, ds, 10)
    assert full["rows"] == n
    if name != "irregular":                                    # the generator's own number, from the GPU's counts
        assert full["truth"]["edge_homophily"] == datagen.edge_homophily(ds)
    check_report(m, ds, 4, split=3)
    check_report(m, ds, 32, split=1)
    rng = np.random.default_rng(4)
    hub = int(np.argmax(np.diff(ds["g_indptr"])))
    q = np.concatenate([[hub, 5, 5, hub], rng.integers(0, n, 50)]).astype(np.int32)
    rep = check_report(m, ds, 1, nodes=q)
    assert rep["rows"] == q.size
    none = m.structure_report(nodes=np.zeros(0, np.int32), bins=3)
    assert none["rows"] == 0 and not none["strata"].any() and none["truth"]["edge_homophily"] == 0.0 and none["truth"]["totals"].sum() == 0
    # without the forward: the truth's side alone
    half = m.structure_report(split=3, predicted=False)
    assert half["pred"] is None and half["strata"] is None and half["by_degree"] is None and half["pred_vs_truth_edge_homophily"] is None
    assert np.array_equal(half["truth"]["mix"], m.structure_report(split=3)["truth"]["mix"])
    again = m.structure_report(bins=10)
    assert again["strata"].tobytes() == full["strata"].tobytes() and again["pred"]["mix"].tobytes() == full["pred"]["mix"].tobytes()


def test_the_row_schedule_does_not_matter(trained):
    from cuda_gcn_amd.model import HipGCNModel, NO_ROW_GROUPS
    ds, m = trained["planted"]
    plain = HipGCNModel(ds, seed=5, hidden_dim=16, dropout=0.0, flags=NO_ROW_GROUPS)
    plain.set_weights(m.var(2), m.var(5))
    a, b = m.structure_report(per_node=True), plain.structure_report(per_node=True)
    for side in ("truth", "pred"):
        for key in ("mix", "class_rows", "totals"):
            assert np.array_equal(a[side][key], b[side][key]), (side, key)
    assert np.array_equal(a["strata"], b["strata"]) and all(np.array_equal(a[k], b[k]) for k in PER_ROW)
    plain.close()


def test_neighbor_agreement_takes_any_labelling(trained):
    ds, m = trained["planted"]
    n, k = ds["num_nodes"], 6
    assign = m.cluster(k=k, iters=10, seed=2)["assign"]
    got = m.neighbor_agreement(assign, k, per_node=True)
    want = R.agreement(ds["g_indptr"], ds["g_indices"], assign, k)
    for key in INT_KEYS:
        assert np.array_equal(got[key], want[key]), key
    R.assert_metrics_close(got, R.metrics(want["mix"], want["class_rows"], want["totals"]))
    assert abs(got["node_homophily"] - R.node_homophily_float(want["same"], want["known"])) <= 2.0 ** -32
    # the dataset's labels with some hidden, int64, over a split and over a query with repeats
    lab = np.asarray(ds["label"]).astype(np.int64)
    lab[::7] = -1
    lab[3::11] = 2 ** 40
    test_nodes = np.flatnonzero(np.asarray(ds["split"]) == 3)
    for kw, rows in ((dict(split=3), test_nodes), (dict(nodes=[9, 9, 0, n - 1]), np.array([9, 9, 0, n - 1]))):
        got = m.neighbor_agreement(lab, per_node=True, **kw)
        want = R.agreement(ds["g_indptr"], ds["g_indices"], np.clip(lab, -1, 2 ** 31 - 1), ds["output_dim"], rows)
        assert all(np.array_equal(got[key], want[key]) for key in INT_KEYS) and got["rows"] == rows.size
    slim = m.neighbor_agreement(lab, split=3)
    assert "deg" not in slim and np.array_equal(slim["mix"], R.agreement(ds["g_indptr"], ds["g_indices"], np.clip(lab, -1, 2 ** 31 - 1), ds["output_dim"], test_nodes)["mix"])


def test_a_multilabel_model_takes_neighbor_agreement():
    from cuda_gcn_amd.model import HipGCNModel, GcnHostError
    ds = datagen.make_dataset("tiny-syn")
    n, C = ds["num_nodes"], ds["output_dim"]
    y = np.zeros((n, C), bool)
    y[np.arange(n), np.asarray(ds["label"])] = True
    m = HipGCNModel(ds, seed=1, hidden_dim=16, multilabel=y)
    got = m.neighbor_agreement(ds["label"], C)
    want = R.agreement(ds["g_indptr"], ds["g_indices"], ds["label"], C)
    assert all(np.array_equal(got[key], want[key]) for key in ("mix", "class_rows", "totals"))
    with pytest.raises(GcnHostError, match="structure_report: predicted=True takes a single-label model"):
        m.structure_report()
    m.close()


def test_a_report_between_epochs_changes_nothing():
    from cuda_gcn_amd import model as M
    ds = datagen.make_dataset("cora-syn")
    a = M.HipGCNModel(ds, seed=6, hidden_dim=16, dropout=0.5)
    b = M.HipGCNModel(ds, seed=6, hidden_dim=16, dropout=0.5)
    ta, tb = [a.run_epochs(3)], [b.run_epochs(3)]
    before = b.predict(logp=True)
    b.structure_report(per_node=True)
    b.structure_report(split=2, bins=3)
    b.neighbor_agreement(ds["label"], nodes=[1, 2, 3])
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
    n, C = ds["num_nodes"], ds["output_dim"]
    m = HipGCNModel(ds, seed=1, hidden_dim=16)
    for bins in (0, 33, 2.5, "ten", True):
        with pytest.raises(GcnHostError, match="structure_report: bins must be"):
            m.structure_report(bins=bins)
    for call in (m.structure_report, lambda **kw: m.neighbor_agreement(ds["label"], **kw)):
        with pytest.raises(GcnHostError, match="give a split or a node query"):
            call(split=1, nodes=[0])
        with pytest.raises(GcnHostError, match="split is 1"):
            call(split=4)
        with pytest.raises(GcnHostError, match="not a node of the dataset"):
            call(nodes=[0, n])
        with pytest.raises(GcnHostError, match="not a node of the dataset"):
            call(nodes=[-1])
    for c in (0, 65, 2.0, "x"):
        with pytest.raises(GcnHostError, match="neighbor_agreement: num_classes must be"):
            m.neighbor_agreement(ds["label"], c)
    for lab in (np.zeros(n - 1, np.int32), np.zeros((n, 1), np.int32), np.zeros(n, np.float32)):
        with pytest.raises(GcnHostError, match="neighbor_agreement: labels must be"):
            m.neighbor_agreement(lab)
    # the host's own refusals, past the Python checks
    lab = np.zeros(n, np.int32)
    out = np.zeros(64 * 64 + 64 + 8 + 3, np.int64)
    o = out.ctypes.data

    def agree(n_labels=n, c=C, split=0):
        return m.lib.gcnhost_model_neighbor_agreement(m.h, lab.ctypes.data, n_labels, c, split, None, 0, n, None, None, None, o, o + 8 * 4096, o + 8 * 4160, o + 8 * 4168)

    def report(bins=10, split=0):
        return m.lib.gcnhost_model_structure(m.h, split, None, 0, bins, 1, n, None, None, None, o, o + 8 * 4096, o + 8 * 4160, o, o + 8 * 4096, o + 8 * 4160, None,
                                             o + 8 * 4168)
    with pytest.raises(GcnHostError, match=r"neighbor_agreement: \d+ labels for \d+ nodes"):
        _ck(m.lib, agree(n_labels=n - 1), "call")
    for c in (0, 65):
        with pytest.raises(GcnHostError, match="neighbor_agreement: 1 to 64 classes"):
            _ck(m.lib, agree(c=c), "call")
    with pytest.raises(GcnHostError, match="neighbor_agreement: invalid argument \\(split"):
        _ck(m.lib, agree(split=4), "call")
    for bins in (0, 33):
        with pytest.raises(GcnHostError, match=r"structure: bins must be in 1\.\.32"):
            _ck(m.lib, report(bins=bins), "call")
    with pytest.raises(GcnHostError, match="structure: invalid argument \\(split"):
        _ck(m.lib, report(split=-1), "call")
    assert not out.any()
    m.close()
    tw = ThreadWorld(2)
    seen, errors = [None, None], []

    def body(rank):
        try:
            ag, ar = tw.callbacks(rank)
            r = HipGCNModel(ds, seed=4, device=0, rank=rank, world=2, host_allgather=ag, host_allreduce=ar, hidden_dim=16, dropout=0.5)
            got = []
            for call in (lambda: r.structure_report(), lambda: r.neighbor_agreement(ds["label"])):
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
    assert all("structure: one rank only" in s[0] and "neighbor_agreement: one rank only" in s[1] for s in seen), seen


# ---- the command line -------------------------------------------------------------------------------------------------------

def test_cli_structure(tmp_path):
    """gcn-hip cora-syn with GCN_STRUCTURE: stdout keeps its lines and gains one; the file's integers are the Python call's on the
    same weights (handed over through a weights file, 0 epochs); without the variable stdout is what it was"""
    from cuda_gcn_amd.model import HipGCNModel, read_structure_report, structure_metrics
    ds = datagen.make_dataset("cora-syn")
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "cora-syn.gcnbin"))
    m = HipGCNModel(ds, seed=3, hidden_dim=16, dropout=0.5)
    m.run_epochs(6, want_trace=False)
    w = str(tmp_path / "w.gcnw")
    m.save_weights(w)
    want = m.structure_report(split=3, bins=7)
    m.close()
    args = ["cora-syn", "-", "-", "16", "-", "0.5", "-", "-", "0"]
    out = str(tmp_path / "s.txt")
    base = dict(os.environ, GCN_SEED="3", GCN_LOAD_WEIGHTS=w)
    base.pop("GCN_STRUCTURE", None)
    env = dict(base, GCN_STRUCTURE=out, GCN_STRUCTURE_BINS="7")
    r = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-2].startswith("test_loss=") and lines[-1].startswith("edge_homophily=")
    fields = dict(p.split("=") for p in lines[-1].split())
    assert list(fields) == ["edge_homophily", "node_homophily", "adjusted_homophily", "class_insensitive_homophily", "pred_edge_homophily"]
    for name in ("edge_homophily", "node_homophily", "adjusted_homophily", "class_insensitive_homophily"):
        assert abs(float(fields[name]) - want["truth"][name]) <= 5e-7, (name, fields, want["truth"][name])
    assert abs(float(fields["pred_edge_homophily"]) - want["pred"]["edge_homophily"]) <= 5e-7
    back = read_structure_report(out)
    assert back["num_classes"] == ds["output_dim"] and back["bins"] == 7 and np.array_equal(back["strata"], want["strata"])
    for side in ("truth", "pred"):
        for key in ("mix", "class_rows", "totals"):
            assert np.array_equal(back[side][key], want[side][key]), (side, key)
    tables = structure_metrics(back["truth"]["mix"], back["truth"]["class_rows"], back["truth"]["totals"], back["strata"])
    assert tables["by_degree"] == want["by_degree"] and tables["by_agreement"] == want["by_agreement"]
    text = open(out).read().splitlines()
    at = text.index("# by_agreement: bucket lo hi rows correct accuracy")
    for b, row in enumerate(want["by_agreement"]):
        f = text[at + 1 + b].split()
        assert int(f[1]) == b and int(f[4]) == row["rows"] and int(f[5]) == row["correct"] and abs(float(f[6]) - row["accuracy"]) <= 5e-10
    plain = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=base, capture_output=True, text=True)
    clock = lambda text: re.sub(r"time=\S+", "time=", text)     # the wall-clock fields differ from run to run
    assert plain.returncode == 0 and clock(plain.stdout).splitlines() == clock(r.stdout).splitlines()[:-1]
    for extra, text in ((dict(GCN_GPUS="2"), "GCN_STRUCTURE runs on one GPU"), (dict(GCN_STRUCTURE_BINS="33"), "GCN_STRUCTURE needs GCN_STRUCTURE_BINS in 1..32")):
        bad = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=dict(env, **extra), capture_output=True, text=True)
        assert bad.returncode != 0 and text in bad.stderr, bad.stderr[-500:]
