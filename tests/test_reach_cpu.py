"""What of the reach report needs no GPU: the Python-integer reference of tests/reach_ref.py against scipy, the measures of
host/reach.h on hand-made tables, the report file, host/reach.cpp under ASan / UBSan in a program of its own, the properties the
generated graphs of the GPU tests are chosen for, refusals and the symbols."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import breadth_first_order, connected_components

from cuda_gcn_amd import _lib
from cuda_gcn_amd.model import GcnHostError, reach_metrics, read_reach_report, write_reach_report
from tests import irregular_inputs as II
from tests import reach_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scipy_matrix(gp, gi):
    n = gp.size - 1
    return sp.csr_matrix((np.ones(gi.size, np.int8), gi.astype(np.int64), gp.astype(np.int64)), shape=(n, n))


def canonical(labels):
    """scipy's component numbers -> the smallest row of each component"""
    lowest = np.full(labels.max() + 1, labels.size, np.int64)
    np.minimum.at(lowest, labels, np.arange(labels.size))
    return lowest[labels].astype(np.int32)


GRAPHS = {"irregular": II.gpu_graph, "sparse": lambda: R.random_mutual_graph(3000, 2100, 11), "denser": lambda: R.random_mutual_graph(3000, 4500, 12),
          "path": lambda: R.path_graph(300), "permuted path": lambda: R.path_graph(300, np.random.default_rng(3).permutation(300)),
          "star": lambda: R.star_graph(700, 5000)}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_reference_components_are_scipys(name):
    gp, gi = GRAPHS[name]()
    k, labels = connected_components(scipy_matrix(gp, gi), directed=True, connection="weak")
    comp = R.components(gp, gi)
    assert np.array_equal(comp, canonical(labels))
    size, marked, totals = R.component_counts(comp)
    assert totals[1] == k and totals[0] == gp.size - 1 and totals[2] == np.bincount(labels).max() and size.sum() == gp.size - 1
    assert totals[3] == k and totals[4] == gp.size - 1 and totals[5] == 0 and not marked.any()


@pytest.mark.parametrize("name", ["sparse", "denser", "path", "star"])
def test_reference_distance_is_scipys_on_a_symmetric_graph(name):
    """on a graph that stores every pair both ways the pull traversal is an ordinary breadth-first search: scipy's from one seed"""
    gp, gi = GRAPHS[name]()
    n = gp.size - 1
    seed = int(np.argmax(np.diff(gp)))
    got = R.hop_distance(gp, gi, [seed])
    order, pred = breadth_first_order(scipy_matrix(gp, gi), seed, directed=False)
    want = np.full(n, -1, np.int64)
    want[seed] = 0
    for v in order[1:]:
        want[v] = want[pred[v]] + 1
    assert np.array_equal(got["dist"], want) and got["levels"] == want.max()
    assert np.array_equal(got["level_counts"], np.bincount(want[want >= 0]))
    assert np.all(got["nearest"][want >= 0] == seed) and np.all(got["nearest"][want < 0] == -1)


def test_the_generated_graphs_have_the_properties_they_are_chosen_for():
    gp, gi = II.gpu_graph()
    n = gp.size - 1
    assert n == 1500 and int(np.diff(gp).max()) == 2500
    seeds = R.random_seeds(n, 0.02, 1)
    d = R.hop_distance(gp, gi, seeds)
    comp = R.components(gp, gi)
    # the direction of the traversal and the symmetry of the components are both exercised: one weak component, yet rows that no
    # seed reaches along stored rows (they store their self loop only, and are listed by others)
    assert d["levels"] == 5 and 40 <= int((d["dist"] < 0).sum()) <= 160 and np.all(comp == 0)
    assert d["level_counts"].sum() + (d["dist"] < 0).sum() == n and d["level_counts"][0] == seeds.size == 30
    gp, gi = GRAPHS["sparse"]()
    _, _, totals = R.component_counts(R.components(gp, gi))
    d = R.hop_distance(gp, gi, R.random_seeds(3000, 0.05, 2))
    assert 800 <= totals[1] <= 1200 and int((d["dist"] < 0).sum()) > 1000
    gp, gi = GRAPHS["denser"]()
    _, _, totals = R.component_counts(R.components(gp, gi))
    d = R.hop_distance(gp, gi, R.random_seeds(3000, 0.05, 2))
    assert 120 <= totals[1] <= 200 and 6 <= d["levels"] <= 12      # this generator: 156 components, 10 levels
    d = R.hop_distance(*GRAPHS["path"](), [0])
    assert d["levels"] == 299 and np.array_equal(d["dist"], np.arange(300))


def test_reference_on_small_cases():
    # row 2 stores 0 and 1 (one way): 2 is reached from them, they are not reached from 2
    gp, gi = R.csr(4, [2, 2], [0, 1])
    d = R.hop_distance(gp, gi, [2])
    assert d["dist"].tolist() == [-1, -1, 0, -1] and d["levels"] == 0 and d["level_counts"].tolist() == [1]
    d = R.hop_distance(gp, gi, [1, 0, 1, 7, -1])
    assert d["dist"].tolist() == [0, 0, 1, -1] and d["nearest"].tolist() == [0, 1, 0, -1] and d["skipped"] == 2
    assert R.components(gp, gi).tolist() == [0, 0, 0, 3]
    none = R.hop_distance(gp, gi, [])
    assert none["levels"] == 0 and none["level_counts"].tolist() == [0] and np.all(none["dist"] == -1)
    cut = R.hop_distance(*R.path_graph(10), [0], max_hops=3)
    assert cut["dist"].tolist() == [0, 1, 2, 3] + [-1] * 6 and cut["levels"] == 3
    st, unl = R.strata([0, 1, 2, 3, -1, 5], [0, 1, 9, 1, 0, -1], 2, 3, nearest=[0, 0, 0, 1, -1, 3], pred=[0, 0, 0, 1, 1, 0], rows=[0, 1, 2, 3, 4, 5, 6, -1, 3])
    assert st.tolist() == [[1, 1, 1, 1], [1, 1, 0, 0], [1, 0, 0, 0], [3, 2, 2, 2], [1, 1, 0, 0]] and unl == 2


# ---- host/reach.h ------------------------------------------------------------------------------------------------------------

def random_strata(rng, hops, hi=1 << 40):
    rows = rng.integers(0, hi, hops + 2)
    lab = (rows * rng.random(hops + 2)).astype(np.int64)
    return np.stack([rows, lab, (lab * rng.random(hops + 2)).astype(np.int64), (lab * rng.random(hops + 2)).astype(np.int64)], axis=1)


def test_metrics_match_the_python_derivation():
    rng = np.random.default_rng(20261021)
    for hops in (1, 2, 3, 8, 32):
        for layers in sorted({0, min(2, hops - 1), hops - 1}):
            for st in (random_strata(rng, hops), random_strata(rng, hops, hi=50), np.zeros((hops + 2, 4), np.int64)):
                got = reach_metrics(st, hops, layers)
                R.assert_metrics_equal(got, R.metrics(st, hops, layers))
                assert reach_metrics(st, layers=layers) == got      # hops from the shape


def test_known_values():
    st = np.zeros((5, 4), np.int64)                            # hops = 3: buckets 0, 1, 2, ">= 3", unreachable
    st[0] = [4, 4, 4, 4]
    st[1] = [10, 8, 6, 4]
    st[2] = [6, 6, 3, 3]
    st[3] = [5, 4, 1, 2]
    st[4] = [5, 2, 0, 0]
    m = reach_metrics(st, 3, 2)
    assert [r["accuracy"] for r in m["by_distance"]] == [1.0, 0.75, 0.5, 0.25, 0.0]
    assert m["inside_receptive_field"] == dict(rows=20, labelled=18, correct=13, nearest_correct=11, accuracy=13 / 18, nearest_label_accuracy=11 / 18)
    assert m["outside_receptive_field"] == dict(rows=10, labelled=6, correct=1, nearest_correct=2, accuracy=1 / 6, nearest_label_accuracy=2 / 6)
    assert m["unreachable"] == 5 and m["unreachable_share"] == 5 / 30 and m["nearest_label_accuracy"] == 13 / 24 and m["all"]["rows"] == 30
    one = reach_metrics(st, 3, 1)                              # the `layers` cut moves bucket 2 outside
    assert one["inside_receptive_field"]["rows"] == 14 and one["outside_receptive_field"]["rows"] == 16 and one["layers"] == 1
    zero = reach_metrics(st, 3, 0)
    assert zero["inside_receptive_field"]["rows"] == 4 and zero["inside_receptive_field"]["accuracy"] == 1.0
    empty = reach_metrics(np.zeros((10, 4), np.int64))
    assert empty["hops"] == 8 and empty["unreachable_share"] == 0.0 and empty["nearest_label_accuracy"] == 0.0
    assert all(r["accuracy"] == 0.0 and r["nearest_label_accuracy"] == 0.0 for r in empty["by_distance"] + [empty["inside_receptive_field"], empty["all"]])


def test_report_file_round_trips(tmp_path):
    rng = np.random.default_rng(9)
    for i, hops in enumerate((1, 8, 32)):
        st = random_strata(rng, hops)
        rep = dict(strata=st, hops=hops, layers=min(2, hops - 1), totals=rng.integers(0, 1 << 40, 6), level_counts=rng.integers(1, 1 << 30, 4 + 100 * i),
                   sources=17, unlabelled=3, rounds=5)
        path = tmp_path / f"r{i}.txt"
        write_reach_report(path, rep)
        back = read_reach_report(path)
        assert back["hops"] == hops and back["layers"] == rep["layers"] and np.array_equal(back["strata"], st)
        assert np.array_equal(back["totals"], rep["totals"]) and np.array_equal(back["level_counts"], rep["level_counts"])
        assert (back["sources"], back["unlabelled"], back["rounds"], back["levels"]) == (17, 3, 5, rep["level_counts"].size - 1)
        again = tmp_path / f"again{i}.txt"
        write_reach_report(again, back)
        assert again.read_bytes() == path.read_bytes()
        text = path.read_text().splitlines()
        assert text[0] == f"gcn-reach 1 hops {hops} layers {rep['layers']} levels {rep['level_counts'].size - 1}"
        assert sum(l.startswith("strata ") for l in text) == hops + 2
        want = R.metrics(st, hops, rep["layers"])
        f = next(l for l in text if l.startswith("# inside ")).split()
        assert int(f[2]) == want["inside_receptive_field"]["rows"] and abs(float(f[6]) - want["inside_receptive_field"]["accuracy"]) <= 5e-10
    (tmp_path / "cut.txt").write_text("\n".join(text[:-3]) + "\n")
    with pytest.raises(GcnHostError, match="not a complete reach report"):
        read_reach_report(tmp_path / "cut.txt")
    (tmp_path / "other.txt").write_text("node cluster\n")
    with pytest.raises(GcnHostError, match="gcn-reach 1 header"):
        read_reach_report(tmp_path / "other.txt")
    with pytest.raises(GcnHostError, match="cannot open"):
        read_reach_report(tmp_path / "missing.txt")


def test_refusals():
    ok = np.ones((5, 4), np.int64)
    for bad_cell, value in (((1, 0), -1), ((2, 1), 2), ((0, 2), 2), ((4, 3), 2)):
        bad = ok.copy()
        bad[bad_cell] = value
        with pytest.raises(GcnHostError, match="a negative count in strata, or a count above"):
            reach_metrics(bad, 3)
    for layers in (-1, 3, 4):
        with pytest.raises(GcnHostError, match="layers must be in 0..hops - 1"):
            reach_metrics(ok, 3, layers)
    for layers in (1.5, True, "two"):
        with pytest.raises(GcnHostError, match="layers must be an integer"):
            reach_metrics(ok, 3, layers)
    for st, hops in ((np.ones((5, 3), np.int64), None), (ok, 4), (np.ones((35, 4), np.int64), None), (np.ones((2, 4), np.int64), None), (np.ones(20, np.int64), None)):
        with pytest.raises(GcnHostError, match="strata must have shape"):
            reach_metrics(st, hops)
    with pytest.raises(GcnHostError, match="layers must be"):   # the default depth does not fit a table of two exact distances
        reach_metrics(np.ones((4, 4), np.int64))
    lib = _lib.gcnhost()
    assert lib.gcnhost_reach_metrics(None, 3, 2, None, None, None) == -1 and b"reach_metrics" in lib.gcnhost_last_error()
    assert lib.gcnhost_reach_metrics(ok.ctypes.data, 33, 2, None, None, None) == -1
    assert lib.gcnhost_reach_metrics(ok.ctypes.data, 3, 2, None, None, None) == 0


def test_the_c_entry_point_agrees_with_the_python_form():
    rng = np.random.default_rng(4)
    st = random_strata(rng, 6)
    lib = _lib.gcnhost()
    bd, gr, sm = np.zeros((8, 6)), np.zeros((3, 6)), np.zeros(2)
    assert lib.gcnhost_reach_metrics(st.ctypes.data, 6, 2, bd.ctypes.data, gr.ctypes.data, sm.ctypes.data) == 0
    m = reach_metrics(st, 6, 2)
    keys = ("rows", "labelled", "correct", "nearest_correct", "accuracy", "nearest_label_accuracy")
    assert [[r[k] for k in keys] for r in m["by_distance"]] == bd.tolist()
    assert [[m[g][k] for k in keys] for g in ("inside_receptive_field", "outside_receptive_field", "all")] == gr.tolist()
    assert [m["unreachable"], m["unreachable_share"]] == sm.tolist()


def test_host_reach_under_the_sanitizers(tmp_path):
    """host/reach.cpp and a program of its own, built with ASan and UBSan: nothing loaded into Python is instrumented"""
    exe = str(tmp_path / "reach_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "reach_check.cpp"), os.path.join(ROOT, "cuda_gcn_amd", "host", "reach.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "reach_check ok" in r.stdout, r.stderr[-2000:]


def test_symbols_are_exported():
    hip, host = _lib.gcnhip(), _lib.gcnhost()
    for n in ("gcnhip_hop_distance", "gcnhip_hop_distance_ex", "gcnhip_components", "gcnhip_component_counts", "gcnhip_distance_strata"):
        assert n in _lib.GCNHIP_SYMBOLS and hasattr(hip, n)
    for n in ("gcnhost_model_label_distance", "gcnhost_model_components", "gcnhost_model_reach", "gcnhost_reach_metrics", "gcnhost_reach_write",
              "gcnhost_reach_read"):
        assert n in _lib.GCNHOST_SYMBOLS and hasattr(host, n)
