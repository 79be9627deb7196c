"""What of the structure report needs no GPU: the measures of host/structure.h against the float64 derivation of
tests/structure_ref.py, the datasets' planted homophily, the 2^-32 bound of the integer node homophily, the report file, refusals
and the symbols."""
import numpy as np
import pytest

from cuda_gcn_amd import _lib, datagen
from cuda_gcn_amd.model import GcnHostError, read_structure_report, structure_metrics, write_structure_report
from tests import structure_ref as R


def random_tables(rng, C, bins, hi=1 << 40):
    mix = rng.integers(0, hi, (C, C))
    class_rows = rng.integers(0, hi, C)
    rows = rng.integers(0, 1 << 20, (32, bins + 1))
    strata = np.stack([rows, (rows * rng.random((32, bins + 1))).astype(np.int64)], axis=2)
    known_rows = int(rng.integers(1, 1 << 20))
    totals = np.array([known_rows + 5, known_rows + 3, known_rows, 1 << 33, 1 << 32, 1 << 31, 77, 0], np.int64)
    totals[7] = int(rng.integers(0, known_rows)) * R.TWO32 + int(rng.integers(0, R.TWO32))
    return mix, class_rows, totals, strata


def cases():
    rng = np.random.default_rng(20261021)
    out = []
    for C, bins in ((2, 1), (5, 10), (41, 10), (64, 32), (7, 3)):
        out.append((f"random C={C}", *random_tables(rng, C, bins)))
    mix, rows, totals, strata = random_tables(rng, 6, 4, hi=1000)
    mix[2, :] = 0                                              # an empty row, an empty column, a class without rows
    mix[:, 4] = 0
    rows[2] = 0
    strata[5:, :, :] = 0
    strata[:, 2, :] = 0
    out.append(("empty rows and columns", mix, rows, totals, strata))
    out.append(("C = 1", *random_tables(rng, 1, 2)))
    out.append(("all zero", np.zeros((5, 5), np.int64), np.zeros(5, np.int64), np.zeros(8, np.int64), np.zeros((32, 11, 2), np.int64)))
    mix, rows, totals, strata = random_tables(rng, 8, 10)
    out.append(("diagonal", np.diag(np.diag(mix)), rows, totals, strata))
    one = np.zeros((4, 4), np.int64)                            # every edge leaves one class: 1 - sum p^2 = 0
    one[1, 1] = 9
    out.append(("one class has every edge", one, np.array([0, 3, 0, 0]), totals, strata))
    return out


@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_metrics_match_the_float64_derivation(case):
    _, mix, class_rows, totals, strata = case
    got = structure_metrics(mix, class_rows, totals, strata)
    R.assert_metrics_close(got, R.metrics(mix, class_rows, totals, strata))
    for v in got.values():                                     # never NaN
        if not isinstance(v, list):
            assert np.all(np.isfinite(np.asarray(v, np.float64)))
    assert all(np.isfinite(r["accuracy"]) for r in got["by_degree"] + got["by_agreement"])
    assert len(got["by_degree"]) == 32 and len(got["by_agreement"]) == strata.shape[1]
    assert got["strata_rows"] == sum(r["rows"] for r in got["by_degree"]) == sum(r["rows"] for r in got["by_agreement"])
    without = structure_metrics(mix, class_rows)
    assert without["node_homophily"] == 0.0 and "by_degree" not in without
    assert without["edge_homophily"] == got["edge_homophily"]


def test_known_values():
    m = structure_metrics([[5, 1], [2, 8]], [3, 4])
    assert m["edge_homophily"] == 13 / 16 and m["edges"] == 16 and m["labelled_rows"] == 7
    assert np.array_equal(m["class_homophily"], [5 / 6, 8 / 10])
    assert np.array_equal(m["compatibility"], [[5 / 6, 1 / 6], [2 / 10, 8 / 10]])
    p2 = (6 / 16) ** 2 + (10 / 16) ** 2
    assert abs(m["adjusted_homophily"] - (13 / 16 - p2) / (1 - p2)) < 1e-15
    assert abs(m["class_insensitive_homophily"] - ((5 / 6 - 3 / 7) + (8 / 10 - 4 / 7))) < 1e-15
    d = structure_metrics(np.eye(3, dtype=np.int64) * 4, [1, 1, 1])
    assert d["edge_homophily"] == 1.0 and d["adjusted_homophily"] == 1.0 and np.array_equal(d["compatibility"], np.eye(3))
    bounds = structure_metrics(np.eye(2, dtype=np.int64), [1, 1], strata=np.zeros((32, 5, 2), np.int64))
    assert [(r["lo"], r["hi"]) for r in bounds["by_degree"][:4]] == [(0, 0), (1, 1), (2, 3), (4, 7)]
    assert bounds["by_degree"][31]["hi"] == 2 ** 31 - 1
    assert [(r["lo"], r["hi"]) for r in bounds["by_agreement"]] == [(0, 0.25), (0.25, 0.5), (0.5, 0.75), (0.75, 1.0), (-1, -1)]


@pytest.mark.parametrize("name", ["tiny-syn", "cora-syn"])
def test_edge_homophily_is_the_generators(name):
    ds = datagen.make_dataset(name)
    C = ds["output_dim"]
    ref = R.agreement(ds["g_indptr"], ds["g_indices"], ds["label"], C)
    got = structure_metrics(ref["mix"], ref["class_rows"], ref["totals"])
    assert got["edge_homophily"] == datagen.edge_homophily(ds)
    assert abs(got["node_homophily"] - R.node_homophily_float(ref["same"], ref["known"])) <= 2.0 ** -32
    assert got["edges"] == int(ref["totals"][4]) and got["labelled_rows"] == ds["num_nodes"]


def test_node_homophily_is_within_2_to_minus_32_of_the_mean():
    rng = np.random.default_rng(5)
    for n in (1, 3, 1000, 100000):
        known = rng.integers(0, 50, n)
        same = (known * rng.random(n)).astype(np.int64)
        same[rng.random(n) < 0.2] = 0                           # some rows agree nowhere
        m = known > 0
        ratio_sum = sum((int(s) * R.TWO32) // int(k) for s, k in zip(same[m], known[m]))
        totals = np.array([n, n, int(m.sum()), 0, int(known.sum()), int(same.sum()), 0, 0], np.int64)
        totals[7] = np.array([ratio_sum], np.uint64).view(np.int64)[0]
        got = structure_metrics(np.eye(2, dtype=np.int64), [1, 1], totals)["node_homophily"]
        want = R.node_homophily_float(same, known)
        assert abs(want - got) <= 2.0 ** -32, (n, got, want)
    # an unsigned sum: 2^31 rows of perfect agreement wrap the int64 the table travels in, not the measure
    totals = np.array([1 << 31, 1 << 31, 1 << 31, 0, 1 << 31, 1 << 31, 0, 0], np.int64)
    totals[7] = np.array([(1 << 31) * R.TWO32], np.uint64).view(np.int64)[0]
    assert totals[7] < 0 and structure_metrics(np.eye(2, dtype=np.int64), [1, 1], totals)["node_homophily"] == 1.0


def test_report_file_round_trips(tmp_path):
    rng = np.random.default_rng(9)
    for i, (C, bins) in enumerate(((1, 1), (5, 10), (64, 32))):
        mix_t, rows_t, tot_t, strata = random_tables(rng, C, bins)
        mix_p, rows_p, tot_p, _ = random_tables(rng, C, bins)
        rep = dict(truth=dict(mix=mix_t, class_rows=rows_t, totals=tot_t), pred=dict(mix=mix_p, class_rows=rows_p, totals=tot_p), strata=strata)
        path = tmp_path / f"s{i}.txt"
        write_structure_report(path, rep)
        back = read_structure_report(path)
        assert back["num_classes"] == C and back["bins"] == bins and np.array_equal(back["strata"], strata)
        for side in ("truth", "pred"):
            for key in ("mix", "class_rows", "totals"):
                assert np.array_equal(back[side][key], rep[side][key]), (side, key)
        again = tmp_path / f"again{i}.txt"
        write_structure_report(again, back)
        assert again.read_bytes() == path.read_bytes()
        text = path.read_text().splitlines()
        assert text[0] == f"gcn-structure 1 classes {C} bins {bins}"
        assert sum(l.startswith("mix_truth ") for l in text) == C and sum(l.startswith("mix_pred ") for l in text) == C
        assert any(l.startswith("# by_degree") for l in text) and any(l.startswith("# by_agreement") for l in text)
        want = R.metrics(mix_t, rows_t, tot_t)
        line = next(l for l in text if l.startswith("# truth "))
        fields = dict(p.split("=") for p in line.split()[2:])
        assert abs(float(fields["edge_homophily"]) - want["edge_homophily"]) <= 5e-10 and int(fields["edges"]) == want["edges"]
    (tmp_path / "cut.txt").write_text("\n".join(text[:-3]) + "\n")
    with pytest.raises(GcnHostError, match="not a complete structure report"):
        read_structure_report(tmp_path / "cut.txt")
    (tmp_path / "other.txt").write_text("node cluster\n")
    with pytest.raises(GcnHostError, match="gcn-structure 1 header"):
        read_structure_report(tmp_path / "other.txt")
    with pytest.raises(GcnHostError, match="cannot open"):
        read_structure_report(tmp_path / "missing.txt")


def test_refusals():
    ok_mix, ok_rows = np.ones((3, 3), np.int64), np.ones(3, np.int64)
    bad = ok_mix.copy()
    bad[1, 2] = -1
    with pytest.raises(GcnHostError, match="a negative count in mix"):
        structure_metrics(bad, ok_rows)
    with pytest.raises(GcnHostError, match="a negative count in class_rows"):
        structure_metrics(ok_mix, [1, -2, 3])
    with pytest.raises(GcnHostError, match="a negative count in totals"):
        structure_metrics(ok_mix, ok_rows, [1, 1, -1, 0, 0, 0, 0, 0])
    strata = np.ones((32, 4, 2), np.int64)
    neg = strata.copy()
    neg[3, 1, 0] = -5
    with pytest.raises(GcnHostError, match="a negative count in strata"):
        structure_metrics(ok_mix, ok_rows, strata=neg)
    more = strata.copy()
    more[0, 0, 1] = 2                                          # more correct rows than rows
    with pytest.raises(GcnHostError, match="more correct rows than rows"):
        structure_metrics(ok_mix, ok_rows, strata=more)
    for mix in (np.ones((3, 4), np.int64), np.ones(9, np.int64), np.ones((65, 65), np.int64), np.ones((0, 0), np.int64)):
        with pytest.raises(GcnHostError, match="mix must be"):
            structure_metrics(mix, ok_rows)
    with pytest.raises(GcnHostError, match="class_rows must have shape"):
        structure_metrics(ok_mix, np.ones(4, np.int64))
    with pytest.raises(GcnHostError, match="totals must have shape"):
        structure_metrics(ok_mix, ok_rows, np.ones(7, np.int64))
    for st, bins in ((np.ones((31, 4, 2), np.int64), None), (strata, 5), (np.ones((32, 34, 2), np.int64), None), (np.ones((32, 4), np.int64), None)):
        with pytest.raises(GcnHostError, match="strata must have shape"):
            structure_metrics(ok_mix, ok_rows, strata=st, bins=bins)
    lib = _lib.gcnhost()
    assert lib.gcnhost_structure_metrics(0, ok_mix.ctypes.data, ok_rows.ctypes.data, None, 0, None, None, None, None, None, None) == -1
    assert b"structure_metrics" in lib.gcnhost_last_error()
    assert lib.gcnhost_structure_metrics(3, ok_mix.ctypes.data, ok_rows.ctypes.data, None, 33, strata.ctypes.data, None, None, None, None, None) == -1


def test_symbols_are_exported():
    hip, host = _lib.gcnhip(), _lib.gcnhost()
    for n in ("gcnhip_nbr_agreement", "gcnhip_nbr_agreement_ex", "gcnhip_strata_counts"):
        assert n in _lib.GCNHIP_SYMBOLS and hasattr(hip, n)
    for n in ("gcnhost_model_neighbor_agreement", "gcnhost_model_structure", "gcnhost_structure_metrics", "gcnhost_structure_write", "gcnhost_structure_read"):
        assert n in _lib.GCNHOST_SYMBOLS and hasattr(host, n)
