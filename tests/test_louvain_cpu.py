"""What of the Louvain communities needs no GPU: the modularity from the integer sums, the plan's byte counts and refusals, the
symbols, and the Python reference of tests/louvain_ref.py on the planted graph."""
import ctypes as C

import numpy as np
import pytest

from cuda_gcn_amd import _lib
from cuda_gcn_amd import model as M
from tests import louvain_ref as L
from tests import overlap_ref as R
from tests.test_overlap_gpu import planted


def test_modularity_from_sums_is_the_formula():
    for num, m2 in ((48575866, 8438), (-392, 56), (0, 56), ((1 << 62) - 1, (1 << 31) - 1), (5, 0)):
        want = num / m2 ** 2 if m2 else 0.0
        assert M.modularity_from_sums(num, m2) == want == _lib.gcnhost().gcnhost_modularity_from_sums(num, m2)
    with pytest.raises(M.GcnHostError):
        M.modularity_from_sums(1, -1)


def test_the_symbols_are_present():
    for name in ("gcnhip_louvain_plan", "gcnhip_louvain_level", "gcnhip_louvain_level_ex", "gcnhip_louvain_coarsen", "gcnhip_louvain_compose"):
        assert name in _lib.GCNHIP_SYMBOLS and hasattr(_lib.gcnhip(), name)
    assert "gcnhost_model_communities" in _lib.GCNHOST_SYMBOLS and hasattr(_lib.gcnhost(), "gcnhost_model_communities")


@pytest.mark.parametrize("n,entries", [(0, 0), (1, 0), (3, 2), (600, 8438), (6000, 25000), (233000, 23_000_000), (5, 1 << 30)])
def test_plan_counts_the_bytes(n, entries):
    r = lambda x: (x + 15) & ~15
    table = 2
    while table < 2 * max(1, min(entries, n)):
        table *= 2
    want = max(64 + 2 * r(8 * n) + 5 * r(4 * n) + 2 * r(4 * table), 64 + 8 * r(4 * (n + 1)))
    got = C.c_int64(-1)
    assert _lib.gcnhip().gcnhip_louvain_plan(n, entries, C.byref(got)) == 0 and got.value == want


def test_plan_refusals():
    lib, got = _lib.gcnhip(), C.c_int64(-1)
    for n, entries, text in ((-1, 0, b"invalid"), (4, -1, b"invalid"), (4, 1 << 31, b"2^31"), (1 << 30, 1 << 30, b"2^30")):
        assert lib.gcnhip_louvain_plan(n, entries, C.byref(got)) == -1 and text in lib.gcnhip_last_error()
    assert lib.gcnhip_louvain_plan(4, 4, None) == -1


def test_read_communities_reads_the_report(tmp_path):
    path = tmp_path / "c.txt"
    path.write_text("gcn-communities 1 nodes 3 communities 2 levels 2\n# Q 0.125 numerator 8 m2 8\n# node community\n0 0\n1 0\n2 1\n")
    got = M.read_communities(path)
    assert got["labels"].tolist() == [0, 0, 1] and got["node"].tolist() == [0, 1, 2]
    assert (got["communities"], got["levels"], got["modularity"], got["numerator"], got["m2"]) == (2, 2, 0.125, 8, 8)
    assert M.modularity_from_sums(got["numerator"], got["m2"]) == got["modularity"]
    path.write_text("gcn-communities 1 nodes 4 communities 2 levels 2\n# Q 0.125 numerator 8 m2 8\n0 0\n")
    for bad in (path, "/nonexistent/c.txt"):
        with pytest.raises(M.GcnHostError, match="read_communities"):
            M.read_communities(bad)


def test_argument_refusals_of_communities():
    m = M.HipGCNModel.__new__(M.HipGCNModel)                                   # the checks come before anything of the model is read
    for kw in (dict(max_levels=0), dict(max_levels=1.5), dict(max_levels=True), dict(max_sweeps=-1)):
        with pytest.raises(M.GcnHostError, match="communities"):
            m.communities(**kw)


def test_the_reference_reaches_the_planted_modularity():
    """a condition on the input, not a tolerance: the move rule finds a labelling at least as good as the planted one"""
    indptr, indices, n = planted()
    S = R.sets(indptr, indices)
    labels, records, num, m2 = L.louvain(S)
    block = np.random.default_rng(78).integers(0, 6, n)                            # planted()'s own first draw, held to its graph:
    same = block[:, None] == block[None, :]                                         # were the helper to change, the densities would not fit
    a = np.zeros((n, n), bool)
    a[np.repeat(np.arange(n), np.diff(indptr)), indices] = True
    assert 0.10 < a[same].sum() / (same.sum() - n) < 0.14 and 0.002 < a[~same].mean() < 0.006
    rows, self_w = L.level0(S)
    planted_num = L.numerator(rows, self_w, [int(np.flatnonzero(block == block[v])[0]) for v in range(n)])[0]
    assert num >= planted_num > 0 and m2 == sum(len(s) for s in S)
    assert L.numerator(rows, self_w, labels)[0] == num == records[-1][2]            # coarsening keeps the numerator
    assert [r[2] for r in records] == sorted(r[2] for r in records)
