"""What the link prediction ranks need without a GPU: the metrics out of the counts, the held-out edges, the ranks file."""
import numpy as np
import pytest

from cuda_gcn_amd import datagen
from cuda_gcn_amd import model as M
from tests import linkrank_ref as R


@pytest.mark.parametrize("above,equal", [([0, 3, 9, 0, 120], [0, 1, 0, 4, 7]),          # ties: ranks 1, 4.5, 10, 3, 124.5
                                         ([2, -1, 0, -1], [1, -1, 0, -1]),             # invalid queries are left out and counted
                                         ([-1], [-1]), ([], [])])                      # no query: zeros, never NaN
def test_link_rank_metrics(above, equal):
    ks = (1, 3, 10)
    got = M.link_rank_metrics(above, equal, ks)
    rank, mrr, mean_rank, hits = R.metrics(above, equal, ks)
    valid = np.asarray(above, np.int64) >= 0
    assert np.array_equal(got["rank"][valid], rank) and np.all(np.isnan(got["rank"][~valid]))
    assert got["queries"] == rank.size and got["invalid"] == len(above) - rank.size
    assert np.isclose(got["mrr"], mrr, rtol=1e-14, atol=0) and np.isclose(got["mean_rank"], mean_rank, rtol=1e-14, atol=0)
    assert got["hits"] == hits
    with pytest.raises(M.GcnHostError):
        M.link_rank_metrics(above, equal, (0,))


def test_hold_out_edges():
    ds = datagen.make_dataset("cora-syn")
    N = ds["num_nodes"]

    def pairs(d):
        row = np.repeat(np.arange(N), np.diff(d["g_indptr"]))
        return set(zip(row.tolist(), d["g_indices"].tolist()))

    out, (src, dst) = datagen.hold_out_edges(ds, 0.1, 7)
    before, after = pairs(ds), pairs(out)
    held = set(zip(src.tolist(), dst.tolist()))
    n_edges = sum(1 for a, b in before if a < b)
    assert len(held) == src.size == round(0.1 * n_edges) and all(a < b for a, b in held)
    assert all((b, a) in after for a, b in after)                                              # symmetric
    assert not any((a, b) in after or (b, a) in after for a, b in held)                        # disjoint from what remains
    assert after | held | {(b, a) for a, b in held} == before
    assert {(v, v) for v in range(N)} <= after                                                 # self loops stay
    again, (s2, d2) = datagen.hold_out_edges(ds, 0.1, 7)
    assert np.array_equal(s2, src) and np.array_equal(d2, dst) and np.array_equal(again["g_indices"], out["g_indices"])
    assert not np.array_equal(datagen.hold_out_edges(ds, 0.1, 8)[1][0], src)
    assert datagen.hold_out_edges(ds, 0.0, 7)[1][0].size == 0


def test_read_link_ranks(tmp_path):
    p = tmp_path / "ranks.txt"
    p.write_text("3 4 0 2\n5 6 -1 -1\n\n7 8 10 0\n")
    got = M.read_link_ranks(str(p), ks=(2,))
    assert got["src"].tolist() == [3, 5, 7] and got["above"].tolist() == [0, -1, 10] and got["invalid"] == 1
    assert got["hits"] == {2: 0.5} and got["mean_rank"] == 6.5
    p.write_text("3 4 0\n")
    with pytest.raises(M.GcnHostError, match="ranks.txt:1"):
        M.read_link_ranks(str(p))
