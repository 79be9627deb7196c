"""Link prediction ranks on the GPU (csrc/linkrank.hip, ops.Device.link_ranks, HipGCNModel.link_ranks) against the plain reference
of tests/linkrank_ref.py: exact integers on integer tables, with and without the filter; the bound of tests/embed_ref.py on real
tables; the model, its metrics and the command line."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import embed_ref as E
from tests import linkrank_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")


@pytest.fixture(scope="module")
def dev():
    from cuda_gcn_amd.ops import Device
    d = Device(0)
    yield d
    d.close()


def queries(n, nq, seed):
    """nq (src, dst) pairs: a repeated query, and past 2 queries one with src and one with dst outside the table"""
    rng = np.random.default_rng(seed)
    s, d = rng.integers(0, n, nq).astype(np.int32), rng.integers(0, n, nq).astype(np.int32)
    if nq > 2:
        s[-1], d[-1] = s[0], d[0]
        s[1], d[2] = -1, n
    return s, d


def padded_ld(dim):
    return (dim + 3) // 4 * 4 + 4


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("dim", [1, 5, 16, 41, 128, 256])
def test_counts_are_exact_on_integer_tables(dev, dim, n):
    """every chunking, batch size, row stride, metric and exclude_self: above and equal are the reference's integers, with and
    without the filter; the filtered counts are the unfiltered ones minus what the reference says the removed candidates counted"""
    tables = {"dot": R.integer_table(n, dim, 100 * dim + n), "cosine": R.integer_table(n, dim, 100 * dim + n + 1, unit=True)}
    score_mats = {m: t.astype(np.float64) @ t.astype(np.float64).T for m, t in tables.items()}       # exact integers
    inv = {"dot": None, "cosine": dev.embed_inv_norms(tables["cosine"])}
    for chunk_rows, nq, ld, metric, ex in itertools.product((0, 64, 333), (1, 19, 67), (dim, padded_ld(dim)), ("dot", "cosine"), (True, False)):
        src, dst = queries(n, nq, nq + chunk_rows)
        x_ptr, x_ids, sets = R.filter_sets(n, chunk_rows, src, dst, nq)
        S = score_mats[metric]
        want_plain = R.link_ranks(lambda s: S[s], n, src, dst, None, ex)
        want = R.link_ranks(lambda s: S[s], n, src, dst, sets, ex)
        what = (chunk_rows, nq, ld, metric, ex)
        a0, e0 = dev.link_ranks(tables[metric], src, dst, inv[metric], exclude_self=ex, chunk_rows=chunk_rows, ld=ld)
        assert np.array_equal(a0, want_plain[0]) and np.array_equal(e0, want_plain[1]), what
        a1, e1 = dev.link_ranks(tables[metric], src, dst, inv[metric], x_ptr, x_ids, exclude_self=ex, chunk_rows=chunk_rows, ld=ld)
        assert np.array_equal(a1, want[0]) and np.array_equal(e1, want[1]), what
        ok = want[0] >= 0
        assert np.array_equal((a0 - a1)[ok], want[2][ok]) and np.array_equal((e0 - e1)[ok], want[3][ok]), what
    a2, e2 = dev.link_ranks(tables[metric], src, dst, inv[metric], x_ptr, x_ids, exclude_self=ex, chunk_rows=chunk_rows, ld=ld)
    assert a2.tobytes() == a1.tobytes() and e2.tobytes() == e1.tobytes()                              # a second call: the same bytes


@pytest.mark.parametrize("dim", [41, 128])
def test_counts_hold_the_bound_on_real_tables(dev, dim):
    """normal entries: per query #{s64 > t64 + E_c + E_d} <= above and above + equal <= #{s64 >= t64 - E_c - E_d} over its candidates
    (E: the bound of tests/embed_ref.py), no query left out; link_thresholds lies within E_d of t64"""
    n = 1000
    x = np.random.default_rng(dim).standard_normal((n, dim)).astype(np.float32)
    src, dst = queries(n, 67, dim)
    x_ptr, x_ids, sets = R.filter_sets(n, 333, src, dst, dim)
    for metric in ("dot", "cosine"):
        inv = dev.embed_inv_norms(x) if metric == "cosine" else None
        r64 = E.inv_norms64(x) if metric == "cosine" else None
        thr = dev.link_thresholds(x, src, dst, inv)
        above, equal = dev.link_ranks(x, src, dst, inv, x_ptr, x_ids, chunk_rows=333)
        for i, (s, d) in enumerate(zip(src, dst)):
            if not (0 <= s < n and 0 <= d < n):
                assert above[i] == -1 and equal[i] == -1 and np.isnan(thr[i])
                continue
            s64, err = E.scores64(x, s, metric, r64)
            assert abs(float(thr[i]) - s64[d]) <= err[d], (metric, i)
            cand = np.ones(n, bool)
            cand[[s, d]] = False
            cand[sets[s][(sets[s] >= 0) & (sets[s] < n)]] = False
            lo = int((s64[cand] > s64[d] + err[cand] + err[d]).sum())
            hi = int((s64[cand] >= s64[d] - err[cand] - err[d]).sum())
            assert lo <= above[i] and above[i] + equal[i] <= hi, (metric, i, lo, int(above[i]), int(equal[i]), hi)


def test_kernel_refusals(dev):
    from cuda_gcn_amd.ops import GcnHipError
    x = np.ones((8, 4), np.float32)
    for kw, word in ((dict(table=np.ones((8, 257), np.float32)), "1 <= dim <= 256"), (dict(chunk_rows=-1), "chunk_rows")):
        with pytest.raises(GcnHipError, match=word):
            dev.link_ranks(**dict(dict(table=x, src=[0], dst=[1]), **kw))


# ---- the model ------------------------------------------------------------------------------------------------------------

def neighbour_sets(ds):
    """the distinct neighbours u != v of every node, sorted: what the model's filter holds"""
    gp, gi = ds["g_indptr"], ds["g_indices"]
    sets = [np.unique(gi[gp[v]:gp[v + 1]][gi[gp[v]:gp[v + 1]] != v]).astype(np.int32) for v in range(ds["num_nodes"])]
    x_ptr = np.zeros(len(sets) + 1, np.int32)
    np.cumsum([s.size for s in sets], out=x_ptr[1:])
    return x_ptr, np.concatenate(sets)


def test_model_link_ranks(dev):
    """HipGCNModel.link_ranks = Device.link_ranks on embed()'s table with sets built from the dataset's rows, byte for byte; the
    metrics are link_rank_metrics of those integers; weights and the next epoch are what they are without the call"""
    from cuda_gcn_amd import model as M
    ds, (src, dst) = datagen.hold_out_edges(datagen.planted_communities(n_comm=4, size=64, p_in=0.8, feats=8), 0.1, 3)
    assert src.size > 64
    src, dst = np.append(src, src[0]), np.append(dst, dst[0])
    a, b = (M.HipGCNModel(ds, seed=5, hidden_dim=16, dropout=0.5) for _ in range(2))
    a.run_epochs(5, want_trace=False)
    b.run_epochs(5, want_trace=False)
    emb = b.embed()
    x_ptr, x_ids = neighbour_sets(ds)
    for metric, filtered in itertools.product(("dot", "cosine"), (True, False)):
        got = b.link_ranks(src, dst, metric=metric, filtered=filtered, ks=(1, 10))
        inv = dev.embed_inv_norms(emb) if metric == "cosine" else None
        wa, we = dev.link_ranks(emb, src, dst, inv, *((x_ptr, x_ids) if filtered else ()))
        assert got["above"].tobytes() == wa.tobytes() and got["equal"].tobytes() == we.tobytes(), (metric, filtered)
        ref = M.link_rank_metrics(wa, we, (1, 10))
        assert all(np.array_equal(got[k], ref[k]) for k in ("rank", "mrr", "mean_rank", "hits", "queries", "invalid")), (metric, filtered)
        assert got["queries"] == src.size and got["invalid"] == 0 and 0 < got["mrr"] <= 1
    assert b.link_ranks([0, 10 ** 6], [1, 2])["invalid"] == 1                       # an id that is no node: answered, not refused
    for k in (2, 5):
        assert a.var(k).tobytes() == b.var(k).tobytes()
    assert a.train_epoch() == b.train_epoch()
    for args, kw in (((src, dst[:-1]), {}), ((src, dst), dict(metric="euclid")), ((src, dst), dict(ks=(0, 10)))):
        with pytest.raises(M.GcnHostError):
            b.link_ranks(*args, **kw)
    a.close()
    b.close()


def test_cli_link_ranks(tmp_path):
    """gcn-hip with GCN_LINK_EDGES and GCN_LINK_RANKS: the printed line and the file are HipGCNModel.link_ranks on the same weights"""
    from cuda_gcn_amd import model as M
    ds, (src, dst) = datagen.hold_out_edges(datagen.make_dataset("cora-syn"), 0.05, 1)
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "cora-syn.gcnbin"))
    m = M.HipGCNModel(ds, seed=3, hidden_dim=16, dropout=0.5)
    m.run_epochs(6, want_trace=False)
    w, edges, out = (str(tmp_path / f) for f in ("w.gcnw", "edges.txt", "ranks.txt"))
    m.save_weights(w)
    want = m.link_ranks(src, dst, ks=(10,))
    m.close()
    np.savetxt(edges, np.stack([src, dst], 1), fmt="%d")
    env = dict(os.environ, GCN_SEED="3", GCN_LOAD_WEIGHTS=w, GCN_LINK_EDGES=edges, GCN_LINK_RANKS=out)
    r = subprocess.run(["timeout", "-k", "10", "50", HIP, "cora-syn", "-", "-", "16", "-", "0.5", "-", "-", "0"], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    line = dict(p.split("=") for p in r.stdout.strip().splitlines()[-1].split())
    got = M.read_link_ranks(out, ks=(10,))
    assert all(np.array_equal(got[k], want[k]) for k in ("above", "equal", "rank", "mrr", "hits")) and np.array_equal(got["src"], src)
    assert int(line["link_queries"]) == src.size and abs(float(line["link_mrr"]) - want["mrr"]) < 1e-6
    assert abs(float(line["link_hits@10"]) - want["hits"][10]) < 1e-6
