"""Irregular inputs on the CPU: the generators of tests/irregular_inputs.py really contain what they promise, the CPU oracle
agrees with a float64 statement of the same products on them (so the expected values of test_irregular_gpu.py are proven
before a GPU sees them, and the reference alone is shown to stay inside the bound applied there), and the host loader
reproduces such files element for element, through the binary cache as well.

Bound: test_ops_gpu.close_mag with k = 8 — the project's bound for two f32 summations of the same terms.  Each test prints
its measured worst ratio |oracle - float64| / (eps_f32 . mag) before asserting it.
"""
import os
import tempfile

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import irregular_inputs as irr
from tests.irregular_inputs import dense_reference
from tests.test_ops_gpu import close_mag, EPS

KEYS = ("g_indptr", "g_indices", "f_indptr", "f_indices", "f_val", "split", "label")


def ratio(got, want, mag):
    """worst |got - want| in units of eps_f32 . mag (close_mag asserts <= 8)"""
    m = np.asarray(mag, np.float64)
    d = np.abs(np.asarray(got, np.float64) - want)
    return float((d[m > 0] / (EPS * m[m > 0])).max()) if np.any(m > 0) else 0.0


# ------------------------------------------------------------------------------------------------- generator properties
@pytest.mark.parametrize("which", ["ops", "model"])
def test_irregular_graph_has_every_property(which):
    if which == "ops":
        gp, gi = irr.gpu_graph()
        n = 1500
    else:
        ds = irr.irregular_dataset()
        gp, gi, n = ds["g_indptr"], ds["g_indices"], ds["num_nodes"]
    assert gp.dtype == np.int32 and gi.dtype == np.int32 and gp.size == n + 1 and gp[-1] == gi.size
    p = irr.graph_properties(gp, gi)
    print(p)
    assert p["self_loop_first"]                                    # the loader's layout
    assert p["unsorted_rows"] >= n // 2                            # shuffled neighbour order
    assert p["repeated_pairs"] >= n // 20                          # a pair stored twice
    assert p["max_repeat"] >= 300                                  # one row lists a single neighbour hundreds of times
    assert p["rows_listing_themselves_again"] >= n // 40           # the self loop stored twice or more
    assert p["one_way_share"] >= 0.10                              # stored edges without their mirror
    assert p["self_only_rows"] >= n // 25                          # rows with the self loop only
    assert p["hub_len"] == 2500 and p["hub_distinct"] < 1024       # above the 1 024 split length through repeats alone
    assert p["unreferenced_nodes_with_neighbours"] >= 1            # a node no other row references
    assert p["rows_where_in_degree_differs"] >= n // 2             # "degree of column j" must be row j's stored length
    # the same generator at the ends of the size range the GPU tests may use
    for m in (300, 3000):
        q = irr.graph_properties(*irr.irregular_graph(np.random.default_rng(irr.SEED_GRAPH), m))
        assert q["hub_len"] == 2500 and q["hub_distinct"] < 1024 and q["max_repeat"] >= 300 and q["one_way_share"] >= 0.10


@pytest.mark.parametrize("case", sorted(irr.FEATURE_CASES))
def test_irregular_features_have_every_property(case):
    fp, fi, fv, F = irr.gpu_features(case)
    cfg = irr.FEATURE_CASES[case]
    n = cfg["n"]
    assert fp.dtype == np.int32 and fi.dtype == np.int32 and fv.dtype == np.float32 and fp.size == n + 1 and fp[-1] == fi.size == fv.size
    p = irr.feature_properties(fp, fi, fv, F)
    print(p)
    assert p["unsorted_rows"] >= n // 2 and p["rows_with_repeats"] >= n // 8
    assert p["pos_zero"] >= 10 and p["neg_zero"] >= 10
    assert p["first_row_empty"] and p["last_row_empty"]
    assert p["rows_of_F_copies"] == 1
    if cfg["missing"] == "last":
        assert p["empty_columns"].tolist() == [F - 3, F - 2, F - 1] and p["full_permutation_rows"] == 0
        assert np.unique(fi[fp[1]:fp[2]]).size == fp[2] - fp[1] == F - 3          # a permutation of every column in use
    elif cfg["missing"] == "first":
        assert p["empty_columns"].tolist() == [0, 1, 2] and p["full_permutation_rows"] == 0
        assert np.unique(fi[fp[1]:fp[2]]).size == fp[2] - fp[1] == F - 3
    else:
        assert p["empty_columns"].size == 0 and p["full_permutation_rows"] == 1     # a permutation of all F columns
    if cfg.get("long_repeat"):
        # longer than every segment length of the weight gradient (1 024 at 1 and 4 waves, 4 096 at 16) through ONE row
        assert p["longest_column"] > 4096 and p["longest_column_most_from_one_row"] >= 4096 and p["longest_column_rows"] < 1024


def test_permuted_full_matrix_is_full_but_not_in_dense_layout():
    n, F = 300, 48
    fp, fi, fv, row = irr.permuted_full_features(np.random.default_rng(irr.SEED_FEAT), n, F)
    assert fi.size == n * F and np.array_equal(np.diff(fp), np.full(n, F))
    ident = (fi.reshape(n, F) == np.arange(F)).all(1)
    assert ident.sum() == n - 1 and not ident[row]
    assert np.array_equal(np.sort(fi.reshape(n, F)[row]), np.arange(F))
    sp, si, sv = irr.sorted_rows(fp, fi, fv)                         # the dense control: same matrix, every row in order
    assert np.array_equal(si, np.tile(np.arange(F), n))
    assert np.array_equal(irr.dense_features(fp, fi, fv, F), irr.dense_features(sp, si, sv, F))


def test_irregular_dataset_has_every_property():
    ds = irr.irregular_dataset()
    n, F, c = ds["num_nodes"], ds["input_dim"], ds["output_dim"]
    assert 600 <= n <= 1200 and F == 60 and c == 5
    p = irr.feature_properties(ds["f_indptr"], ds["f_indices"], ds["f_val"], F)
    print(p)
    assert p["unsorted_rows"] >= n // 2 and p["rows_with_repeats"] >= n // 8 and p["pos_zero"] >= 10 and p["neg_zero"] >= 10
    assert p["first_row_empty"] and p["last_row_empty"] and p["rows_of_F_copies"] == 1 and p["empty_columns"].tolist() == [0, 1, 2]
    assert int(ds["f_indices"].max()) == F - 1 and int(ds["label"].max()) == c - 1       # the loader recovers both widths
    assert all(int((ds["split"] == s).sum()) >= n // 5 for s in (1, 2, 3))
    # labels are planted: most of a node's feature mass sits in its class's block, most neighbours share its class
    gp, gi = ds["g_indptr"], ds["g_indices"]
    src = np.repeat(np.arange(n), np.diff(gp))
    other = src != gi
    assert (ds["label"][src[other]] == ds["label"][gi[other]]).mean() > 0.5


# ---------------------------------------------------------------------------------------------- oracle against float64
HEAVY_ROW_K = {1: 8.25, 7: 31.5, 41: 35.5, 128: 44.0, 260: 45.0}      # 1.25 x (6.6, 25.1, 28.2, 34.9, 36.0): see the finding below


@pytest.mark.parametrize("dim", [1, 7, 41, 128, 260])
def test_oracle_graphsum_vs_float64(oracle, dim):
    """FINDING (the reference's arithmetic, not a defect of the checker): on the row that lists one neighbour 300 times the
    reference's sequential f32 sum is 6.6 / 25.1 / 28.2 / 34.9 / 36.0 eps.mag away from float64 at widths 1 / 7 / 41 / 128 /
    260 — outside close_mag's k = 8.  300 identical terms are added to a growing partial sum, so the rounding errors share
    a sign instead of cancelling; k = 8 is a statement about terms of mixed sign.  Every other row, the 2 500-entry hub
    included (2.2), is inside k = 8.  (The bound that holds for ANY f32 sum of m = 307 terms is (m + 2) / 2 = 154.)  On
    that one row the assertion here is HEAVY_ROW_K: the measured figure of each width plus a quarter, so that a later change
    of the oracle on this row shows; test_irregular_gpu.py holds the GPU on that row to float64 within max(8, the oracle's
    own distance on its input)."""
    gp, gi = irr.gpu_graph()
    n = gp.size - 1
    x = np.random.default_rng(dim).standard_normal((n, dim)).astype(np.float32)
    want, mag = dense_reference.graphsum(gp, gi, x)
    got = oracle.graphsum(gp, gi, x, dim)
    heavy = irr.rows_repeating_one_entry(gp, gi)
    assert heavy.tolist() == [1]
    rest = np.setdiff1d(np.arange(n), heavy)
    print(f"graphsum dim {dim}: oracle vs float64 = {ratio(got[rest], want[rest], mag[rest]):.2f} eps.mag, "
          f"row of 300 identical terms {ratio(got[heavy], want[heavy], mag[heavy]):.2f}")
    close_mag(got[rest], want[rest], mag[rest])
    for r in heavy:                                   # the figure measured on this input, with a quarter of headroom
        close_mag(got[r], want[r], mag[r], k=HEAVY_ROW_K[dim])
    # the oracle's own magnitude (what existing GPU tests pass as `mag`) is the float64 one to a relative 1e-5: a scale
    omag = oracle.graphsum(gp, gi, np.abs(x), dim)
    assert np.all(np.abs(omag - mag) <= 1e-5 * mag)


@pytest.mark.parametrize("case", sorted(irr.FEATURE_CASES))
@pytest.mark.parametrize("p", [3, 16, 41, 64, 128, 256])
def test_oracle_spmm_vs_float64(oracle, case, p):
    fp, fi, fv, F = irr.gpu_features(case)
    n = fp.size - 1
    rng = np.random.default_rng(p)
    w = rng.standard_normal((F, p)).astype(np.float32)
    dout = rng.standard_normal((n, p)).astype(np.float32)
    want, mag = dense_reference.spmm_fwd(fp, fi, fv, F, w)
    got = oracle.spmm_fwd(fp, fi, fv, w, p)
    r_f = ratio(got, want, mag)
    wantb, magb = dense_reference.spmm_bwd(fp, fi, fv, F, dout)
    gotb = oracle.spmm_bwd(fp, fi, fv, dout, F, p)
    print(f"spmm {case} p {p}: oracle vs float64 forward {r_f:.2f}, weight gradient {ratio(gotb, wantb, magb):.2f} eps.mag")
    close_mag(got, want, mag)
    close_mag(gotb, wantb, magb)
    assert np.all(got[0] == 0) and np.all(got[-1] == 0)                     # the empty rows
    empty = irr.feature_properties(fp, fi, fv, F)["empty_columns"]
    assert np.all(gotb[empty] == 0)                                         # the columns that never occur


def test_oracle_first_epoch_loss_vs_float64(oracle):
    """the oracle model's first training loss and accuracy on the irregular dataset (dropout 0) against a float64 numpy
    forward with the same Glorot weights: 2e-5, test_first_epoch_tensors_vs_oracle's first-epoch bound"""
    ds = irr.irregular_dataset()
    om = oracle.model(ds, seed_time=5, hidden_dim=16, dropout=0.0)
    w1 = om.var(2).reshape(ds["input_dim"], 16)
    w2 = om.var(5).reshape(16, ds["output_dim"])
    want_loss, want_acc, z = dense_reference.model_forward(ds, w1, w2, split=1)
    loss, acc = om.train_epoch()
    print(f"first-epoch loss: oracle {loss:.7f} float64 {want_loss:.7f} (diff {abs(loss - want_loss):.2e}); acc {acc:.5f} / {want_acc:.5f}")
    assert abs(loss - want_loss) <= 2e-5
    assert abs(acc - want_acc) <= 1.0 / int((ds["split"] == 1).sum()) + 1e-7
    # and training moves on this dataset
    for _ in range(30):
        last = om.train_epoch()
    assert last[0] < loss - 0.2 and last[1] > max(acc, 0.5)
    om.close()


# ------------------------------------------------------------------------------------------------- parser round trip
def test_parser_round_trip_of_an_irregular_dataset(oracle):
    """text files of an irregular dataset -> the C++ loader == the oracle's loader == the generator's arrays (values by
    their bits: -0.0 survives), and again through the .gcnbin cache"""
    from cuda_gcn_amd import model
    ds = irr.irregular_dataset()
    with tempfile.TemporaryDirectory() as td:
        datagen.write_text(ds, td, "irr")
        a = model.load_dataset(td, "irr")
        b = oracle.parse(td, "irr")
        for k in KEYS:
            assert a[k].size == np.asarray(ds[k]).size, k
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], ds[k]), k
        assert np.array_equal(np.asarray(a["f_val"], np.float32).view(np.uint32), ds["f_val"].view(np.uint32))
        assert np.array_equal(np.asarray(b["f_val"], np.float32).view(np.uint32), ds["f_val"].view(np.uint32))
        assert (a["num_nodes"], a["input_dim"], a["output_dim"]) == (ds["num_nodes"], ds["input_dim"], ds["output_dim"])
        model.save_binary(a, os.path.join(td, "irr.gcnbin"))
        for ext in (".graph", ".split", ".svmlight"):
            os.remove(os.path.join(td, "irr" + ext))
        c = model.load_dataset(td, "irr")                            # only the cache is left
        for k in KEYS:
            assert np.array_equal(c[k], ds[k]), k
        assert np.array_equal(np.asarray(c["f_val"], np.float32).view(np.uint32), ds["f_val"].view(np.uint32))
        assert (c["num_nodes"], c["input_dim"], c["output_dim"]) == (ds["num_nodes"], ds["input_dim"], ds["output_dim"])


# ------------------------------------------------------------------------------------- host plans on a non-symmetric graph
@pytest.mark.parametrize("world,mode", [(2, 0), (3, 1), (3, 2), (4, 2)])
def test_exchange_plans_on_a_non_symmetric_graph(world, mode):
    """test_host_cpu.test_exchange_plans_are_consistent_across_ranks on the irregular adjacency: a rank's halo is what ITS rows
    list, not who lists them; repeats stay; the column degrees are stored row lengths — the aggregation through each rank's
    table equals the float64 operator"""
    from cuda_gcn_amd import model
    gp, gi = irr.gpu_graph()
    N = gp.size - 1
    start, _ = model.partition(gp, world)
    plans = [model.exchange_plan(gp, gi, world, r, mode) for r in range(world)]
    assert len({p["halo"] for p in plans}) == 1
    halo = plans[0]["halo"]
    assert halo == (mode == 2) or mode == 0
    x = np.random.default_rng(1).standard_normal((N, 5)).astype(np.float32)
    want, mag = dense_reference.graphsum(gp, gi, x)
    deg = np.diff(gp).astype(np.int64)
    for rank, p in enumerate(plans):
        r0, r1 = int(start[rank]), int(start[rank + 1])
        tg = p["table_global"]
        assert p["n_local"] == r1 - r0 and np.array_equal(tg[p["own_offset"]:p["own_offset"] + p["n_local"]], np.arange(r0, r1))
        if halo:
            for q in range(world):
                seg = p["recv_rows"][p["recv_off"][q]:p["recv_off"][q + 1]]
                sent = plans[q]["send_rows"][plans[q]["send_off"][rank]:plans[q]["send_off"][rank + 1]]
                assert np.array_equal(seg, sent), (rank, q)
            need = np.unique(gi[gp[r0]:gp[r1]])
            need = need[(need < r0) | (need >= r1)]
            assert np.array_equal(np.sort(tg[p["n_local"]:p["n_local"] + p["recv_rows"].size]), need)   # no more, no less
        ip, ix, cd = p["indptr"], p["indices"], p["col_deg"]
        assert np.array_equal(np.diff(ip), deg[r0:r1])                           # every stored entry, repeats included
        assert np.array_equal(tg[ix], gi[gp[r0]:gp[r1]]) and np.array_equal(cd[ix], deg[gi[gp[r0]:gp[r1]]])
        src = np.repeat(np.arange(r1 - r0), np.diff(ip))
        coef = (1.0 / np.sqrt((deg[r0:r1][src] * cd[ix].astype(np.int64)).astype(np.float32)).astype(np.float64)).astype(np.float32)
        got = np.zeros((r1 - r0, 5), np.float64)
        np.add.at(got, src, coef[:, None].astype(np.float64) * x[tg[ix]].astype(np.float64))
        close_mag(got, want[r0:r1], mag[r0:r1])


def _neediest_halo(gp, gi, world):
    """rows the neediest rank must receive: the distinct columns ITS rows list outside its own block"""
    from cuda_gcn_amd import model
    start, _ = model.partition(gp, world)
    out = []
    for r in range(world):
        r0, r1 = int(start[r]), int(start[r + 1])
        need = np.unique(gi[gp[r0]:gp[r1]])
        out.append(int(((need < r0) | (need >= r1)).sum()))
    return max(out)


def test_node_order_by_structure_on_a_non_symmetric_graph():
    """choose_node_order on a graph with one-way and repeated edges: the halo it reports for the ids as given and for the
    order it found is the halo counted here from what each rank's rows LIST (on a one-way graph, who lists a rank's rows
    is another number); forced, the order is a real renumbering; unforced, it renumbers only when that shrinks the halo"""
    from cuda_gcn_amd import model
    ds = irr.irregular_dataset()
    gp, gi, n = ds["g_indptr"], ds["g_indices"], ds["num_nodes"]
    deg = np.diff(gp)
    for world in (2, 3):
        for force in (False, True):
            c = model.choose_node_order(gp, gi, world, force=force)
            order = c["order"]
            assert np.array_equal(np.sort(order), np.arange(n))
            assert c["ids_recv_rows"] == _neediest_halo(gp, gi, world)
            inv = np.argsort(order).astype(np.int32)
            ngp = np.zeros(n + 1, np.int64)
            ngp[1:] = np.cumsum(deg[order])
            ngi = np.concatenate([inv[gi[gp[o]:gp[o + 1]]] for o in order]).astype(np.int32)
            assert c["new_recv_rows"] == _neediest_halo(ngp.astype(np.int32), ngi, world)
            if force:
                assert c["renumbered"] and not np.array_equal(order, np.arange(n))
            else:
                assert c["renumbered"] == (not np.array_equal(order, np.arange(n)))
                assert c["new_recv_rows"] <= c["ids_recv_rows"]
