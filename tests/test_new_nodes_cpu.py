"""New nodes attached to a dataset's graph, host side (host/attach.h, model.new_node_rows): the stored rows and their
coefficients against a numpy construction of the augmented CSR, every refusal with its message, and the new entry points in
the binding tables and headers.  No GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The per-edge coefficient is (float)(1 / sqrtf((float)(len . len))): the product is exact in f32 below 2^24 (here it is), sqrtf
# rounds once (relative 2^-24), the division is done in double and narrowed once (2^-24): 2 . 2^-24 against the float64 value,
# and one more 2^-24 of slack for the float64 reference's own narrowing in the comparison.
COEF_RTOL = 3 * 2.0 ** -24


def base_graph(n=12, seed=0):
    """a small dataset graph as the loader stores it: self loop first, then 0-4 listed ids (repeats and one-way entries included)"""
    rng = np.random.default_rng(seed)
    rows = [[i] + list(rng.integers(0, n, rng.integers(0, 5))) for i in range(n)]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return indptr, np.concatenate(rows).astype(np.int32)


def augmented(g_indptr, lists):
    """the augmented CSR's new rows in numpy: (ptr, col, len of every node old and new)"""
    n, m = len(g_indptr) - 1, len(lists)
    rows = [[n + i] + list(l) for i, l in enumerate(lists)]
    length = np.concatenate([np.diff(g_indptr), [len(r) for r in rows]]).astype(np.int64)
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.array([c for r in rows for c in r], np.int64)
    return ptr, col, length


def lists_to_csr(lists):
    ptr = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    ids = np.array([c for l in lists for c in l], np.int32)
    return ptr, ids


N = 12
CASES = {
    "no neighbour": [[]],
    "m = 1": [[3, 0, 7]],
    "repeats": [[5, 5, 5, 2], [2, 2]],
    "self listed again": [[N + 0, 1], [N + 1, N + 1]],
    "new-to-new, also to a later one": [[N + 2, 0], [N + 0], [N + 1, N + 0, 4]],
    "unsorted": [[9, 1, 11, 0, 4, 2], [N + 1, 3, N + 0, 3]],
    "mixed": [[], [N + 3, N + 3, 1], [0], [N + 0, N + 1, N + 2, N + 3, 11, 11], []],
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("factored", [False, True])
def test_rows_and_coefficients_match_the_augmented_csr(case, factored):
    from cuda_gcn_amd.model import new_node_rows
    gp, _ = base_graph(N)
    lists = CASES[case]
    nbr_ptr, nbr_ids = lists_to_csr(lists)
    got = new_node_rows(gp, nbr_ptr, nbr_ids, factored=factored)
    ptr, col, length = augmented(gp, lists)
    m = len(lists)
    assert got["ptr"].dtype == np.int32 and got["col"].dtype == np.int32 and got["coef"].dtype == np.float32 and got["len"].dtype == np.int32
    assert np.array_equal(got["ptr"], ptr) and np.array_equal(got["col"], col)          # self loop first, then listed order
    assert np.array_equal(got["len"], length[N:])
    row_of = np.repeat(np.arange(m), np.diff(ptr))
    lv = length[N + row_of].astype(np.float64)
    want = 1.0 / np.sqrt(lv) if factored else 1.0 / np.sqrt(lv * length[col].astype(np.float64))
    assert np.all(np.abs(got["coef"].astype(np.float64) - want) <= COEF_RTOL * want), case


def test_wide_degree_product_is_formed_in_64_bits():
    """a new node listing 70 000 ids of a dataset whose hub row has 70 000 entries: the product 70 001 . 70 000 is past 2^31"""
    from cuda_gcn_amd.model import new_node_rows
    gp = np.array([0, 70000, 70001], np.int32)
    ids = np.zeros(70000, np.int32)
    got = new_node_rows(gp, [0, 70000], ids)
    want = 1.0 / np.sqrt(70001.0 * 70000.0)
    assert np.all(np.abs(got["coef"][1:].astype(np.float64) - want) <= COEF_RTOL * want)
    assert abs(float(got["coef"][0]) - 1.0 / 70001.0) <= COEF_RTOL / 70001.0


def test_refusals_carry_their_message():
    from cuda_gcn_amd.model import new_node_rows, GcnHostError
    gp, _ = base_graph(N)
    with pytest.raises(GcnHostError, match=r"nbr_ptr\[0\] = 1, not 0"):
        new_node_rows(gp, [1, 2], [0, 0])
    with pytest.raises(GcnHostError, match="nbr_ptr decreases at new node 1"):
        new_node_rows(gp, [0, 2, 1], [0, 0])
    with pytest.raises(GcnHostError, match=rf"id {N + 2} is outside \[0, {N + 2}\)"):
        new_node_rows(gp, [0, 1, 2], [0, N + 2])
    with pytest.raises(GcnHostError, match=r"id -1 is outside"):
        new_node_rows(gp, [0, 1], [-1])
    with pytest.raises(GcnHostError, match="m = -1 is negative"):
        new_node_rows(gp, [0], [], m=-1)
    with pytest.raises(GcnHostError, match=r"2147483648 stored entries: more than 2\^31 - 1"):
        new_node_rows(gp, [0, 2 ** 31 - 1], [0])
    ok = new_node_rows(gp, [0], [], m=0)                                          # no new node: empty arrays
    assert ok["ptr"].tolist() == [0] and ok["col"].size == 0 and ok["coef"].size == 0 and ok["len"].size == 0


def test_names_in_the_binding_tables_and_headers():
    from cuda_gcn_amd import _lib, ops, model
    drv = open(os.path.join(ROOT, "include", "gcnhip_driver.h")).read()
    host_h = open(os.path.join(ROOT, "include", "gcnhost.h")).read()
    hip, host = _lib.gcnhip(), _lib.gcnhost()
    assert "gcnhip_attach_gather" in _lib.GCNHIP_SYMBOLS and hasattr(hip, "gcnhip_attach_gather") and re.search(r"\bint gcnhip_attach_gather\(", drv)
    for n in ("gcnhost_attach_rows", "gcnhost_model_predict_new"):
        assert n in _lib.GCNHOST_SYMBOLS and hasattr(host, n) and re.search(rf"\bint {n}\(", host_h)
    assert hasattr(ops.Device, "attach_gather") and hasattr(model.HipGCNModel, "predict_new_nodes") and hasattr(model, "new_node_rows")
