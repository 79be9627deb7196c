"""tests/spmm_ref.py before a GPU sees it: the float64 restatements against the oracle's SparseMatmul and against the dense
product, the dropout identity, and the table of paths against gate()."""
import itertools

import numpy as np
import pytest

from tests import spmm_ref as R
from tests.test_ops_gpu import close_mag, philox_keep, thr_of


def _dense_of(fp, fi, vals, F):
    x = np.zeros((fp.size - 1, F))
    x[R.row_of(fp), fi] = np.asarray(vals, np.float64)
    return x


@pytest.fixture(scope="module")
def small():
    """a ragged CSR matrix with empty rows and columns, and a dense one"""
    rng = np.random.default_rng(0)
    fp, fi = R.sparse_layout(n=300, F=40, per_row=6)
    sv = rng.standard_normal(fi.size).astype(np.float32)
    dp, _ = R.dense_layout(37, 21)
    dv = rng.standard_normal(37 * 21).astype(np.float32)
    return dict(sparse=(fp, fi, sv, 40), dense=(dp, None, dv, 21))


@pytest.mark.parametrize("layout", ["sparse", "dense"])
@pytest.mark.parametrize("p", [1, 7, 16, 130])
def test_restatements_against_the_oracle_and_the_dense_product(oracle, small, layout, p):
    fp, fi, vals, F = small[layout]
    n = fp.size - 1
    idx = fi if fi is not None else np.tile(np.arange(F, dtype=np.int32), n)
    rng = np.random.default_rng(p)
    w = rng.standard_normal((F, p)).astype(np.float32)
    dout = rng.standard_normal((n, p)).astype(np.float32)
    x = _dense_of(fp, idx, vals, F)
    want, mag = R.fwd_ref(fp, fi, vals, w)
    close_mag(oracle.spmm_fwd(fp, idx, vals, w, p), want, mag)
    assert np.allclose(want, x @ w.astype(np.float64), rtol=1e-13, atol=1e-13) and np.allclose(mag, np.abs(x) @ np.abs(w.astype(np.float64)), rtol=1e-13)
    assert np.array_equal(R.fwd_ref(fp, fi, vals, w, relu=True)[0], np.maximum(want, 0))
    want, mag = R.bwd_ref(fp, fi, vals, dout, F)
    close_mag(oracle.spmm_bwd(fp, idx, vals, dout, F, p), want, mag)
    assert np.allclose(want, x.T @ dout.astype(np.float64), rtol=1e-13, atol=1e-13) and np.allclose(mag, np.abs(x).T @ np.abs(dout.astype(np.float64)), rtol=1e-13)
    if layout == "sparse":
        assert np.all(want[-3:] == 0) and np.all(R.fwd_ref(fp, fi, vals, w)[0][5] == 0)       # empty columns, an empty row
    # a CSR layout that happens to be dense gives the dense answer
    if fi is None:
        a, b = R.fwd_ref(fp, idx, vals, w), R.fwd_ref(fp, None, vals, w)
        assert np.allclose(a[0], b[0], rtol=1e-13, atol=1e-13) and np.allclose(a[1], b[1], rtol=1e-13)


def test_blocks_of_a_csr_reference_change_nothing(small, monkeypatch):
    fp, fi, vals, F = small["sparse"]
    w = np.random.default_rng(1).standard_normal((F, 9)).astype(np.float32)
    dout = np.random.default_rng(2).standard_normal((fp.size - 1, 9)).astype(np.float32)
    a, b = R.fwd_ref(fp, fi, vals, w), R.bwd_ref(fp, fi, vals, dout, F)
    monkeypatch.setattr(R, "BLOCK", 9 * 50)                 # blocks that end inside rows and columns
    for x, y in zip(a + b, R.fwd_ref(fp, fi, vals, w) + R.bwd_ref(fp, fi, vals, dout, F)):
        assert np.allclose(x, y, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("layout", ["sparse", "dense"])
@pytest.mark.parametrize("drop", [k for k in R.DROPS if k != "none"])
def test_dropout_is_the_product_on_dropped_values(small, layout, drop):
    fp, fi, vals, F = small[layout]
    rng = np.random.default_rng(3)
    w = rng.standard_normal((F, 5)).astype(np.float32)
    dout = rng.standard_normal((fp.size - 1, 5)).astype(np.float32)
    mask = rng.integers(0, 2, vals.size).astype(np.uint8)
    d = R.DROPS[drop]
    keep = R.keep_of(d, vals.size, mask)
    if not d.get("mask"):
        assert np.array_equal(keep, philox_keep(R.SEED, R.EPOCH, np.arange(vals.size, dtype=np.uint64) + np.uint64(d["off"]), thr_of(d["p"])))
        assert abs(1 - keep.mean() - d["p"]) < 0.1                                           # the rate is the stream's
    scale = R.drop_scale(d["p"])
    pre = np.where(keep, vals.astype(np.float64) * float(scale), 0.0)                         # float64: no rounding of the scaled value
    for got, ref in ((R.fwd_ref(fp, fi, vals, w, keep, scale), R.fwd_ref(fp, fi, pre, w)),
                     (R.bwd_ref(fp, fi, vals, dout, F, keep, scale), R.bwd_ref(fp, fi, pre, dout, F))):
        # (pre goes through float32 inside the restatement: one rounding per term)
        assert np.all(np.abs(got[0] - ref[0]) <= R.EPS * got[1] + 1e-30) and np.allclose(got[1], ref[1], rtol=1e-6)


def test_fused_bound_is_the_two_products_bound():
    rng = np.random.default_rng(4)
    X, w1, w2 = rng.standard_normal((20, 33)), rng.standard_normal((33, 128)), rng.standard_normal((128, 7))
    want, bound = R.fused_ref(X, w1, w2)
    x, a, b = (t.astype(np.float32).astype(np.float64) for t in (X, w1, w2))
    h = x @ a
    assert np.allclose(want, np.maximum(h, 0) @ b, rtol=1e-13)
    assert np.allclose(bound, 8 * R.EPS * ((np.abs(x) @ np.abs(a) + np.maximum(h, 0)) @ np.abs(b)), rtol=1e-12)
    # the float32 two-step product is inside it
    h32 = np.maximum(X.astype(np.float32) @ w1.astype(np.float32), 0)
    assert np.all(np.abs((h32 @ w2.astype(np.float32)).astype(np.float64) - want) <= bound)


def test_the_table_names_the_path_the_gate_takes():
    for pid, row in R.PATHS.items():
        assert R.gate_of(row) == row["name"], (pid, R.gate_of(row))
    named = {r["name"] for r in R.PATHS.values()} - {"NOT_AVAILABLE"}
    assert named == R.every_name(), (sorted(R.every_name() - named), sorted(named - R.every_name()))
    # ... and gate() has no name outside that list, whatever it is asked
    seen = set()
    dense_shapes = [(289, F) for F in (33, 34, 40, 64, 65, 70, 72, 96, 128, 2656, 2657, 2720, 2721, 4096, 4097)]
    for (n, F), p, ld_pad, own, va, ia, oa, drop, bx, co in itertools.product(dense_shapes, (3, 16, 29, 41, 64, 65, 100, 128, 256), (0, 1, 4),
                                                                              (True, False), (16, 8, 4), (16, 4), (16, 4), ("none", "mask", "philox.5@0"),
                                                                              (0, 1, 2), (0, 1)):
        for op in ("fwd", "bwd"):
            seen.add(R.gate(op, True, n, F, n * F, p, p + ld_pad, own, va, ia, oa, R.DROPS[drop], True, bx, co))
        seen.add(R.gate("fwd", True, n, F, n * F, p, p + ld_pad, own, va, ia, oa, R.DROPS[drop], True, bx, co,
                        fused=dict(p2=7, ld_z0=8, ld_w2=8, z_align=oa)))
    for p, ld_pad, own, ia, general, slices, nw, (F, nnz) in itertools.product(range(1, 300), (0, 1, 4), (True, False), (16, 4), (-1, 0, 1), (0, 1),
                                                                               (1, 4, 16), ((90, 35000), (16500, 35000), (90, 300000))):
        ld = (p + 3) // 4 * 4 if ld_pad == 4 else p + ld_pad
        for op in ("fwd", "bwd"):
            seen.add(R.gate(op, False, 4400, F, nnz, p, ld, own, 16, ia, 16, None, True, 2, 0, general, slices, nw))
    assert seen - {"NOT_AVAILABLE"} <= R.every_name(), sorted(seen - R.every_name())
    assert R.every_name() <= seen, sorted(R.every_name() - seen)


def test_the_gate_at_the_edges_the_issue_names():
    g = lambda K, **kw: R.gate("fwd", True, 289, K, 289 * K, 128, 128, **kw)
    z = dict(p2=41, ld_z0=44, ld_w2=44)
    # 83 / 85 / 128 chunks of 32 columns: what 2 MiB of packed W holds in each form
    assert (2 * 83 * R.BX_BH_BYTES + R.BX_W2_BYTES <= R.WPACK_BYTES < 2 * 84 * R.BX_BH_BYTES + R.BX_W2_BYTES) and R.K_FUSED == 83 * 32
    assert (2 * 85 * R.BX_BH_BYTES <= R.WPACK_BYTES < 2 * 86 * R.BX_BH_BYTES) and R.K_BF16X3 == 85 * 32
    assert 128 * R.PERSIST_CHUNK_BYTES == R.WPACK_BYTES and R.K_PERSIST == 128 * 32
    assert g(2656, fused=z) == "fwd_bf16x3<z0>" and g(2657, fused=z) == "NOT_AVAILABLE" and g(2720, fused=z) == "NOT_AVAILABLE"
    assert g(2657) == g(2720) == "fwd_bf16x3" and g(2721) == g(4096) == "fwd_persist" and g(4097) == "fwd_t128w8"
    assert g(2721, corun=1) == "fwd_t128w8" and g(96, bx=1, corun=1) == "fwd_t128w8" and g(96, bx=2, corun=1) == "fwd_bf16x3"
    # keep words: chunk-major for bf16x3; whole Philox blocks only from a stream offset that is a multiple of 128
    assert R.keep_bits_by_block(R.DROPS["philox.5@640"]) and not R.keep_bits_by_block(R.DROPS["philox.3@77"]) and not R.keep_bits_by_block(R.DROPS["mask"])
    assert g(96, drop=R.DROPS["mask"]) == "fwd_bf16x3<bits>" and g(96, drop=R.DROPS["mask"], keep_bits=False) == "refused"
    # the padded copy: dense, K >= 64, K not a multiple of 128
    assert [R.has_pad(True, K) for K in (63, 64, 96, 128, 130)] == [False, True, True, False, True] and not R.has_pad(False, 96)
    # the split-K plan fills the chip twice
    assert R.dense_bwd_plan(True, 289, 96, 128) == (32, 10) and R.dense_bwd_plan(True, 100000, 602, 128) == (992, 101)
    assert R.dense_bwd_plan(True, 289, 96, 256, n_cu=256)[1] == 10 and R.dense_bwd_plan(True, 289, 40, 128) is None and R.dense_bwd_plan(True, 289, 96, 64) is None
    # narrow rows: by size, or always under spmm_general = -1, never under 1; the CSC copy exists only of the object's own values
    s = lambda **kw: R.gate("fwd", False, 4400, 90, kw.pop("nnz", 35000), 16, 16, **kw)
    assert s() == "fwd_csr<4,vec>" and s(nnz=R.NARROW_MIN_NNZ) == "fwd_csr_q<4>" and s(general=-1) == "fwd_csr_q<4>" and s(general=1, nnz=10 ** 6) == "fwd_csr<4,vec>"
    assert R.gate("bwd", False, 4400, 90, 35000, 16, 16, general=-1, own_vals=False, nw=4) == "bwd_csc<4,vec,4>"
