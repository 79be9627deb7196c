"""Every producer of dropout decisions on the GPU, decision by decision, against the definition (tests/dropout_ref.py).

A decision is a pure function of (seed, epoch, stream index, thr16), and the multi-rank design rests on it: a rank that
passes elem_offset must draw what one GPU draws.  The function is written out in many kernels; each is reached here through
its entry point, every decision is recovered exactly from what the entry point returns, and required equal to
dropout_ref.keep (the materialised U16 >= thr16: no plane skipping, no recurrence), on thresholds of 0, 1, 2, 15 and 16 bit
planes, stream offsets that are whole Philox blocks, whole words or neither, that cross 2^32 and 2^39 (where the block
counter's high word turns non-zero) inside the array, seeds with a high word and epoch 0xFFFFFFFF.

  keep1            gcnhip_dropout_fwd / _fwd_2d (x = 1: mask == reference, output bit-equal to scale(p) or +0.0), the scalar
                   GraphSum kernel and graphsum_finalize_kernel (hub graph), spmm_csr_fwd / spmm_csc_bwd (drop_scale),
                   spmm_csr_fwd_q, spmm_csc_bwd_q
  keep4 / keep1    relu_dropout4 of the vector and bf16 GraphSum kernels: dims 4, 128, 256 (launch_vec<64>) and 41 in rows
                   of 44 at offsets that are multiples of 4 (keep4) and at 1, 33, 77 (the keep1 fallback)
  dropbits_kernel, dropbits_block_kernel, dropbits_pack_w_kernel, dropbits_cm_kernel, dropbits_bx_pack_w_kernel
                   dense X at p = 128: forward and weight gradient with gemm_bf16x3 off and on, the kernel named by
                   spmm_ref.gate and the block / flat choice by spmm_ref.keep_bits_by_block; K = 100 and 602 with m = 130
                   (rows start at arbitrary stream bits, a partial last chunk, the padded copy of X, a workgroup of 128 rows
                   and one of 2), K = 1433 with m = 100 (R = 91 rows per workgroup).  The products are decoded as
                   dropout_ref's docstring explains.
  invariance       rows [a, b) alone with elem_offset = base + a . dim give the bits of the whole matrix, base = 2^32 - 50

Not reachable: the keepv<VA> / keep1 branch of spmm_atb_kernel (dense_kernels.h).  Its only caller with dropout,
gcnhip_spmm_bwd on a dense X below the split-K plan, always passes the keep-bit array, so the branch that reads it runs;
that one is covered by the flat producers above.

Out of scope, noted from reading: relu_dropout4 and the finalizers form r * dim + col in int64, dropout_fwd_kernel indexes
with int64, dropbits_cm_body keeps only the offset INSIDE a workgroup's LDS image in 32 bits (at most 131072 bits).  No
32-bit overflow of an element index was found.

Mutants.  Each was applied to the kernels in a scratch state, built, run on an MI355X and discarded; none is committed.
(d) was run with (e); then (a), (b), (c), (e) together, each in a different producer, so the failing cases tell them apart.
  (a) keep_word: the counter's high word dropped, (uint32_t)(c >> 32) -> 0.  Run on the GPU: test_dropout_fwd_every_threshold
      fails at offsets 2^39 - 200 and 2^45 + 77 for all three seeds and passes at the other eleven; both GraphSum tests (all
      six widths), all four sparse kernels and the flat dense producer fail at the same two offsets only.
  (b) dropbits_cm_body: seed >> 32 -> 0.  Run on the GPU: test_dense_first_layer_products with gemm_bf16x3 = 2, forward
      (dropbits_bx_pack_w_kernel) and gradient (dropbits_cm_kernel), fails at every offset paired with seed 0xabcdef12345 or
      2^64 - 1 (43 to 48 of 72 cases per shape) and at none paired with seed 42.
  (c) dropbits_block_body: n_planes one short.  Run on the GPU: test_dense_first_layer_products with gemm_bf16x3 = 0 fails
      at the whole-block offsets 0, 128, 640, 2^32 - 128, 2^39 - 256: every threshold at K = 1433, and at K = 100 (13 000
      decisions) the thresholds of one or two planes and, by the numbers, some of 15 and 16 (one decision in 2^15 changes).
  (d) dropbits_block_body: and/or swapped.  Run on the GPU: the same six tests fail from their first case on (thr16 =
      0x8000 at offset 0 then keeps everything: 6 434 of 13 000 decisions differ at K = 100).
  (e) dropbits_kernel: << (31 - sh).  Run on the GPU: test_dense_first_layer_products with gemm_bf16x3 = 0 fails at offsets
      77 and 2^32 - 50 (no multiple of 32; five to eight of the eight thresholds, the rates near 0 and 1 can agree), and
      test_rows_alone_draw_what_the_whole_matrix_draws fails.
(a) to (c) on the CPU restatement alone: test_dropout_stream_cpu.py::test_the_table_notices_three_slips_of_the_recurrence.

Measured on an MI355X: 68 cases in 2.8 s, the slowest 0.44 s (test_graphsum_epilogue_on_a_split_row[256-256]; its reference
of 768 000 decisions per case is most of it).  Every decision of every case equals the reference as the kernels stand.
"""
import contextlib
import itertools

import numpy as np
import pytest

from tests import dropout_ref as D
from tests import spmm_ref as R
from tests.test_ops_gpu import hub_graph

pytestmark = pytest.mark.gpu

THR_BY_LABEL = {label: (t, p) for label, t, p in D.THR}


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def dev():
    from cuda_gcn_amd.ops import Device
    d = Device(0)
    yield d
    d.close()


@contextlib.contextmanager
def options(dev, **opts):
    old = {k: dev.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            dev.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            dev.set_option(k, v)


def spread(offsets, per_offset=2):
    """(offset, threshold entry, (seed, epoch)) cases: every offset, with thresholds and seeds dealt round so that each
    threshold of the table and each seed meets several offsets"""
    cases, k = [], 0
    for i, off in enumerate(offsets):
        for _ in range(per_offset):
            cases.append((off, D.THR[(5 * k) % len(D.THR)], D.SEEDS[(i + k) % len(D.SEEDS)]))
            k += 1
    return cases


def on_or_zero(out, keep, sc, what):
    """out is bit-equal to the scale where kept and +0.0 where dropped"""
    want = np.where(keep, np.float32(sc), np.float32(0))
    bad = np.flatnonzero(u32(out).ravel() != u32(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} elements differ, first at {bad[:5]}"


# ------------------------------------------------------------------------------------------------------- elementwise
N_FLAT = 5003
ROWS_2D, COLS_2D, LD_2D = 61, 82, 88


@pytest.mark.parametrize("seed,epoch", D.SEEDS)
@pytest.mark.parametrize("off", D.OFFSETS)
def test_dropout_fwd_every_threshold(dev, off, seed, epoch):
    """all of THR x OFFSETS x seeds, the flat form on 5003 elements and the strided one on 61 x 82 in rows of 88"""
    u = D.u16_cached(seed, epoch, off, N_FLAT)
    x2 = np.full((ROWS_2D, LD_2D), 7.0, np.float32)
    x2[:, :COLS_2D] = 1
    for label, t, p in D.THR:
        keep, sc = u >= t, D.scale(p)
        y, m = dev.dropout_fwd(np.ones(N_FLAT, np.float32), p, seed=seed, epoch=epoch, elem_offset=off)
        assert np.array_equal(m, keep.astype(np.int32)), (label, "mask")
        on_or_zero(y, keep, sc, label)
        k2 = keep[:ROWS_2D * COLS_2D]
        y2, m2 = dev.dropout_fwd_2d(x2, COLS_2D, p, seed=seed, epoch=epoch, elem_offset=off)
        assert np.array_equal(m2, k2.astype(np.int32)), (label, "mask, strided")
        on_or_zero(y2[:, :COLS_2D], k2.reshape(ROWS_2D, COLS_2D), sc, label + ", strided")
        assert np.all(y2[:, COLS_2D:] == 7.0), (label, "padding")


# ---------------------------------------------------------------------------------------------------------- GraphSum
GS_DIMS = [(4, 4), (128, 128), (256, 256), (41, 44), (5, 5), (41, 41)]     # the last two: rows not 16-byte aligned, scalar kernel
GS_ENTRIES = ("relu_dropout", "bits", "part", "ex", "bf16")


def gs_call(dev, entry, g, x, tab, dim, ld, p, seed, epoch, off):
    """-> (out [n, dim], mask words or None)"""
    kw = dict(p=p, seed=seed, epoch=epoch, elem_offset=off)
    if entry == "relu_dropout":
        return dev.graphsum_relu_dropout(g, x, True, ld=ld, **kw), None
    if entry == "bits":
        return dev.graphsum_relu_dropout_bits(g, x, True, ld=ld, **kw)
    if entry == "part":
        return dev.graphsum_part(g, x, ld=ld, relu_dropout=True, training=True, **kw), None
    if entry == "ex":
        if dim % 32 == 0:
            return dev.graphsum_ex(g, x, ld=ld, relu_dropout=True, training=True, want_bits=True, **kw)
        return dev.graphsum_ex(g, x, ld=ld, relu_dropout=True, training=True, **kw), None
    return dev.graphsum_bf16(g, tab, dim, ld_out=ld, relu_dropout=dict(training=1, **kw)), None


def words_of(flags):
    n, dim = flags.shape
    return np.packbits(flags.reshape(n, dim // 32, 32), axis=2, bitorder="little").view(np.uint32).reshape(n, dim // 32)


def gs_entries(dim, ld):
    return [e for e in GS_ENTRIES if e != "bits" or (dim % 32 == 0 and ld % 4 == 0)]


@pytest.mark.parametrize("dim,ld", GS_DIMS)
def test_graphsum_epilogue_on_self_loops(dev, dim, ld):
    """a graph of self-loops: the coefficient is exactly 1, so with x = 1 every output is scale(p) or +0.0, bit for bit"""
    n = 300
    g = dev.graph(np.arange(n + 1), np.arange(n))
    x = np.ones((n, dim), np.float32)
    tab = dev.to_bf16(x)
    assert np.all(u32(dev.graphsum_relu_dropout(g, x, False, 0.5, ld=ld)) == u32(np.float32(1)))
    for off, (label, t, p), (seed, epoch) in spread(D.OFFSETS):
        keep = D.keep_range(seed, epoch, off, n * dim, t).reshape(n, dim)
        for entry in gs_entries(dim, ld):
            what = f"{entry}, {label}, offset {off}, seed {seed:#x}"
            out, bits = gs_call(dev, entry, g, x, tab, dim, ld, p, seed, epoch, off)
            on_or_zero(out, keep, D.scale(p), what)
            if bits is not None:
                assert np.array_equal(bits, words_of(keep)), what + ": mask words"
    g.free()


HUB_CASES = [(off, (label,) + THR_BY_LABEL[label], D.SEEDS[i % 3]) for i, (off, label) in enumerate(
    ((0, "p0.3"), (33, "thr0x5555"), (77, "thr0xc000"), (2 ** 32 - 50, "p0.9"), (2 ** 39 - 200, "thr0x8000"), (2 ** 45 + 77, "p0.1")))]


@pytest.mark.parametrize("dim,ld", GS_DIMS)
def test_graphsum_epilogue_on_a_split_row(dev, dim, ld):
    """hub_graph: a row above the split length goes through the segment sums and graphsum_finalize_kernel.  x > 0, so an
    output is non-zero exactly where the decision was to keep"""
    gp, gi = hub_graph()
    n = gp.size - 1
    assert np.diff(gp).max() > 1024
    g = dev.graph(gp, gi)
    x = np.random.default_rng(dim).uniform(0.5, 1.5, (n, dim)).astype(np.float32)
    tab = dev.to_bf16(x)
    assert np.all(dev.graphsum_relu_dropout(g, x, False, 0.5, ld=ld) > 0)
    for off, (label, t, p), (seed, epoch) in HUB_CASES:
        keep = D.keep_range(seed, epoch, off, n * dim, t).reshape(n, dim)
        for entry in gs_entries(dim, ld):
            what = f"{entry}, {label}, offset {off}, seed {seed:#x}"
            out, bits = gs_call(dev, entry, g, x, tab, dim, ld, p, seed, epoch, off)
            bad = np.argwhere((out != 0) != keep)
            assert bad.size == 0, f"{what}: {len(bad)} decisions differ, first at {bad[:3].tolist()}"
            assert np.all(out >= 0)
            if bits is not None:
                assert np.array_equal(bits, words_of(keep)), what + ": mask words"
    g.free()


# ------------------------------------------------------------------------------------------------- sparse-X products
SPARSE_ROWS = {"fwd_csr<16,vec>": "sparse-fwd-vec-64-64", "fwd_csr_q<16>": "sparse-fwd-q-64-64",
               "bwd_csc<16,vec,1>": "sparse-bwd-vec-64-64-nw1", "bwd_csc_q<16,4>": "sparse-bwd-q-64-64-nw4"}
SPARSE_CASES = [(off, THR_BY_LABEL[label], D.SEEDS[i % 3])
                for i, (off, label) in enumerate(itertools.product((0, 77, 2 ** 32 - 50, 2 ** 39 - 200, 2 ** 45 + 77), ("p0.3", "thr0x8000", "thr0xfffe")))]


@pytest.mark.parametrize("name", list(SPARSE_ROWS))
def test_sparse_first_layer_products(dev, name):
    """one dispatch row of spmm_ref per kernel of spmm_sparse.h that draws decisions (keep1 at the stored element's CSR
    position; the weight gradient finds it through csc_pos)"""
    row = R.PATHS[SPARSE_ROWS[name]]
    assert row["name"] == name == R.gate_of(row, drop="philox.3@77") and row["p"] == 64
    fp, fi = R.sparse_layout()
    n, F, p = fp.size - 1, R.SPARSE["F"], row["p"]
    vals, t_of = D.sparse_fwd_operands(fp, p)
    if row["op"] == "bwd":
        vals = np.ones_like(vals)
    with options(dev, spmm_nw=row["nw"]):                        # read by gcnhip_feat_create
        f = dev.feat(fp, fi, vals, F)
    assert not f.dense
    douts = [d for _, d in D.sparse_bwd_douts(n, p)] if row["op"] == "bwd" else None
    with options(dev, **row["opts"]):
        for off, (t, rate), (seed, epoch) in SPARSE_CASES:
            keep, sc = D.keep_range(seed, epoch, off, int(fp[-1]), t), D.scale(rate)
            kw = dict(p_drop=rate, seed=seed, epoch=epoch, nnz_offset=off)
            if row["op"] == "fwd":
                got = D.decode_sparse_fwd(dev.spmm_fwd(f, np.ones((F, p), np.float32), **kw), fp, t_of, sc)
            else:
                got = D.decode_sparse_bwd([dev.spmm_bwd(f, d, **kw) for d in douts], fp, fi, p, sc)
            bad = np.flatnonzero(got != keep)
            assert bad.size == 0, f"{name}, thr16 {t:#x}, offset {off}, seed {seed:#x}: {bad.size} decisions differ, first at {bad[:5]}"
    f.free()


# -------------------------------------------------------------------------------------------------- dense-X products
DENSE_SHAPES = [(130, 100), (130, 602), (100, 1433)]            # (m, K)
# the table's offsets the issue names, and two whole-block ones at the crossings, where only the block producers run
DENSE_OFFSETS = (0, 77, 128, 640, 2 ** 32 - 50, 2 ** 32 - 128, 2 ** 39 - 200, 2 ** 39 - 256, 2 ** 45 + 77)
DENSE_THR = ("thr0x8000", "thr0xc000", "thr0x4000", "thr0xfffe", "thr0x0002", "p0.3", "thr0x5555", "thr0x0001")
# (op, gemm_bf16x3) -> (kernel gate() names, producer at a whole-block offset, producer elsewhere)
DENSE_PRODUCERS = {("fwd", 0): ("fwd_persist<bits>", "dropbits_pack_w_kernel", "dropbits_kernel"),
                   ("bwd", 0): ("bwd_t128<4,fast>", "dropbits_block_kernel", "dropbits_kernel"),
                   ("fwd", 2): ("fwd_bf16x3<bits>", "dropbits_bx_pack_w_kernel", "dropbits_bx_pack_w_kernel"),
                   ("bwd", 2): ("bwd_bf16x3<bits>", "dropbits_cm_kernel", "dropbits_cm_kernel")}


def dense_feat(dev, m, K, X):
    f = dev.feat((np.arange(m + 1) * K).astype(np.int32), np.tile(np.arange(K, dtype=np.int32), m), X.ravel(), K)
    assert f.dense
    return f


def dense_keep(dev, f, op, m, K, W, dout, rate, seed, epoch, off):
    kw = dict(p_drop=rate, seed=seed, epoch=epoch, nnz_offset=off)
    if op == "fwd":
        return D.decode_fwd(dev.spmm_fwd(f, W, **kw), K, D.scale(rate))
    return D.decode_bwd(dev.spmm_bwd(f, dout, **kw), m, D.scale(rate))


@pytest.mark.parametrize("op,bx", list(DENSE_PRODUCERS))
@pytest.mark.parametrize("m,K", DENSE_SHAPES)
def test_dense_first_layer_products(dev, m, K, op, bx):
    name, by_block, elsewhere = DENSE_PRODUCERS[(op, bx)]
    row = R._row(op, "dense", m, K, 128, name, opts=dict(gemm_bf16x3=bx), drop="philox.3@77")
    assert R.gate_of(row) == name and R.has_pad(True, K)
    assert {D.n_planes(THR_BY_LABEL[l][0]) for l in DENSE_THR} == {1, 2, 15, 16}
    seen, failed = set(), []
    X, W, dout = D.dense_operands(m, K)
    f = dense_feat(dev, m, K, X)
    with options(dev, gemm_bf16x3=bx):
        for i, off in enumerate(DENSE_OFFSETS):
            seed, epoch = D.SEEDS[i % 3]
            seen.add(by_block if R.keep_bits_by_block(dict(p=0.5, off=off)) else elsewhere)
            for label in DENSE_THR:
                t, rate = THR_BY_LABEL[label]
                keep = D.keep_range(seed, epoch, off, m * K, t).reshape(m, K)
                got = dense_keep(dev, f, op, m, K, W, dout, rate, seed, epoch, off)
                bad = np.argwhere(got != keep)
                if bad.size:
                    failed.append(f"{label} @ {off} seed {seed:#x}: {len(bad)} differ, first at {bad[0].tolist()}")
    assert not failed, f"{name}: {len(failed)} of {len(DENSE_OFFSETS) * len(DENSE_THR)} cases fail: " + "; ".join(failed)
    assert seen == {by_block, elsewhere}
    f.free()


# -------------------------------------------------------------------------------------------------------- invariance
BASE = 2 ** 32 - 50


def test_rows_alone_draw_what_the_whole_matrix_draws(dev):
    """what a rank relies on: rows [a, b) with elem_offset = base + a . dim give the bits of the one-GPU run.  The index
    passes 2^32 inside the whole matrix, before row a in one case and inside [a, b) in the other"""
    seed, epoch = D.SEEDS[1]
    t, rate = THR_BY_LABEL["p0.3"]
    for a, b in ((37, 101), (0, 3)):
        # elementwise, strided
        x2 = np.ones((ROWS_2D, LD_2D), np.float32)
        _, whole = dev.dropout_fwd_2d(x2, COLS_2D, rate, seed=seed, epoch=epoch, elem_offset=BASE)
        b2 = min(b, ROWS_2D)
        _, part = dev.dropout_fwd_2d(x2[a:b2], COLS_2D, rate, seed=seed, epoch=epoch, elem_offset=BASE + a * COLS_2D)
        assert np.array_equal(part, whole[a * COLS_2D:b2 * COLS_2D])
        assert np.array_equal(whole != 0, D.keep_range(seed, epoch, BASE, ROWS_2D * COLS_2D, t))
        # GraphSum, self-loops
        n, dim = 130, 128
        g, gpart = dev.graph(np.arange(n + 1), np.arange(n)), dev.graph(np.arange(b - a + 1), np.arange(b - a))
        kw = dict(p=rate, seed=seed, epoch=epoch)
        whole = dev.graphsum_relu_dropout(g, np.ones((n, dim), np.float32), True, elem_offset=BASE, **kw)
        part = dev.graphsum_relu_dropout(gpart, np.ones((b - a, dim), np.float32), True, elem_offset=BASE + a * dim, **kw)
        assert np.array_equal(u32(part), u32(whole[a:b]))
        on_or_zero(whole, D.keep_range(seed, epoch, BASE, n * dim, t).reshape(n, dim), D.scale(rate), "whole")
        g.free()
        gpart.free()
        # dense first-layer product, both kernel families
        m, K = 130, 100
        X, W, dout = D.dense_operands(m, K)
        f, fpart = dense_feat(dev, m, K, X), dense_feat(dev, b - a, K, X[a:b])
        for bx in (0, 2):
            with options(dev, gemm_bf16x3=bx):
                whole = dense_keep(dev, f, "fwd", m, K, W, dout, rate, seed, epoch, BASE)
                part = dense_keep(dev, fpart, "fwd", b - a, K, W, dout[a:b], rate, seed, epoch, BASE + a * K)
                assert np.array_equal(part, whole[a:b]), bx
                assert np.array_equal(whole, D.keep_range(seed, epoch, BASE, m * K, t).reshape(m, K)), bx
        f.free()
        fpart.free()
