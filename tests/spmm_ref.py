"""One first-layer product in float64, the choice of its kernel as a pure function, and the table of paths.

fwd_ref / bwd_ref / fused_ref restate one call of gcnhip_spmm_fwd(_relu), gcnhip_spmm_bwd and gcnhip_spmm_fwd_relu_matmul;
gate() restates spmm_fwd_impl, dense_bwd_part and gcnhip_spmm_bwd (csrc/spmm.hip): the name of the kernel each launches.
PATHS gives every kernel name a shape that reaches it.  test_spmm_dispatch_cpu.py proves all three before a GPU sees them,
test_spmm_dispatch_gpu.py holds every row of the table to the float64 product.

A layout is (fp, fi): CSR row pointers and column indices; fi = None says "every row stores all F columns in order", the
dense layout (plan::dense_layout), and the product is then a float64 matmul.  CSR products are accumulated row-wise in
blocks of at most BLOCK products, never densified.

NT = 8 of spmm_dense_fwd_kernel is missing from the table on purpose: the p <= 64 branch sees at most four 16-column
tiles, so spmm_fwd_impl cannot name it.
"""
import itertools

import numpy as np

EPS = float(np.finfo(np.float32).eps)
BLOCK = 1 << 21                     # products (stored value x columns) formed at once by a CSR reference

# csrc/common.h, dense_bf16x3.h, dense_persist.h, spmm.hip
WPACK_BYTES = 2 << 20
BX_BH_BYTES, BX_W2_BYTES, BX_BITS_LDS_WORDS = 12288, 49152, 4096
PERSIST_CHUNK_BYTES = 4096 * 4
NARROW_MIN_NNZ = 262144
SLICE_W_BYTES = 4 << 20
K_FUSED, K_BF16X3, K_PERSIST = 2656, 2720, 4096          # the last K each form takes, as the three limits above give them
N_CU = 256                                               # compute units of an MI355X (the split-K plan reads the device's count)


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------- float64
def row_of(fp):
    fp = np.asarray(fp, np.int64)
    return np.repeat(np.arange(fp.size - 1), np.diff(fp))


def dropped(vals, keep=None, scale=1):
    """float64 X~: kept values times the f32 scale, dropped ones zero"""
    v = np.asarray(vals, np.float32).astype(np.float64).ravel()
    if keep is None:
        return v
    return np.where(np.asarray(keep).ravel().astype(bool), v * float(np.float32(scale)), 0.0)


def _segment_sums(keys, n_out, width, products):
    """out[k] += products(lo, hi)[i - lo] for the elements i of [lo, hi) with keys[i] == k; keys ascending"""
    out = np.zeros((n_out, width))
    step = max(1, BLOCK // max(width, 1))
    for lo in range(0, keys.size, step):
        hi = min(keys.size, lo + step)
        k = keys[lo:hi]
        starts = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
        out[k[starts]] += np.add.reduceat(products(lo, hi), starts, axis=0)
    return out


def fwd_ref(fp, fi, vals, w, keep=None, scale=1, relu=False):
    """-> (want, mag) float64 [n_rows, p]: X~ . w and |X~| . |w|"""
    w64 = np.asarray(w, np.float32).astype(np.float64)
    v = dropped(vals, keep, scale)
    n = np.asarray(fp).size - 1
    if fi is None:
        x = v.reshape(n, -1)
        want, mag = x @ w64, np.abs(x) @ np.abs(w64)
    else:
        fi = np.asarray(fi, np.int64)
        rows = row_of(fp)
        want = _segment_sums(rows, n, w64.shape[1], lambda lo, hi: v[lo:hi, None] * w64[fi[lo:hi]])
        mag = _segment_sums(rows, n, w64.shape[1], lambda lo, hi: np.abs(v[lo:hi, None] * w64[fi[lo:hi]]))
    return (np.maximum(want, 0.0) if relu else want), mag


def bwd_ref(fp, fi, vals, dout, F, keep=None, scale=1):
    """-> (want, mag) float64 [F, p]: X~^T . dout and |X~|^T . |dout|"""
    d64 = np.asarray(dout, np.float32).astype(np.float64)
    v = dropped(vals, keep, scale)
    n = np.asarray(fp).size - 1
    if fi is None:
        x = v.reshape(n, F)
        return x.T @ d64, np.abs(x).T @ np.abs(d64)
    fi = np.asarray(fi, np.int64)
    order = np.argsort(fi, kind="stable")                  # a column's entries in row order, as the CSC view keeps them
    cols, rows, v = fi[order], row_of(fp)[order], v[order]
    want = _segment_sums(cols, F, d64.shape[1], lambda lo, hi: v[lo:hi, None] * d64[rows[lo:hi]])
    mag = _segment_sums(cols, F, d64.shape[1], lambda lo, hi: np.abs(v[lo:hi, None] * d64[rows[lo:hi]]))
    return want, mag


def fused_ref(X, w1, w2):
    """-> (want, bound): relu(X . w1) . w2 in float64, and the bound of test_both_layers_products_in_one_evaluation_launch — the
    hidden layer's error enters the second product: 8 eps ((|X| . |w1| + relu(H)) . |w2|)"""
    X, w1, w2 = (np.asarray(t, np.float32).astype(np.float64) for t in (X, w1, w2))
    H = X @ w1
    magH = np.abs(X) @ np.abs(w1)
    want = np.maximum(H, 0) @ w2
    return want, 8 * EPS * ((magH + np.maximum(H, 0)) @ np.abs(w2)) + 1e-30


# ---------------------------------------------------------------------------------------------------------- dropout
SEED, EPOCH = 0x5eed1234abc, 9
DROPS = {"none": None, "mask": dict(p=0.5, mask=True), "philox.5@0": dict(p=0.5, off=0), "philox.5@640": dict(p=0.5, off=128 * 5),
         "philox.3@77": dict(p=0.3, off=77)}


def drop_scale(p):
    return np.float32(1) / (np.float32(1) - np.float32(p))


def keep_of(drop, nnz, mask=None):
    """the keep decisions (bool [nnz]) of a DROPS entry: the injected mask, or the documented Philox stream"""
    if drop is None:
        return None
    if drop.get("mask"):
        return np.asarray(mask).astype(bool)
    from tests.test_ops_gpu import philox_keep, thr_of
    return philox_keep(SEED, EPOCH, np.arange(nnz, dtype=np.uint64) + np.uint64(drop["off"]), thr_of(drop["p"]))


def drop_kwargs(drop, mask=None):
    """the wrapper arguments of a DROPS entry"""
    if drop is None:
        return {}
    if drop.get("mask"):
        return dict(p_drop=drop["p"], keep_mask=np.asarray(mask, np.uint8))
    return dict(p_drop=drop["p"], seed=SEED, epoch=EPOCH, nnz_offset=drop["off"])


# ------------------------------------------------------------------------------------------------------------- gate
def has_pad(dense, n_cols):
    """gcnhip_feat_create keeps a second, zero-padded copy of a dense X whose rows are not whole 128-column tiles"""
    return bool(dense and n_cols % 128 != 0 and n_cols >= 64)


def x_vec_width(n_cols, align):
    return 4 if n_cols % 4 == 0 and align % 16 == 0 else 2 if n_cols % 2 == 0 and align % 8 == 0 else 1


def keep_bits_by_block(drop):
    return drop is not None and not drop.get("mask") and (drop["off"] & 127) == 0


def keep_bits_cm_fit(dense, keep_bits, n_cols):
    return bool(dense and keep_bits and n_cols // 32 + 16 <= BX_BITS_LDS_WORDS)


def lanes(units):
    return next(l for l in (1, 2, 4, 8, 16, 32, 64) if units <= l or l == 64)


def dense_bwd_plan(dense, n_rows, n_cols, p, n_cu=N_CU):
    """-> (rows per split, splits) or None"""
    if not (dense and p > 64 and n_cols >= 64):
        return None
    kt, pt = cdiv(n_cols, 128), cdiv(p, 128)
    S = max(1, (2 * n_cu) // (kt * pt))
    rps = max(32, cdiv(cdiv(n_rows, S), 32) * 32)
    return rps, cdiv(n_rows, rps)


def _x_operand(dense, n_cols, own_vals, vals_align):
    """(vector width of the X loads, row stride) of a dense product"""
    if own_vals and has_pad(dense, n_cols):
        return 4, cdiv(n_cols, 128) * 128
    return x_vec_width(n_cols, 16 if own_vals else vals_align), n_cols


def gate(op, dense, n_rows, n_cols, nnz, p, ld_in, own_vals=True, vals_align=16, in_align=16, out_align=16, drop=None, keep_bits=True,
         bx=2, corun=0, general=0, slices=1, nw=1, fused=None, n_cu=N_CU):
    """the kernel one call launches.  op: "fwd" (gcnhip_spmm_fwd / _fwd_relu; with fused = dict(p2, ld_z0, ld_w2, z_align):
    gcnhip_spmm_fwd_relu_matmul) or "bwd" (gcnhip_spmm_bwd, and every gcnhip_spmm_bwd_part of its plan).  ld_in / in_align: row
    stride and address alignment in bytes of w (fwd) or dout (bwd); out_align: of out; vals_align: of an external value
    array.  keep_bits: the object has a keep-bit array (an aggregated one has none).  bx, corun, general, slices: the
    context's gemm_bf16x3, co-run mark, spmm_general and spmm_slices; nw: the object's waves per column task.
    "NOT_AVAILABLE" and "refused" launch nothing."""
    on = drop is not None
    if op == "fwd":
        if fused is not None and not (dense and p == 128):
            return "NOT_AVAILABLE"
        if dense and p > 64:
            if on and not keep_bits:
                return "refused"
            vx, ldx = _x_operand(dense, n_cols, own_vals, vals_align)
            fast = vx == 4 and ldx % 4 == 0 and cdiv(n_cols, 32) * 32 <= ldx and ld_in % 4 == 0 and p % 128 == 0 and in_align % 16 == 0
            chunks = cdiv(n_cols, 32)
            if fused is not None:
                z = fused
                if not (fast and bx and not on and 1 <= z["p2"] <= 64 and z["ld_z0"] % 4 == 0 and z["ld_z0"] >= z["p2"] and z["ld_w2"] >= z["p2"]
                        and z.get("z_align", 16) % 16 == 0 and chunks * 2 * BX_BH_BYTES + BX_W2_BYTES <= WPACK_BYTES):
                    return "NOT_AVAILABLE"
            if (fast and p == 128 and bx and (not on or keep_bits_cm_fit(dense, keep_bits, n_cols))
                    and (fused is not None or ((bx >= 2 or not corun) and out_align % 16 == 0)) and chunks * 2 * BX_BH_BYTES <= WPACK_BYTES):
                return "fwd_bf16x3<z0>" if fused is not None else "fwd_bf16x3<bits>" if on else "fwd_bf16x3"
            if fast and p == 128 and not corun and out_align % 16 == 0 and chunks * PERSIST_CHUNK_BYTES <= WPACK_BYTES:
                return "fwd_persist<bits>" if on else "fwd_persist"
            return "fwd_t128w8" if fast else f"fwd_t128<{vx}>"
        if dense:
            if on and not keep_bits:
                return "refused"
            vx, _ = _x_operand(dense, n_cols, own_vals, vals_align)
            nt = cdiv(p, 16)
            return f"fwd_dense<{8 if nt > 4 else 4 if nt > 2 else nt},{vx}>"
        vec = ld_in % 4 == 0 and in_align % 16 == 0
        units = cdiv(p, 4) if vec else p
        if vec and slices != 0 and p % 32 == 0 and p // 32 in (2, 4, 8) and n_cols * ld_in * 4 > SLICE_W_BYTES and n_rows >= 8 * 64:
            return "fwd_csr_sliced"
        if vec and units <= 16 and nnz * 4 < 0x7FFFFFFF and general <= 0 and (nnz >= NARROW_MIN_NNZ or general < 0):
            return f"fwd_csr_q<{lanes(units)}>"
        return f"fwd_csr<{lanes(units)},{'vec' if vec else 'scalar'}>"
    assert op == "bwd" and fused is None
    plan = dense_bwd_plan(dense, n_rows, n_cols, p, n_cu)
    if plan:
        if on and not keep_bits:
            return "refused"
        kt = cdiv(n_cols, 128)
        padded = own_vals and has_pad(dense, n_cols)
        if (bx and (bx >= 2 or not corun) and p == 128 and padded and plan[0] % 16 == 0 and ld_in % 4 == 0 and in_align % 16 == 0
                and (not on or keep_bits_cm_fit(dense, keep_bits, n_cols))):
            return "bwd_bf16x3<bits>" if on else "bwd_bf16x3"
        vx, ldx = _x_operand(dense, n_cols, own_vals, vals_align)
        fast = vx == 4 and ldx % 4 == 0 and kt * 128 <= ldx and ld_in % 4 == 0 and p % 128 == 0 and in_align % 16 == 0
        return "bwd_t128<4,fast>" if fast else f"bwd_t128<{vx}>"
    if dense:
        return "refused" if on and not keep_bits else "bwd_atb"
    vec = ld_in % 4 == 0 and in_align % 16 == 0
    units = cdiv(p, 4) if vec else p
    if vec and units <= 16 and own_vals and nnz * 4 < 0x7FFFFFFF and general <= 0 and (nnz >= NARROW_MIN_NNZ or general < 0):
        return f"bwd_csc_q<{lanes(units)},{nw}>"
    return f"bwd_csc<{lanes(units)},{'vec' if vec else 'scalar'},{nw}>"


def every_name():
    """every kernel name gate() can give (refusals aside), written out from the template lists of csrc/spmm.hip"""
    L = (1, 2, 4, 8, 16, 32, 64)
    names = {"fwd_bf16x3", "fwd_bf16x3<bits>", "fwd_bf16x3<z0>", "fwd_persist", "fwd_persist<bits>", "fwd_t128w8",
             "fwd_t128<4>", "fwd_t128<2>", "fwd_t128<1>", "fwd_csr_sliced",
             "bwd_bf16x3", "bwd_bf16x3<bits>", "bwd_t128<4,fast>", "bwd_t128<4>", "bwd_t128<2>", "bwd_t128<1>", "bwd_atb"}
    names |= {f"fwd_dense<{nt},{v}>" for nt in (1, 2, 4) for v in (1, 2, 4)}
    names |= {f"fwd_csr<{l},{v}>" for l in L for v in ("vec", "scalar")} | {f"fwd_csr_q<{l}>" for l in L[:5]}
    names |= {f"bwd_csc<{l},{v},{nw}>" for l in L for v in ("vec", "scalar") for nw in (1, 4, 16)}
    names |= {f"bwd_csc_q<{l},{nw}>" for l in L[:5] for nw in (1, 4, 16)}
    return names


# ----------------------------------------------------------------------------------------------------- the layouts
SPARSE = dict(n=4400, F=90, per_row=8)                    # column 0 in every stored row: 4 350 entries, past every segment length
SPARSE_BIG_F = 16500                                      # F x 64 x 4 bytes > 4 MiB: the sliced forward at p = 64


def sparse_layout(n=SPARSE["n"], F=SPARSE["F"], per_row=SPARSE["per_row"], seed=11):
    """-> (fp, fi): rows of per_row sorted columns that all hold column 0; every 97th row is empty, the last three columns are"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        if i % 97 == 5:
            rows.append(np.zeros(0, np.int64))
            continue
        rows.append(np.concatenate([[0], np.sort(1 + rng.choice(F - 4, per_row - 1, replace=False))]))
    fp = np.zeros(n + 1, np.int64)
    fp[1:] = np.cumsum([r.size for r in rows])
    return fp.astype(np.int32), np.concatenate(rows).astype(np.int32)


def dense_layout(n, F):
    return (np.arange(n + 1, dtype=np.int64) * F).astype(np.int32), None


# ------------------------------------------------------------------------------------------------------- the table
# id -> dict(op, layout "dense" | "sparse" | "sparse_big", N, F, p, ld (w / dout), ldo (out / dw), ext (external vals), shift
# {operand: floats}, opts {context option: value}, corun, nw, drop (a DROPS key), fused p2, name = what gate() must answer)
def _row(op, layout, N, F, p, name, ld=None, ldo=None, ext=False, shift=None, opts=None, corun=0, nw=0, drop="none", fused=None):
    return dict(op=op, layout=layout, N=N, F=F, p=p, ld=ld or p, ldo=ldo or ld or p, ext=ext, shift=shift or {}, opts=opts or {}, corun=corun,
                nw=nw, drop=drop, fused=fused, name=name)


def _k_name(K, fused=False):
    if fused:
        return "fwd_bf16x3<z0>" if K <= K_FUSED else "NOT_AVAILABLE"
    return "fwd_bf16x3" if K <= K_BF16X3 else "fwd_persist" if K <= K_PERSIST else "fwd_t128w8"


def _paths():
    P = {}
    D, S = "dense", "sparse"
    n0 = 289                                               # nine 32-row blocks and one row
    # dense, p > 64: one row per kernel
    P["fwd-bf16x3"] = _row("fwd", D, n0, 96, 128, "fwd_bf16x3")
    P["fwd-bf16x3-bits"] = _row("fwd", D, n0, 96, 128, "fwd_bf16x3<bits>", drop="philox.3@77")
    P["fused-z0"] = _row("fwd", D, n0, 96, 128, "fwd_bf16x3<z0>", fused=41)
    for p2 in (1, 33, 64):
        P[f"fused-z0-p2-{p2}"] = _row("fwd", D, n0, 96, 128, "fwd_bf16x3<z0>", fused=p2)
    P["fused-refused-p2-65"] = _row("fwd", D, n0, 96, 128, "NOT_AVAILABLE", fused=65)
    P["fwd-persist"] = _row("fwd", D, n0, 96, 128, "fwd_persist", opts=dict(gemm_bf16x3=0))
    P["fwd-persist-bits"] = _row("fwd", D, n0, 96, 128, "fwd_persist<bits>", opts=dict(gemm_bf16x3=0), drop="philox.5@640")
    P["fwd-persist-flat-bits"] = _row("fwd", D, n0, 96, 128, "fwd_persist<bits>", opts=dict(gemm_bf16x3=0), drop="philox.3@77")
    P["fwd-t128w8"] = _row("fwd", D, n0, 96, 128, "fwd_t128w8", opts=dict(gemm_bf16x3=0), corun=1)
    for F, v in ((33, 1), (34, 2), (40, 4)):               # small F: no padded copy, rows of X not 16-byte aligned
        P[f"fwd-t128-F{F}"] = _row("fwd", D, n0, F, 128, f"fwd_t128<{v}>")
        P[f"bwd-atb-F{F}"] = _row("bwd", D, n0, F, 128, "bwd_atb")
        P[f"fwd-dense-F{F}"] = _row("fwd", D, n0, F, 16, f"fwd_dense<1,{v}>")
        P[f"bwd-atb-F{F}-p16"] = _row("bwd", D, n0, F, 16, "bwd_atb")
        for p, ld, nt in ((29, 32, 2), (41, 44, 4)):
            P[f"fwd-dense-F{F}-p{p}"] = _row("fwd", D, n0, F, p, f"fwd_dense<{nt},{v}>", ld=ld)
    P["fused-refused-p16"] = _row("fwd", D, n0, 40, 16, "NOT_AVAILABLE", fused=7)
    P["fused-refused-p256"] = _row("fwd", D, n0, 96, 256, "NOT_AVAILABLE", fused=7)
    P["fused-refused-sparse"] = _row("fwd", S, 0, 0, 128, "NOT_AVAILABLE", fused=7)
    # dense, p = 128: K around the W ring (BX_PD = 6 ahead, BX_NB = 10 deep) and at the three byte limits
    for K in (64, 65, 96, 97, 128, 130, 160, 161, 320, 321, K_FUSED, K_FUSED + 1, K_BF16X3, K_BF16X3 + 1, K_PERSIST, K_PERSIST + 1):
        big = K > 321
        P[f"k{K}-fwd"] = _row("fwd", D, n0, K, 128, _k_name(K))
        P[f"k{K}-fused"] = _row("fwd", D, n0, K, 128, _k_name(K, True), fused=41)
        P[f"k{K}-bwd"] = _row("bwd", D, n0, K, 128, "bwd_bf16x3" if K % 128 else "bwd_t128<4,fast>")
        if big:                                            # ... and what takes over when bf16x3 is switched off
            P[f"k{K}-fwd-f32"] = _row("fwd", D, n0, K, 128, "fwd_persist" if K <= K_PERSIST else "fwd_t128w8", opts=dict(gemm_bf16x3=0))
    P["rows-16401"] = _row("fwd", D, 2 * 8192 + 17, 64, 128, "fwd_bf16x3")       # workgroups own several row blocks
    P["rows-16401-bwd"] = _row("bwd", D, 2 * 8192 + 17, 64, 128, "bwd_bf16x3")
    for n in (1, 31, 32, 33, 255, 256, 257):
        P[f"rows-{n}"] = _row("fwd", D, n, 96, 128, "fwd_bf16x3")
        P[f"rows-{n}-f32"] = _row("fwd", D, n, 96, 128, "fwd_persist", opts=dict(gemm_bf16x3=0))
        P[f"rows-{n}-bwd"] = _row("bwd", D, n, 96, 128, "bwd_bf16x3")
    # dense, external vals: the call after gcnhip_dropout_fwd has no padded copy
    for F, v in ((65, 1), (70, 2), (72, 4)):
        P[f"ext-F{F}-fwd"] = _row("fwd", D, n0, F, 128, f"fwd_t128<{v}>", ext=True)
        P[f"ext-F{F}-bwd"] = _row("bwd", D, n0, F, 128, f"bwd_t128<{v}>", ext=True)
    P["ext-F96-fwd"] = _row("fwd", D, n0, 96, 128, "fwd_bf16x3", ext=True)        # `fast` on an unpadded X
    P["ext-F96-fwd-f32"] = _row("fwd", D, n0, 96, 128, "fwd_persist", ext=True, opts=dict(gemm_bf16x3=0))
    P["ext-F96-bwd"] = _row("bwd", D, n0, 96, 128, "bwd_t128<4>", ext=True)       # not padded: no bf16x3, and 128 columns past its stride
    P["ext-F128-bwd"] = _row("bwd", D, n0, 128, 128, "bwd_t128<4,fast>", ext=True)
    # dense, other p > 64: guarded tiles, two column tiles, pt = 2 in the split-K plan, launch_atb below 64 columns of X
    for p in (65, 100, 130, 256):
        P[f"p{p}-F96-fwd"] = _row("fwd", D, n0, 96, p, "fwd_t128w8" if p == 256 else "fwd_t128<4>", ld=cdiv(p, 4) * 4)
        P[f"p{p}-F96-bwd"] = _row("bwd", D, n0, 96, p, "bwd_t128<4,fast>" if p == 256 else "bwd_t128<4>", ld=cdiv(p, 4) * 4)
        P[f"p{p}-F40-fwd"] = _row("fwd", D, n0, 40, p, "fwd_t128<4>")
        P[f"p{p}-F40-bwd"] = _row("bwd", D, n0, 40, p, "bwd_atb")
    # strides (p, ld) on dense X
    for p, ld in ((7, 8), (41, 44), (41, 41), (128, 132), (100, 100), (3, 4), (29, 32)):
        nt = cdiv(p, 16)
        fn = "fwd_bf16x3" if p == 128 else "fwd_t128<4>" if p > 64 else f"fwd_dense<{4 if nt > 2 else nt},4>"
        bn = "bwd_bf16x3" if p == 128 else "bwd_t128<4>" if p > 64 else "bwd_atb"
        P[f"ld-{p}-{ld}-dense-fwd"] = _row("fwd", D, n0, 96, p, fn, ld=ld, ldo=ld + 5)
        P[f"ld-{p}-{ld}-dense-bwd"] = _row("bwd", D, n0, 96, p, bn, ld=ld, ldo=ld + 5)
    # operands that start one or two floats into their allocation
    for s in (1, 2):
        v = {1: 1, 2: 2}[s]
        P[f"shift{s}-w-dense"] = _row("fwd", D, n0, 96, 128, "fwd_t128<4>", shift=dict(w=s))
        P[f"shift{s}-out-dense"] = _row("fwd", D, n0, 96, 128, "fwd_t128w8", shift=dict(out=s))
        P[f"shift{s}-vals-dense"] = _row("fwd", D, n0, 96, 128, f"fwd_t128<{v}>", ext=True, shift=dict(vals=s))
        P[f"shift{s}-vals-dense-p16"] = _row("fwd", D, n0, 96, 16, f"fwd_dense<1,{v}>", ext=True, shift=dict(vals=s))
        P[f"shift{s}-vals-dense-p29"] = _row("fwd", D, n0, 96, 29, f"fwd_dense<2,{v}>", ld=32, ext=True, shift=dict(vals=s))
        P[f"shift{s}-vals-dense-p41"] = _row("fwd", D, n0, 96, 41, f"fwd_dense<4,{v}>", ld=44, ext=True, shift=dict(vals=s))
        P[f"shift{s}-dout-dense"] = _row("bwd", D, n0, 96, 128, "bwd_t128<4>", shift=dict(dout=s))
        P[f"shift{s}-dw-dense"] = _row("bwd", D, n0, 96, 128, "bwd_bf16x3", shift=dict(out=s))
        P[f"shift{s}-vals-dense-bwd"] = _row("bwd", D, n0, 96, 128, f"bwd_t128<{v}>", ext=True, shift=dict(vals=s))
        P[f"shift{s}-vals-atb"] = _row("bwd", D, n0, 40, 16, "bwd_atb", ext=True, shift=dict(vals=s))
        P[f"shift{s}-dout-atb"] = _row("bwd", D, n0, 40, 16, "bwd_atb", shift=dict(dout=s))
        P[f"shift{s}-dw-atb"] = _row("bwd", D, n0, 40, 16, "bwd_atb", shift=dict(out=s))
        P[f"shift{s}-w-dense-p16"] = _row("fwd", D, n0, 96, 16, "fwd_dense<1,4>", shift=dict(w=s))
        P[f"shift{s}-out-dense-p16"] = _row("fwd", D, n0, 96, 16, "fwd_dense<1,4>", shift=dict(out=s))
        P[f"shift{s}-z-fused"] = _row("fwd", D, n0, 96, 128, "NOT_AVAILABLE", shift=dict(out=s), fused=7)
        P[f"shift{s}-w-sparse"] = _row("fwd", S, 0, 0, 16, "fwd_csr<16,scalar>", shift=dict(w=s))
        P[f"shift{s}-out-sparse"] = _row("fwd", S, 0, 0, 16, "fwd_csr<4,vec>", shift=dict(out=s))
        P[f"shift{s}-vals-sparse"] = _row("fwd", S, 0, 0, 16, "fwd_csr_q<4>", ext=True, shift=dict(vals=s), opts=dict(spmm_general=-1))
        P[f"shift{s}-dout-sparse"] = _row("bwd", S, 0, 0, 16, "bwd_csc<16,scalar,1>", shift=dict(dout=s), nw=1)
        P[f"shift{s}-dw-sparse"] = _row("bwd", S, 0, 0, 16, "bwd_csc_q<4,1>", shift=dict(out=s), nw=1, opts=dict(spmm_general=-1))
        P[f"shift{s}-vals-sparse-bwd"] = _row("bwd", S, 0, 0, 16, "bwd_csc<4,vec,1>", ext=True, shift=dict(vals=s), nw=1)
    # gemm_bf16x3 x the co-run mark, wherever a predicate reads them
    for bx, co in itertools.product((0, 1, 2), (0, 1)):
        lane = bx == 2 or (bx == 1 and not co)
        o = dict(gemm_bf16x3=bx)
        P[f"bx{bx}-corun{co}-fwd"] = _row("fwd", D, n0, 96, 128, "fwd_bf16x3" if lane else "fwd_t128w8" if co else "fwd_persist", opts=o, corun=co)
        P[f"bx{bx}-corun{co}-bwd"] = _row("bwd", D, n0, 96, 128, "bwd_bf16x3" if lane else "bwd_t128<4,fast>", opts=o, corun=co)
        P[f"bx{bx}-corun{co}-fused"] = _row("fwd", D, n0, 96, 128, "fwd_bf16x3<z0>" if bx else "NOT_AVAILABLE", opts=o, corun=co, fused=7)
    P["bwd-bf16x3-bits"] = _row("bwd", D, n0, 96, 128, "bwd_bf16x3<bits>", drop="philox.3@77")
    # sparse X: lanes per row by (p, ld), vector and scalar; the narrow kernels under spmm_general = -1; the sliced form
    vec = ((3, 4, 1), (7, 8, 2), (16, 16, 4), (29, 32, 8), (41, 44, 16), (64, 64, 16), (100, 100, 32), (128, 132, 32), (130, 132, 64), (256, 256, 64),
           (260, 260, 64))                                 # p > 256: a second column pass
    scalar = ((1, 1, 1), (2, 2, 2), (3, 3, 4), (7, 7, 8), (13, 13, 16), (29, 29, 32), (41, 41, 64), (70, 70, 64))
    for p, ld, l in vec:
        P[f"sparse-fwd-vec-{p}-{ld}"] = _row("fwd", S, 0, 0, p, f"fwd_csr<{l},vec>", ld=ld, ldo=ld + 1)
        if l <= 16:
            P[f"sparse-fwd-q-{p}-{ld}"] = _row("fwd", S, 0, 0, p, f"fwd_csr_q<{l}>", ld=ld, ldo=ld + 1, opts=dict(spmm_general=-1))
    for p, ld, l in scalar:
        P[f"sparse-fwd-scalar-{p}-{ld}"] = _row("fwd", S, 0, 0, p, f"fwd_csr<{l},scalar>", ld=ld, ldo=ld + 3)
    P["sparse-fwd-sliced"] = _row("fwd", "sparse_big", 0, 0, 64, "fwd_csr_sliced")
    P["sparse-fwd-unsliced"] = _row("fwd", "sparse_big", 0, 0, 64, "fwd_csr<16,vec>", opts=dict(spmm_slices=0))
    for nw in (1, 4, 16):
        for p, ld, l in vec:
            P[f"sparse-bwd-vec-{p}-{ld}-nw{nw}"] = _row("bwd", S, 0, 0, p, f"bwd_csc<{l},vec,{nw}>", ld=ld, ldo=ld + 1, nw=nw)
            if l <= 16:
                P[f"sparse-bwd-q-{p}-{ld}-nw{nw}"] = _row("bwd", S, 0, 0, p, f"bwd_csc_q<{l},{nw}>", ld=ld, ldo=ld + 1, nw=nw, opts=dict(spmm_general=-1))
                # the same call with a value array of the caller's: no CSC copy of it, the general kernel gathers through csc_pos
                P[f"sparse-bwd-pos-{p}-{ld}-nw{nw}"] = _row("bwd", S, 0, 0, p, f"bwd_csc<{l},vec,{nw}>", ld=ld, ldo=ld + 1, nw=nw, ext=True,
                                                            opts=dict(spmm_general=-1))
        for p, ld, l in scalar:
            P[f"sparse-bwd-scalar-{p}-{ld}-nw{nw}"] = _row("bwd", S, 0, 0, p, f"bwd_csc<{l},scalar,{nw}>", ld=ld, ldo=ld + 3, nw=nw)
    return P


PATHS = _paths()


def shape_of(row):
    """(dense, n_rows, n_cols, nnz) of a table row"""
    if row["layout"] == "dense":
        return True, row["N"], row["F"], row["N"] * row["F"]
    F = SPARSE_BIG_F if row["layout"] == "sparse_big" else SPARSE["F"]
    n = SPARSE["n"]
    return False, n, F, (n - cdiv(n - 5, 97)) * SPARSE["per_row"]


def gate_of(row, drop="row", n_cu=N_CU, **over):
    """gate() on a table row; drop: a DROPS key ("row": the row's own)"""
    dense, n, F, nnz = shape_of(row)
    sh = row["shift"]
    in_key = "w" if row["op"] == "fwd" else "dout"
    al = lambda s: 16 if s % 4 == 0 else 8 if s % 2 == 0 else 4
    fused = None
    if row["fused"]:
        ldz = cdiv(row["fused"], 4) * 4
        fused = dict(p2=row["fused"], ld_z0=ldz, ld_w2=ldz, z_align=al(sh.get("out", 0)))
    kw = dict(op=row["op"], dense=dense, n_rows=n, n_cols=F, nnz=nnz, p=row["p"], ld_in=row["ld"], own_vals=not row["ext"],
              vals_align=al(sh.get("vals", 0)), in_align=al(sh.get(in_key, 0)), out_align=al(sh.get("out", 0)),
              drop=DROPS[row["drop"] if drop == "row" else drop], bx=row["opts"].get("gemm_bf16x3", 2), corun=row["corun"],
              general=row["opts"].get("spmm_general", 0), slices=row["opts"].get("spmm_slices", 1), nw=row["nw"] or 1, fused=fused, n_cu=n_cu)
    kw.update(over)
    return gate(**kw)
