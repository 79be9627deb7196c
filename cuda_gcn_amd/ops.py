"""numpy front end of the op-level C-ABI (include/gcnhip.h).

Each function mirrors one module of the reference (Matmul, SparseMatmul,
GraphSum, CrossEntropyLoss, ReLU, Dropout, Adam): same operand meaning, numpy
arrays in and out.  Arrays are staged through device buffers owned by a
``Device`` (gcnhip_malloc / h2d / d2h); all compute happens in the HIP kernels.
There is no CPU path here: without libgcnhip.so and a GPU these calls raise.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


class GsOpts(C.Structure):
    """gcnhip_gs_opts (include/gcnhip.h)"""
    _fields_ = [("rows", C.c_void_p), ("in_row_bits", C.c_void_p), ("accumulate", C.c_int), ("relu_dropout", C.c_int), ("training", C.c_int),
                ("p", C.c_float), ("seed", C.c_uint64), ("d_epoch", C.c_void_p), ("elem_offset", C.c_uint64), ("keep_mask", C.c_void_p),
                ("pos_bits", C.c_void_p), ("words_per_row", C.c_int), ("scaling", C.c_int), ("loss", C.c_void_p)]


class GsLoss(C.Structure):
    """gcnhip_gs_loss (include/gcnhip.h)"""
    _fields_ = [("truth", C.c_void_p), ("grad", C.c_void_p), ("ld_grad", C.c_int), ("training", C.c_int), ("count", C.c_int),
                ("grad_row_scale", C.c_void_p), ("row_terms", C.c_void_p)]


class GcnHipError(RuntimeError):
    pass


def _ck(lib, code, what):
    if code != 0:
        msg = lib.gcnhip_error_string(code)
        raise GcnHipError(f"{what}: error {code} ({msg.decode() if msg else '?'})")


class Buf:
    """a device allocation with a numpy-ish shape/dtype"""

    def __init__(self, dev: "Device", shape, dtype):
        self.dev = dev
        self.shape = tuple(int(s) for s in np.atleast_1d(shape))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        _ck(dev.lib, dev.lib.gcnhip_malloc(dev.ctx, C.byref(p), max(self.nbytes, 16)), "gcnhip_malloc")
        self.ptr = p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, self.dtype)
        assert arr.nbytes == self.nbytes, (arr.shape, self.shape)
        _ck(self.dev.lib, self.dev.lib.gcnhip_h2d(self.dev.ctx, self.ptr, arr.ctypes.data, self.nbytes), "gcnhip_h2d")
        return self

    def download(self):
        out = np.empty(self.shape, self.dtype)
        _ck(self.dev.lib, self.dev.lib.gcnhip_d2h(self.dev.ctx, out.ctypes.data, self.ptr, self.nbytes), "gcnhip_d2h")
        return out

    def fill_bytes(self, byte=0):
        _ck(self.dev.lib, self.dev.lib.gcnhip_memset_async(self.dev.ctx, self.ptr, byte, self.nbytes), "memset")
        return self

    def free(self):
        if self.ptr and self.dev.ctx:            # a closed Device has already released the GPU
            self.dev.lib.gcnhip_free(self.dev.ctx, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Device:
    """one GPU context (device + stream + scratch)"""

    def __init__(self, device: int = 0, stream=None):
        self.lib = _lib.gcnhip()
        n = C.c_int()
        _ck(self.lib, self.lib.gcnhip_device_count(C.byref(n)), "gcnhip_device_count")
        if n.value <= device:
            raise GcnHipError(f"no GPU {device} (device count {n.value}); this package has no CPU path")
        ctx = C.c_void_p()
        _ck(self.lib, self.lib.gcnhip_ctx_create(C.byref(ctx), device, stream), "gcnhip_ctx_create")
        self.ctx = ctx

    def close(self):
        if self.ctx:
            self.lib.gcnhip_ctx_destroy(self.ctx)
            self.ctx = None

    def sync(self):
        _ck(self.lib, self.lib.gcnhip_ctx_sync(self.ctx), "sync")

    def set_option(self, name: str, value: int):
        """gcnhip_ctx_set_option: a named option of this context (read by the ops at call time from the context, never from the environment)"""
        _ck(self.lib, self.lib.gcnhip_ctx_set_option(self.ctx, name.encode(), int(value)), f"gcnhip_ctx_set_option({name})")

    def get_option(self, name: str) -> int:
        v = C.c_int()
        _ck(self.lib, self.lib.gcnhip_ctx_get_option(self.ctx, name.encode(), C.byref(v)), f"gcnhip_ctx_get_option({name})")
        return v.value

    def buf(self, arr_or_shape, dtype=np.float32):
        if isinstance(arr_or_shape, np.ndarray):
            return Buf(self, arr_or_shape.shape, arr_or_shape.dtype).upload(arr_or_shape)
        return Buf(self, arr_or_shape, dtype)

    def padded(self, arr, ld):
        """upload a 2-D float array into a buffer with leading dimension ld (pad = NaN to catch misuse)"""
        arr = np.asarray(arr, np.float32)
        out = np.full((arr.shape[0], ld), np.nan, np.float32)
        out[:, :arr.shape[1]] = arr
        return self.buf(out)

    # ---- prepared objects
    def graph(self, indptr, indices, n_cols=None, col_deg=None, row_group=None):
        return Graph(self, indptr, indices, n_cols, col_deg, row_group)

    def feat(self, indptr, indices, values, n_cols):
        return Feat(self, indptr, indices, values, n_cols)

    # ---- ops (numpy in, numpy out)
    def _bits(self, flags):
        bits = np.packbits(np.asarray(flags, bool), bitorder="little")
        return self.buf(np.concatenate([bits, np.zeros((-bits.size) % 4 + 4, np.uint8)]).view(np.uint32))

    def graphsum_masked(self, g: "Graph", x, ld_in=None, ld_out=None, row_nonzero=None, out_rows=None, fill=np.nan):
        """gcnhip_graphsum_masked: rows of x flagged zero are not read, rows of the result not in out_rows are
        not computed (they keep `fill`)"""
        x = np.asarray(x, np.float32)
        dim = x.shape[1]
        ld_in, ld_out = ld_in or dim, ld_out or dim
        xin = self.padded(x, ld_in)
        out = self.buf(np.full((g.n_rows, ld_out), fill, np.float32))
        g.reserve(dim)
        ib = self._bits(row_nonzero) if row_nonzero is not None else None
        ob = self._bits(out_rows) if out_rows is not None else None
        _ck(self.lib, self.lib.gcnhip_graphsum_masked(self.ctx, g.h, xin.ptr, ld_in, out.ptr, ld_out, dim,
                                                       ib.ptr if ib else None, ob.ptr if ob else None), "gcnhip_graphsum_masked")
        return out.download()[:, :dim]

    def graphsum_rowset(self, g: "Graph", rows_handle, x, ld_in=None, ld_out=None, row_nonzero=None, fill=np.nan):
        """gcnhip_graphsum_rowset: only the rows of a subset registered with Graph.add_rowset are computed"""
        x = np.asarray(x, np.float32)
        dim = x.shape[1]
        ld_in, ld_out = ld_in or dim, ld_out or dim
        xin = self.padded(x, ld_in)
        out = self.buf(np.full((g.n_rows, ld_out), fill, np.float32))
        g.reserve(dim)
        ib = self._bits(row_nonzero) if row_nonzero is not None else None
        _ck(self.lib, self.lib.gcnhip_graphsum_rowset(self.ctx, g.h, rows_handle, xin.ptr, ld_in, out.ptr, ld_out, dim,
                                                       ib.ptr if ib else None), "gcnhip_graphsum_rowset")
        return out.download()[:, :dim]

    def _gs_operands(self, g, x, dim, ld, ld_in, ld_out, prev, fill, out, row_nonzero, keep_mask, epoch, want_bits, bits):
        """the device operands of one aggregation call.  x, row_nonzero (packed bits), keep_mask, out and bits may be Bufs that
        already sit on the device (a table of cases keeps them there between calls); arrays are uploaded.  `out` given as a
        Buf is used as the caller left it."""
        if isinstance(x, Buf):
            xin, ld_in = x, x.shape[1]
            dim = dim or ld_in
        else:
            x = np.asarray(x, np.float32)
            dim = x.shape[1]
            ld_in = ld_in or ld or (dim + 3) // 4 * 4
            xin = self.padded(x, ld_in)
        ld_out = out.shape[1] if out is not None else (ld_out or ld or (dim + 3) // 4 * 4)
        if out is None:
            out = self.padded(prev, ld_out) if prev is not None else self.buf(np.full((g.n_rows, ld_out), fill, np.float32))
        g.reserve(dim)
        ib = row_nonzero if isinstance(row_nonzero, Buf) or row_nonzero is None else self._bits(row_nonzero)
        km = keep_mask if isinstance(keep_mask, Buf) or keep_mask is None else self.buf(np.ascontiguousarray(keep_mask, np.uint8))
        ep = self.buf(np.array([epoch], np.uint32))
        wpr = (dim + 31) // 32
        if want_bits and bits is None:
            bits = self.buf(np.full((g.n_rows, wpr), 0xDEADBEEF, np.uint32))
        return xin, ld_in, out, ld_out, dim, ib, km, ep, bits, wpr

    def graphsum_ex(self, g: "Graph", x, scaling=0, ld=None, rows=None, row_nonzero=None, prev=None, fill=np.nan, ld_in=None, ld_out=None,
                    out_rows=None, relu_dropout=False, training=False, p=0.0, seed=0, epoch=0, elem_offset=0, keep_mask=None,
                    want_bits=False, dim=None, out=None, bits=None, accumulate=None):
        """gcnhip_graphsum_ex: one aggregation with every option of the launch record.  scaling != 0 is the factored operator:
        `x` must already hold dinv[col] * (the reference's input).  prev: the rows of `out` before the call (accumulate = 1).
        ld_in / ld_out: any value >= dim (ld: both); rows: a handle from Graph.add_rowset.  relu_dropout, training, p, seed,
        epoch, elem_offset, keep_mask: the store epilogue; want_bits: also return the (out > 0) words, uint32 [n_rows, dim / 32].
        out_rows (bool per row, or a Buf of packed bits): output-row bits.  The entry point that carries them is
        gcnhip_graphsum_masked, which takes input-row bits beside them and nothing else, so the call goes there.
        x, row_nonzero, keep_mask, out and bits may be device Bufs (see _gs_operands); `accumulate` then says what prev would."""
        xin, ld_in, out, ld_out, dim, ib, km, ep, bits, wpr = self._gs_operands(g, x, dim, ld, ld_in, ld_out, prev, fill, out, row_nonzero,
                                                                                 keep_mask, epoch, want_bits, bits)
        acc = int(accumulate if accumulate is not None else prev is not None)
        if out_rows is not None:
            if rows is not None or acc or scaling or relu_dropout or bits is not None:
                raise ValueError("graphsum_ex: output-row bits travel through gcnhip_graphsum_masked, which takes only input-row bits beside them")
            ob = out_rows if isinstance(out_rows, Buf) else self._bits(out_rows)
            _ck(self.lib, self.lib.gcnhip_graphsum_masked(self.ctx, g.h, xin.ptr, ld_in, out.ptr, ld_out, dim, ib.ptr if ib else None, ob.ptr),
                "gcnhip_graphsum_masked")
            return out.download()[:, :dim]
        o = GsOpts()
        o.rows = rows
        o.in_row_bits = ib.ptr if ib else None
        o.accumulate = acc
        o.relu_dropout, o.training, o.p = int(bool(relu_dropout)), int(bool(training)), float(p)
        o.seed, o.d_epoch, o.elem_offset = int(seed), ep.ptr, int(elem_offset)
        o.keep_mask = km.ptr if km else None
        o.pos_bits, o.words_per_row = (bits.ptr, wpr) if bits is not None else (None, 0)
        o.scaling = int(scaling)
        rc = self.lib.gcnhip_graphsum_ex(self.ctx, g.h, C.byref(o), xin.ptr, ld_in, out.ptr, ld_out, dim)
        if rc != 0:
            raise GcnHipError(f"gcnhip_graphsum_ex: error {rc} ({self.lib.gcnhip_error_string(rc).decode()}): {self.lib.gcnhip_last_error().decode()}")
        res = out.download()[:, :dim]
        return (res, bits.download()) if bits is not None else res

    def graphsum_part(self, g: "Graph", x, rows=None, row_nonzero=None, prev=None, fill=np.nan, ld=None, ld_in=None, ld_out=None,
                      relu_dropout=False, training=False, p=0.0, seed=0, epoch=0, elem_offset=0, keep_mask=None, dim=None, out=None,
                      accumulate=None):
        """gcnhip_graphsum_part: one operator's share of a row-partitioned aggregation (arguments as graphsum_ex)"""
        xin, ld_in, out, ld_out, dim, ib, km, ep, _, _ = self._gs_operands(g, x, dim, ld, ld_in, ld_out, prev, fill, out, row_nonzero,
                                                                            keep_mask, epoch, False, None)
        acc = int(accumulate if accumulate is not None else prev is not None)
        rc = self.lib.gcnhip_graphsum_part(self.ctx, g.h, rows, xin.ptr, ld_in, out.ptr, ld_out, dim, ib.ptr if ib else None, acc,
                                           int(bool(relu_dropout)), int(bool(training)), float(p), int(seed), ep.ptr, int(elem_offset),
                                           km.ptr if km else None)
        if rc != 0:
            raise GcnHipError(f"gcnhip_graphsum_part: error {rc} ({self.lib.gcnhip_error_string(rc).decode()}): {self.lib.gcnhip_last_error().decode()}")
        return out.download()[:, :dim]

    def graphsum_loss(self, g: "Graph", x, scaling, truth, rows=None, training=True, grad_row_scale=None, ld=None, epilogue=True, grad_fill=0.0):
        """the logits' aggregation followed by the loss over the labelled rows (truth >= 0), two ways:
        epilogue=True : gcnhip_graphsum_ex with a gcnhip_gs_loss + gcnhip_xent_from_row_terms;
        epilogue=False: gcnhip_graphsum_ex, then gcnhip_xent_fwd_rows_scaled on the stored logits.
        returns dict(logits, grad, loss_sum, count, correct, total)"""
        x = np.asarray(x, np.float32)
        truth = np.ascontiguousarray(truth, np.int32)
        dim = x.shape[1]
        ld = ld or (dim + 3) // 4 * 4
        xin = self.padded(x, ld)
        out = self.buf(np.full((g.n_rows, ld), np.nan, np.float32))
        gb = self.buf(np.full((g.n_rows, ld), grad_fill, np.float32))
        listed = np.flatnonzero(truth >= 0).astype(np.int32)
        tb, rb = self.buf(truth), self.buf(listed if listed.size else np.zeros(1, np.int32))
        sb = self.buf(np.ascontiguousarray(grad_row_scale, np.float32)) if grad_row_scale is not None else None
        res, resi = self.buf(np.zeros(4, np.float32)), self.buf(np.zeros(2, np.int32))
        terms = self.buf(np.full((g.n_rows, 2), np.nan, np.float32))
        count = max(int(listed.size), 1)
        o = GsOpts()
        o.rows = rows
        o.scaling = int(scaling)
        lo = GsLoss()
        if epilogue:
            lo.truth = tb.ptr; lo.grad = gb.ptr; lo.ld_grad = ld; lo.training = int(training); lo.count = count
            lo.grad_row_scale = sb.ptr if sb else None
            lo.row_terms = terms.ptr
            o.loss = C.addressof(lo)
        _ck(self.lib, self.lib.gcnhip_graphsum_ex(self.ctx, g.h, C.byref(o), xin.ptr, ld, out.ptr, ld, dim), "gcnhip_graphsum_ex")
        if epilogue:
            _ck(self.lib, self.lib.gcnhip_xent_from_row_terms(self.ctx, terms.ptr, tb.ptr, rb.ptr, int(listed.size), res.ptr, resi.ptr), "gcnhip_xent_from_row_terms")
        else:
            _ck(self.lib, self.lib.gcnhip_xent_fwd_rows_scaled(self.ctx, out.ptr, ld, gb.ptr, ld, tb.ptr, rb.ptr, int(listed.size), dim, int(training), count, 0,
                                                               res.ptr, resi.ptr, sb.ptr if sb else None), "gcnhip_xent_fwd_rows_scaled")
        r, ri = res.download(), resi.download()
        return dict(logits=out.download()[:, :dim], grad=gb.download(), loss_sum=float(r[0]), count=float(r[1]), correct=int(ri[0]), total=int(ri[1]),
                    res=r, terms=terms.download() if epilogue else None)

    def graphsum_predict(self, g: "Graph", x=None, scaling=0, rows=None, table_bf16=None, dim=None, ld=None, logp=True, store_logits=True):
        """gcnhip_graphsum_predict: the logits' aggregation with the prediction epilogue.  Either f32 rows `x` (scaling as in
        graphsum_ex) or a bf16 table `table_bf16` (uint16 [n_cols, ld], with `dim` columns).  rows: a handle from Graph.add_rowset
        (None: every row).  Returns dict(pred int32 [n_rows], prob, logp [n_rows, dim] or None, logits or None); rows not
        computed hold pred = -1 and NaN."""
        if (x is None) == (table_bf16 is None):
            raise ValueError("graphsum_predict: pass exactly one of x and table_bf16")
        if x is not None:
            x = np.asarray(x, np.float32)
            dim = x.shape[1]
            ld = ld or (dim + 3) // 4 * 4
            xin, tin, ld_in = self.padded(x, ld), None, ld
        else:
            t = np.ascontiguousarray(table_bf16, np.uint16)
            xin, tin, ld_in = None, self.buf(t), t.shape[1]
        ld_out = (dim + 3) // 4 * 4
        out = self.buf(np.full((g.n_rows, ld_out), np.nan, np.float32)) if store_logits else None
        pb = self.buf(np.full(max(g.n_rows, 1), -1, np.int32))
        qb = self.buf(np.full(max(g.n_rows, 1), np.nan, np.float32))
        lb = self.buf(np.full((max(g.n_rows, 1), dim), np.nan, np.float32)) if logp else None
        g.reserve(dim)
        _ck(self.lib, self.lib.gcnhip_graphsum_predict(self.ctx, g.h, rows, xin.ptr if xin else None, tin.ptr if tin else None, ld_in,
                                                        out.ptr if out else None, ld_out, dim, int(scaling), pb.ptr, qb.ptr,
                                                        lb.ptr if lb else None, dim), "gcnhip_graphsum_predict")
        n = g.n_rows
        return dict(pred=pb.download()[:n], prob=qb.download()[:n], logp=lb.download()[:n] if lb else None,
                    logits=out.download()[:, :dim] if out else None)

    def graphsum_blend(self, g: "Graph", x, base=None, alpha=1.0, beta=0.0, lo=-np.inf, hi=np.inf, ld=None, argmax=False, fill=np.nan,
                       alias_out=False):
        """gcnhip_graphsum_blend: clip(alpha . (A^ . x) + beta . base, lo, hi) with the object's per-edge coefficients.  base=None:
        the gathered table itself is the base (the same device buffer); alias_out=True passes out = in (refused).  Returns the
        WHOLE out table [n_rows, ld] (its padding columns keep `fill`), and with argmax=True also pred int32 [n_rows]."""
        x = np.asarray(x, np.float32)
        dim = x.shape[1]
        ld = ld or (dim + 3) // 4 * 4
        xin = self.padded(x, ld)
        bb = xin if base is None else self.padded(np.asarray(base, np.float32), ld)
        out = xin if alias_out else self.buf(np.full((g.n_rows, ld), fill, np.float32))
        pb = self.buf(np.full(max(g.n_rows, 1), -1, np.int32)) if argmax else None
        g.reserve(dim)
        rc = self.lib.gcnhip_graphsum_blend(self.ctx, g.h, xin.ptr, ld, bb.ptr, ld, out.ptr, ld, dim, float(alpha), float(beta), float(lo),
                                            float(hi), pb.ptr if pb else None)
        if rc != 0:
            raise GcnHipError(f"gcnhip_graphsum_blend: error {rc}: {self.lib.gcnhip_last_error().decode()}")
        o = out.download()
        return (o, pb.download()[:g.n_rows]) if argmax else o

    def cs_error_rows(self, logp, truth, rows=None, ld_e=None, fill=np.nan):
        """gcnhip_cs_error_rows: (E [n, ld_e] — uploaded as `fill`, the launch zeroes it —, sigma f32 [2] = {sum |E|, rows}).  logp
        f32 [n, C] (unpadded rows), truth int32 [n]; rows: the listed rows (None: every row)"""
        logp = np.ascontiguousarray(logp, np.float32)
        truth = np.ascontiguousarray(truth, np.int32)
        n, c = logp.shape
        ld_e = ld_e or (c + 3) // 4 * 4
        rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
        lb, tb = self.buf(logp), self.buf(truth)
        rb = self.buf(rows if rows.size else np.zeros(1, np.int32)) if rows is not None else None
        eb = self.buf(np.full((n, ld_e), fill, np.float32))
        sb = self.buf(np.full(2, np.nan, np.float32))
        rc = self.lib.gcnhip_cs_error_rows(self.ctx, lb.ptr, c, tb.ptr, n, rb.ptr if rb else None, int(n if rows is None else rows.size), c,
                                           eb.ptr, ld_e, sb.ptr)
        if rc != 0:
            raise GcnHipError(f"gcnhip_cs_error_rows: error {rc}: {self.lib.gcnhip_last_error().decode()}")
        return eb.download(), sb.download()

    def cs_correct_rows(self, logp, e_hat, truth, sigma, ld_g=None, fill=np.nan):
        """gcnhip_cs_correct_rows: G0 [n, ld_g] (padding columns keep `fill`).  logp f32 [n, C], e_hat f32 [n, ld_e >= C], truth
        int32 [n], sigma f32 [2] as cs_error_rows leaves it"""
        logp = np.ascontiguousarray(logp, np.float32)
        e_hat = np.ascontiguousarray(e_hat, np.float32)
        n, c = logp.shape
        ld_g = ld_g or (c + 3) // 4 * 4
        lb, eb, tb = self.buf(logp), self.buf(e_hat), self.buf(np.ascontiguousarray(truth, np.int32))
        sb = self.buf(np.ascontiguousarray(sigma, np.float32))
        gb = self.buf(np.full((n, ld_g), fill, np.float32))
        rc = self.lib.gcnhip_cs_correct_rows(self.ctx, lb.ptr, c, eb.ptr, e_hat.shape[1], tb.ptr, n, c, sb.ptr, gb.ptr, ld_g)
        if rc != 0:
            raise GcnHipError(f"gcnhip_cs_correct_rows: error {rc}: {self.lib.gcnhip_last_error().decode()}")
        return gb.download()

    def _calib_inputs(self, logp, ld, truth, rows):
        logp = np.ascontiguousarray(logp, np.float32)
        n_table, c = logp.shape
        lb = self.padded(logp, ld or c)
        tb = self.buf(np.ascontiguousarray(truth, np.int32) if n_table else np.zeros(1, np.int32)) if truth is not None else None
        rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
        rb = self.buf(rows if rows.size else np.zeros(1, np.int32)) if rows is not None else None
        return lb, tb, rb, n_table, c, int(n_table if rows is None else rows.size)

    def calib_nll_rows(self, logp, truth, beta, rows=None, ld=None, n=None):
        """gcnhip_calib_nll_rows: float64 [4] = {sum nll, sum g, sum h, rows counted}.  logp f32 [n_table, C] (uploaded with row
        stride ld, NaN padding), truth int32 [n_table]; rows: the listed rows (None: rows 0 .. n - 1, n = n_table unless given)"""
        lb, tb, rb, n_table, c, listed = self._calib_inputs(logp, ld, truth, rows)
        ob = self.buf(np.full(4, np.nan, np.float64))
        rc = self.lib.gcnhip_calib_nll_rows(self.ctx, lb.ptr, ld or c, tb.ptr, n_table, rb.ptr if rb else None, listed if n is None else int(n), c,
                                            float(beta), ob.ptr)
        if rc != 0:
            raise GcnHipError(f"gcnhip_calib_nll_rows: error {rc}: {self.lib.gcnhip_last_error().decode()}")
        return ob.download()

    def calib_bins_rows(self, logp, truth, beta, bins, rows=None, ld=None):
        """gcnhip_calib_bins_rows: (count int32 [bins], correct int32 [bins], conf_sum float64 [bins]); the outputs are uploaded as
        garbage — the launch zeroes or overwrites them"""
        lb, tb, rb, n_table, c, listed = self._calib_inputs(logp, ld, truth, rows)
        k = max(int(bins), 1)
        cb, kb = self.buf(np.full(k, 12345, np.int32)), self.buf(np.full(k, -777, np.int32))
        sb = self.buf(np.full(k, np.nan, np.float64))
        rc = self.lib.gcnhip_calib_bins_rows(self.ctx, lb.ptr, ld or c, tb.ptr, n_table, rb.ptr if rb else None, listed, c, float(beta), int(bins),
                                             cb.ptr, kb.ptr, sb.ptr)
        if rc != 0:
            raise GcnHipError(f"gcnhip_calib_bins_rows: error {rc}: {self.lib.gcnhip_last_error().decode()}")
        return cb.download(), kb.download(), sb.download()

    def calib_scale_rows(self, logp, beta, rows=None, ld=None, ld_out=None, in_place=False, fill=np.nan):
        """gcnhip_calib_scale_rows: (out [n_table, ld_out] — rows not listed and padding columns keep `fill` —, prob f32 [n_table],
        `fill` where no row was scaled).  in_place=True: out is the uploaded logp table itself (its own stride and contents)"""
        lb, _, rb, n_table, c, listed = self._calib_inputs(logp, ld, None, rows)
        ld_out = (ld or c) if in_place else (ld_out or c)
        ob = lb if in_place else self.buf(np.full((n_table, ld_out), fill, np.float32))
        pb = self.buf(np.full(max(n_table, 1), fill, np.float32))
        rc = self.lib.gcnhip_calib_scale_rows(self.ctx, lb.ptr, ld or c, n_table, rb.ptr if rb else None, listed, c, float(beta), ob.ptr, ld_out, pb.ptr)
        if rc != 0:
            raise GcnHipError(f"gcnhip_calib_scale_rows: error {rc}: {self.lib.gcnhip_last_error().decode()}")
        return ob.download(), pb.download()[:n_table]

    # ---- Monte Carlo dropout (csrc/mcdropout.hip)
    def mc_accumulate_rows(self, samples, rows=None, ld=None, n=None, fill=None):
        """gcnhip_mc_accumulate_rows, one launch per sample in order, the first with first=1: (acc float64 [n, C + 1], votes int32
        [n, C]) by list position.  samples: f32 [S, n_table, C] log-softmax rows (each uploaded with row stride ld, NaN padding);
        rows: the listed rows (None: rows 0 .. n - 1, n = n_table unless given).  fill=(f64, i32): the accumulators start as these
        sentinels (the first launch must store over them); None: NaN / -777"""
        samples = np.ascontiguousarray(samples, np.float32)
        if samples.ndim == 2:
            samples = samples[None]
        s_count, n_table, c = samples.shape
        rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
        rb = self.buf(rows if rows.size else np.zeros(1, np.int32)) if rows is not None else None
        listed = int(n_table if rows is None else rows.size) if n is None else int(n)
        f64, i32 = (np.nan, -777) if fill is None else fill
        ab = self.buf(np.full((max(listed, 1), c + 1), f64, np.float64))
        vb = self.buf(np.full((max(listed, 1), c), i32, np.int32))
        for s in range(s_count):
            lb = self.padded(samples[s], max(ld or c, c)) if n_table else self.buf(np.zeros(1, np.float32))   # (a stride below C is refused)
            rc = self.lib.gcnhip_mc_accumulate_rows(self.ctx, lb.ptr, ld or c, n_table, rb.ptr if rb else None, listed, c, int(s == 0), ab.ptr, vb.ptr)
            if rc != 0:
                raise GcnHipError(f"gcnhip_mc_accumulate_rows: error {rc}: {self.lib.gcnhip_last_error().decode()}")
        return ab.download()[:listed], vb.download()[:listed]

    MC_OUTPUTS = ("mean_prob", "pred", "confidence", "entropy", "expected_entropy", "mutual_information", "variation_ratio")

    def mc_finalize_rows(self, acc, votes, samples, ld_mp=None, outputs=MC_OUTPUTS, fill=np.nan, pred_fill=-777):
        """gcnhip_mc_finalize_rows: a dict of the outputs named in `outputs` (the others are passed as NULL) — mean_prob f32
        [n, ld_mp] whose padding columns keep `fill`, pred int32 [n], the rest f32 [n]; every array starts as `fill` / `pred_fill`"""
        acc = np.ascontiguousarray(acc, np.float64)
        votes = np.ascontiguousarray(votes, np.int32)
        n, c = votes.shape
        ld_mp = ld_mp or c
        ab = self.buf(acc if n else np.zeros(1, np.float64))
        vb = self.buf(votes if n else np.zeros(1, np.int32))
        bufs = {}
        for name in self.MC_OUTPUTS:
            if name not in outputs:
                continue
            if name == "mean_prob":
                bufs[name] = self.buf(np.full((max(n, 1), ld_mp), fill, np.float32))
            elif name == "pred":
                bufs[name] = self.buf(np.full(max(n, 1), pred_fill, np.int32))
            else:
                bufs[name] = self.buf(np.full(max(n, 1), fill, np.float32))
        ptr = lambda name: bufs[name].ptr if name in bufs else None
        rc = self.lib.gcnhip_mc_finalize_rows(self.ctx, ab.ptr, vb.ptr, n, c, int(samples), ptr("mean_prob"), ld_mp, ptr("pred"), ptr("confidence"),
                                              ptr("entropy"), ptr("expected_entropy"), ptr("mutual_information"), ptr("variation_ratio"))
        if rc != 0:
            raise GcnHipError(f"gcnhip_mc_finalize_rows: error {rc}: {self.lib.gcnhip_last_error().decode()}")
        return {name: b.download()[:n] for name, b in bufs.items()}

    # ---- split conformal prediction sets (csrc/conformal.hip)
    def conformal_scores(self, logp, beta, method, lam=0.0, k_reg=0, rows=None, ld=None, ld_out=None, fill=np.nan, n=None):
        """gcnhip_conformal_scores: out [n_table, ld_out] — rows not listed and padding columns keep `fill`.  logp f32 [n_table, C]
        (uploaded with row stride ld, NaN padding); method 0 lac, 1 aps; rows: the listed rows (None: rows 0 .. n - 1)"""
        lb, _, rb, n_table, c, listed = self._calib_inputs(logp, ld, None, rows)
        ld_out = ld_out or c
        ob = self.buf(np.full((max(n_table, 1), ld_out), fill, np.float32))
        rc = self.lib.gcnhip_conformal_scores(self.ctx, lb.ptr, ld or c, n_table, rb.ptr if rb else None, listed if n is None else int(n), c, float(beta),
                                              int(method), float(lam), int(k_reg), ob.ptr, ld_out)
        if rc != 0:
            raise GcnHipError(f"gcnhip_conformal_scores: error {rc}: {self.lib.gcnhip_last_error().decode()}")
        return ob.download()[:n_table]

    def conformal_true_scores(self, table, truth, rows=None, ld=None, fill=np.nan):
        """gcnhip_conformal_true_scores: f32 [n listed] = table[r, truth[r]], -1 for an id outside the table or a truth outside
        [0, C).  table f32 [n_table, C] (uploaded with row stride ld, NaN padding)"""
        tb, hb, rb, n_table, c, listed = self._calib_inputs(table, ld, truth, rows)
        sb = self.buf(np.full(max(listed, 1), fill, np.float32))
        rc = self.lib.gcnhip_conformal_true_scores(self.ctx, tb.ptr, ld or c, hb.ptr, n_table, rb.ptr if rb else None, listed, c, sb.ptr)
        if rc != 0:
            raise GcnHipError(f"gcnhip_conformal_true_scores: error {rc}: {self.lib.gcnhip_last_error().decode()}")
        return sb.download()[:listed]

    def conformal_sets_rows(self, table, thresh, truth=None, rows=None, ld=None, bits=True, size=True, counts=True):
        """gcnhip_conformal_sets_rows: (sets bool [n listed, C], size int32 [n listed], counts int32 [4 + 3 C + 1]), None for an
        output that was not asked for; the outputs are uploaded as garbage — the launch zeroes or overwrites them.  thresh f32 [C]"""
        tb, hb, rb, n_table, c, listed = self._calib_inputs(table, ld, truth, rows)
        wpr = (c + 31) // 32
        th = self.buf(np.ascontiguousarray(thresh, np.float32))
        bb = self.buf(np.full((max(listed, 1), wpr), 0xdeadbeef, np.uint32)) if bits else None
        zb = self.buf(np.full(max(listed, 1), -777, np.int32)) if size else None
        cb = self.buf(np.full(4 + 3 * c + 1, 12345, np.int32)) if counts else None
        rc = self.lib.gcnhip_conformal_sets_rows(self.ctx, tb.ptr, ld or c, n_table, rb.ptr if rb else None, listed, c, th.ptr, hb.ptr if hb else None,
                                                 bb.ptr if bb else None, zb.ptr if zb else None, cb.ptr if cb else None)
        if rc != 0:
            raise GcnHipError(f"gcnhip_conformal_sets_rows: error {rc}: {self.lib.gcnhip_last_error().decode()}")
        return (unpack_multihot(bb.download()[:listed], c) if bits else None, zb.download()[:listed] if size else None,
                cb.download() if counts else None)

    # ---- ranking metrics (csrc/ranking.hip)
    def rank_keys(self, table, c0=0, c1=None, truth=None, truth_bits=None, rows=None, ld=None, stride=None, fill=0x5A5A5A5A, n=None):
        """gcnhip_rank_keys: (pos_keys, neg_keys uint32 [c1 - c0, stride], pos, neg, invalid int32 [c1 - c0], unlabelled int).
        table f32 [n_table, C] (uploaded with row stride ld, NaN padding); truth int32 [n_table] OR truth_bits bool [n_table, C];
        rows: the listed rows (None: rows 0 .. n_table - 1).  The key tables are uploaded holding `fill`, the counts as garbage."""
        lb, tb, rb, n_table, c, listed = self._calib_inputs(table, ld, truth, rows)
        listed = listed if n is None else int(n)
        c1 = c if c1 is None else int(c1)
        s, stride = max(c1 - c0, 1), int(stride or max(listed, 1))
        words = pack_multihot(truth_bits) if truth_bits is not None else None
        wb = self.buf(words if words.size else np.zeros(1, np.uint32)) if words is not None else None
        pk, nk = self.buf(np.full((s, stride), fill, np.uint32)), self.buf(np.full((s, stride), fill, np.uint32))
        cnt = [self.buf(np.full(s, 12345, np.int32)) for _ in range(3)]
        ub = self.buf(np.full(1, -777, np.int32))
        rc = self.lib.gcnhip_rank_keys(self.ctx, lb.ptr, ld or c, n_table, rb.ptr if rb else None, listed, int(c0), c1, c, tb.ptr if tb else None,
                                       wb.ptr if wb else None, words.shape[1] if words is not None else 0, pk.ptr, nk.ptr, stride, cnt[0].ptr,
                                       cnt[1].ptr, cnt[2].ptr, ub.ptr)
        if rc != 0:
            raise GcnHipError(f"gcnhip_rank_keys: error {rc}: {self.lib.gcnhip_last_error().decode()}")
        return pk.download(), nk.download(), cnt[0].download(), cnt[1].download(), cnt[2].download(), int(ub.download()[0])

    def sort_segments(self, keys, n=None, segments=None, scratch_fill=0xC3C3C3C3, scratch=True, return_scratch=False):
        """gcnhip_sort_segments_u32: keys uint32 [S, stride] with the first n (default: stride) keys of every row sorted ascending;
        the scratch table is uploaded holding `scratch_fill` and returned too when asked for."""
        keys = np.ascontiguousarray(keys, np.uint32)
        s, stride = keys.shape
        kb = self.buf(keys if keys.size else np.zeros(1, np.uint32))
        sb = self.buf(np.full(max(keys.size, 1), scratch_fill, np.uint32)) if scratch else None
        rc = self.lib.gcnhip_sort_segments_u32(self.ctx, kb.ptr, sb.ptr if sb else None, stride if n is None else int(n),
                                               s if segments is None else int(segments), stride)
        if rc != 0:
            raise GcnHipError(f"gcnhip_sort_segments_u32: error {rc}: {self.lib.gcnhip_last_error().decode()}")
        out = kb.download()[:keys.size].reshape(s, stride)
        return (out, sb.download()[:keys.size].reshape(s, stride)) if return_scratch else out

    def rank_stats(self, pos_keys, neg_keys, pos, neg, n=None):
        """gcnhip_rank_stats: (u2 int64 [S], ap_sum float64 [S]) from two sorted key tables uint32 [S, stride] and their valid
        lengths pos / neg int32 [S]; n: the keys per class (default: stride).  The outputs are uploaded as garbage."""
        pos_keys, neg_keys = np.ascontiguousarray(pos_keys, np.uint32), np.ascontiguousarray(neg_keys, np.uint32)
        s, stride = pos_keys.shape
        assert neg_keys.shape == pos_keys.shape
        pk, nk = self.buf(pos_keys), self.buf(neg_keys)
        pb, nb = self.buf(np.ascontiguousarray(pos, np.int32)), self.buf(np.ascontiguousarray(neg, np.int32))
        work = self.buf(np.full(s * RANK_STATS_BLOCKS * 2, np.nan, np.float64))
        ub, ab = self.buf(np.full(s, -777, np.int64)), self.buf(np.full(s, np.nan, np.float64))
        rc = self.lib.gcnhip_rank_stats(self.ctx, pk.ptr, nk.ptr, stride, stride if n is None else int(n), s, pb.ptr, nb.ptr, work.ptr, ub.ptr, ab.ptr)
        if rc != 0:
            raise GcnHipError(f"gcnhip_rank_stats: error {rc}: {self.lib.gcnhip_last_error().decode()}")
        return ub.download(), ab.download()

    # ---- multi-label decision thresholds (csrc/thresholds.hip)
    def threshold_scan(self, pos_keys, neg_keys, pos, neg, beta=1.0, n=None):
        """gcnhip_threshold_scan: (threshold f32 [S], counts int32 [3, S] = TP, FP, FN at it, f float64 [S], defined int32 [S])
        from two sorted key tables uint32 [S, stride] and their valid lengths pos / neg int32 [S]; n: the keys per class
        (default: stride).  The outputs are uploaded as garbage."""
        pos_keys, neg_keys = np.ascontiguousarray(pos_keys, np.uint32), np.ascontiguousarray(neg_keys, np.uint32)
        s, stride = pos_keys.shape
        assert neg_keys.shape == pos_keys.shape
        pk, nk = self.buf(pos_keys), self.buf(neg_keys)
        pb, nb = self.buf(np.ascontiguousarray(pos, np.int32)), self.buf(np.ascontiguousarray(neg, np.int32))
        work = self.buf(np.full(s * THRESHOLD_SCAN_BLOCKS * 2, np.nan, np.float64))
        tb, cb = self.buf(np.full(s, np.nan, np.float32)), self.buf(np.full(3 * s, 0x5A5A5A5A, np.int32))
        fb, db = self.buf(np.full(s, np.nan, np.float64)), self.buf(np.full(s, -777, np.int32))
        rc = self.lib.gcnhip_threshold_scan(self.ctx, pk.ptr, nk.ptr, stride, stride if n is None else int(n), s, pb.ptr, nb.ptr, float(beta), work.ptr,
                                            tb.ptr, cb.ptr, fb.ptr, db.ptr)
        if rc != 0:
            raise GcnHipError(f"gcnhip_threshold_scan: error {rc}: {self.lib.gcnhip_last_error().decode()}")
        return tb.download(), cb.download().reshape(3, s), fb.download(), db.download()

    # ---- node embeddings (csrc/embed.hip): the table is uploaded with row stride ld and NaN padding
    def _embed_inputs(self, table, ld, inv_norm):
        table = np.ascontiguousarray(table, np.float32)
        n_table, dim = table.shape
        tb = self.padded(table, ld or dim) if n_table else self.buf(np.full((1, ld or dim), np.nan, np.float32))
        nb = None if inv_norm is None else self.buf(np.ascontiguousarray(inv_norm, np.float32) if n_table else np.zeros(1, np.float32))
        return tb, nb, n_table, dim, int(ld or dim)

    def _embed_fail(self, what, rc):
        raise GcnHipError(f"{what}: error {rc}: {self.lib.gcnhip_last_error().decode()}")

    def embed_inv_norms(self, table, ld=None):
        """gcnhip_embed_inv_norms: f32 [n_table] = 1 / sqrt(sum of squares) of every row, exactly 0 for an all-zero row"""
        tb, _, n_table, dim, ld = self._embed_inputs(table, ld, None)
        ob = self.buf(np.full(max(n_table, 1), np.nan, np.float32))
        rc = self.lib.gcnhip_embed_inv_norms(self.ctx, tb.ptr, ld, n_table, dim, ob.ptr)
        if rc != 0:
            self._embed_fail("gcnhip_embed_inv_norms", rc)
        return ob.download()[:n_table]

    def topk_plan(self, n_table, nq, k, chunk_rows=0):
        """gcnhip_topk_plan: dict(chunk_rows, n_chunks, scratch_bytes, scratch_bytes_min) of a gcnhip_topk_rows call"""
        rows, chunks = C.c_int(), C.c_int()
        full, least = C.c_size_t(), C.c_size_t()
        rc = self.lib.gcnhip_topk_plan(int(n_table), int(nq), int(k), int(chunk_rows), C.byref(rows), C.byref(chunks), C.byref(full), C.byref(least))
        if rc != 0:
            self._embed_fail("gcnhip_topk_plan", rc)
        return dict(chunk_rows=rows.value, n_chunks=chunks.value, scratch_bytes=full.value, scratch_bytes_min=least.value)

    def topk_rows(self, table, q_rows, k, inv_norm=None, row_id=None, exclude_self=True, chunk_rows=0, ld=None, scratch_bytes=None, launches=3,
                  plan=False):
        """gcnhip_topk_rows: (ids int32 [nq, k], scores f32 [nq, k]) — the k best rows of `table` per listed query row, by dot
        product (inv_norm None) or cosine (inv_norm: embed_inv_norms of the table), best first, equal scores by ascending id
        (row_id[c], or c).  The outputs are uploaded as garbage.  scratch_bytes: the caller's scratch (None: room for every query
        at once); plan=True: a third value, topk_plan's dict for this call."""
        tb, nb, n_table, dim, ld = self._embed_inputs(table, ld, inv_norm)
        q = np.ascontiguousarray(q_rows, np.int32).ravel()
        nq, k = int(q.size), int(k)
        qb = self.buf(q if nq else np.zeros(1, np.int32))
        rb = None if row_id is None else self.buf(np.ascontiguousarray(row_id, np.int32))
        info = self.topk_plan(n_table, nq, k, chunk_rows)
        sbytes = info["scratch_bytes"] if scratch_bytes is None else int(scratch_bytes)
        sb = self.buf(np.full(max(sbytes // 4, 4), 0x7fc12345, np.uint32))
        ib = self.buf(np.full(max(nq * k, 1), 12345, np.int32))
        ob = self.buf(np.full(max(nq * k, 1), np.nan, np.float32))
        rc = self.lib.gcnhip_topk_rows(self.ctx, tb.ptr, ld, n_table, dim, nb.ptr if nb else None, rb.ptr if rb else None, qb.ptr, nq, k,
                                       int(bool(exclude_self)), int(chunk_rows), sb.ptr, sbytes, int(launches), ib.ptr, ob.ptr)
        if rc != 0:
            self._embed_fail("gcnhip_topk_rows", rc)
        out = ib.download()[:nq * k].reshape(nq, k), ob.download()[:nq * k].reshape(nq, k)
        return out + (info,) if plan else out

    def pair_scores(self, table, src, dst, inv_norm=None, ld=None):
        """gcnhip_pair_scores: f32 [m] = the score (dot, or cosine with inv_norm) of the listed row pairs"""
        tb, nb, n_table, dim, ld = self._embed_inputs(table, ld, inv_norm)
        s, d = np.ascontiguousarray(src, np.int32).ravel(), np.ascontiguousarray(dst, np.int32).ravel()
        assert s.size == d.size
        m = int(s.size)
        sb, db = self.buf(s if m else np.zeros(1, np.int32)), self.buf(d if m else np.zeros(1, np.int32))
        ob = self.buf(np.full(max(m, 1), np.nan, np.float32))
        rc = self.lib.gcnhip_pair_scores(self.ctx, tb.ptr, ld, n_table, dim, nb.ptr if nb else None, sb.ptr, db.ptr, m, ob.ptr)
        if rc != 0:
            self._embed_fail("gcnhip_pair_scores", rc)
        return ob.download()[:m]

    def embed_rows(self, table, rows=None, inv_norm=None, ld=None, ld_out=None, fill=np.nan):
        """gcnhip_embed_rows: f32 [n, dim] = the listed rows of the table (None: every row), times inv_norm of the row when given"""
        tb, nb, n_table, dim, ld = self._embed_inputs(table, ld, inv_norm)
        r = None if rows is None else np.ascontiguousarray(rows, np.int32).ravel()
        n = n_table if r is None else int(r.size)
        rb = None if r is None else self.buf(r if n else np.zeros(1, np.int32))
        ld_out = int(ld_out or dim)
        ob = self.buf(np.full((max(n, 1), ld_out), fill, np.float32))
        rc = self.lib.gcnhip_embed_rows(self.ctx, tb.ptr, ld, n_table, dim, nb.ptr if nb else None, rb.ptr if rb else None, n, ob.ptr, ld_out)
        if rc != 0:
            self._embed_fail("gcnhip_embed_rows", rc)
        return ob.download()[:n, :dim]

    # ---- k-means on the rows of a table (csrc/kmeans.hip): table and centres are uploaded with their row strides and NaN padding
    def _kmeans_rows(self, rows, n_table):
        r = None if rows is None else np.ascontiguousarray(rows, np.int32).ravel()
        n = n_table if r is None else int(r.size)
        return (None if r is None else self.buf(r if n else np.zeros(1, np.int32))), n

    def kmeans_plan(self, n, k, dim):
        """gcnhip_kmeans_plan: dict(update_bytes, update_bytes_min, seed_bytes) of device scratch"""
        a, b, s = C.c_size_t(), C.c_size_t(), C.c_size_t()
        rc = self.lib.gcnhip_kmeans_plan(int(n), int(k), int(dim), C.byref(a), C.byref(b), C.byref(s))
        if rc != 0:
            self._embed_fail("gcnhip_kmeans_plan", rc)
        return dict(update_bytes=a.value, update_bytes_min=b.value, seed_bytes=s.value)

    def kmeans_assign(self, table, centers, cn, rows=None, inv_norm=None, prev=None, ld=None, ldm=None):
        """gcnhip_kmeans_assign: (assign int32 [n], dist2 f32 [n], moved) — per list position (rows None: every row) the centre
        with the smallest cn[c] - 2 (dot . inv_norm), the lowest c on equal values; -1 / NaN for a row outside the table.  The
        outputs are uploaded as garbage."""
        tb, nb, n_table, dim, ld = self._embed_inputs(table, ld, inv_norm)
        centers = np.ascontiguousarray(centers, np.float32)
        k, ldm = centers.shape[0], int(ldm or dim)
        mb = self.padded(centers, ldm)
        cb = self.buf(np.ascontiguousarray(cn, np.float32).ravel())
        rb, n = self._kmeans_rows(rows, n_table)
        pb = None if prev is None else self.buf(np.ascontiguousarray(prev, np.int32).ravel() if n else np.zeros(1, np.int32))
        ab = self.buf(np.full(max(n, 1), 12345, np.int32))
        db = self.buf(np.full(max(n, 1), 7.5, np.float32))
        fb = self.buf(np.full(1, -777, np.int32))
        rc = self.lib.gcnhip_kmeans_assign(self.ctx, tb.ptr, ld, n_table, dim, nb.ptr if nb else None, rb.ptr if rb else None, n, mb.ptr, ldm, cb.ptr, k,
                                           pb.ptr if pb else None, ab.ptr, db.ptr, fb.ptr)
        if rc != 0:
            self._embed_fail("gcnhip_kmeans_assign", rc)
        return ab.download()[:n], db.download()[:n], int(fb.download()[0])

    def kmeans_update(self, table, assign, centers, dist2=None, rows=None, inv_norm=None, ld=None, ldm=None, scratch_bytes=None):
        """gcnhip_kmeans_update: dict(centers f32 [k, dim], sizes int32 [k], cn f32 [k], inertia float) — the float64 mean of every
        centre's members in ascending list position (an empty centre keeps its row of `centers`).  scratch_bytes: the caller's
        scratch (None: gcnhip_kmeans_plan's update_bytes)."""
        tb, nb, n_table, dim, ld = self._embed_inputs(table, ld, inv_norm)
        centers = np.ascontiguousarray(centers, np.float32)
        k, ldm = centers.shape[0], int(ldm or dim)
        mb = self.padded(centers, ldm)
        rb, n = self._kmeans_rows(rows, n_table)
        a = np.ascontiguousarray(assign, np.int32).ravel()
        assert a.size == n, (a.size, n)
        ab = self.buf(a if n else np.zeros(1, np.int32))
        db = None if dist2 is None else self.buf(np.ascontiguousarray(dist2, np.float32).ravel() if n else np.zeros(1, np.float32))
        sbytes = self.kmeans_plan(n, k, dim)["update_bytes"] if scratch_bytes is None else int(scratch_bytes)
        sb = self.buf(np.full(max(sbytes // 4, 4), 0x7fc12345, np.uint32))
        zb, cb, ib = self.buf(np.full(k, -777, np.int32)), self.buf(np.full(k, np.nan, np.float32)), self.buf(np.full(1, np.nan, np.float64))
        rc = self.lib.gcnhip_kmeans_update(self.ctx, tb.ptr, ld, n_table, dim, nb.ptr if nb else None, rb.ptr if rb else None, n, ab.ptr,
                                           db.ptr if db else None, k, mb.ptr, ldm, zb.ptr, cb.ptr, ib.ptr, sb.ptr, sbytes)
        if rc != 0:
            self._embed_fail("gcnhip_kmeans_update", rc)
        return dict(centers=mb.download()[:, :dim].copy(), sizes=zb.download(), cn=cb.download(), inertia=float(ib.download()[0]))

    def kmeans_seed(self, table, k, stream_seed, rows=None, inv_norm=None, ld=None, ldm=None):
        """gcnhip_kmeans_seed: (seed_pos int32 [k], centers f32 [k, dim]) — k-means++ by an exponential race on the Philox stream
        `stream_seed` (the caller's seed ^ KEY_KMEANS)"""
        tb, nb, n_table, dim, ld = self._embed_inputs(table, ld, inv_norm)
        k, ldm = int(k), int(ldm or dim)
        mb = self.buf(np.full((max(k, 1), ldm), np.nan, np.float32))
        rb, n = self._kmeans_rows(rows, n_table)
        pb = self.buf(np.full(max(k, 1), -777, np.int32))
        sbytes = self.kmeans_plan(n, k, dim)["seed_bytes"] if 1 <= k <= 256 else 1024
        sb = self.buf(np.full(max(sbytes // 4, 4), 0x7fc12345, np.uint32))
        rc = self.lib.gcnhip_kmeans_seed(self.ctx, tb.ptr, ld, n_table, dim, nb.ptr if nb else None, rb.ptr if rb else None, n, k,
                                         int(stream_seed) & ((1 << 64) - 1), mb.ptr, ldm, pb.ptr, sb.ptr, sbytes)
        if rc != 0:
            self._embed_fail("gcnhip_kmeans_seed", rc)
        return pb.download()[:k], mb.download()[:k, :dim].copy()

    def contingency_rows(self, assign, truth, k, num_classes, rows=None):
        """gcnhip_contingency_rows: (counts int32 [k, C], skipped) — counts[a, y] = list positions with assign a whose row's truth is y"""
        t = np.ascontiguousarray(truth, np.int32).ravel()
        rb, n = self._kmeans_rows(rows, int(t.size))
        a = np.ascontiguousarray(assign, np.int32).ravel()
        assert a.size == n, (a.size, n)
        ab, tb = self.buf(a if n else np.zeros(1, np.int32)), self.buf(t if t.size else np.zeros(1, np.int32))
        cb = self.buf(np.full(max(int(k) * int(num_classes), 1), 0x5A5A5A5A, np.int32))
        kb = self.buf(np.full(1, -777, np.int32))
        rc = self.lib.gcnhip_contingency_rows(self.ctx, ab.ptr, tb.ptr, int(t.size), rb.ptr if rb else None, n, int(k), int(num_classes), cb.ptr, kb.ptr)
        if rc != 0:
            self._embed_fail("gcnhip_contingency_rows", rc)
        return cb.download()[:int(k) * int(num_classes)].reshape(int(k), int(num_classes)), int(kb.download()[0])

    # ---- silhouette widths of a labelling of a table's rows (csrc/silhouette.hip)
    def silhouette_plan(self, n, k, dim):
        """gcnhip_silhouette_plan: dict(bytes, bytes_min) of device scratch for gcnhip_silhouette_sums"""
        a, b = C.c_size_t(), C.c_size_t()
        rc = self.lib.gcnhip_silhouette_plan(int(n), int(k), int(dim), C.byref(a), C.byref(b))
        if rc != 0:
            self._embed_fail("gcnhip_silhouette_plan", rc)
        return dict(bytes=a.value, bytes_min=b.value)

    def silhouette_sums(self, table, labels, k, rows=None, inv_norm=None, ld=None, scratch_bytes=None):
        """gcnhip_silhouette_sums: (sums float64 [n, k], sizes int32 [k]) — sums[i, c] = the sum of the Euclidean distances from list
        position i to the points of label c (the pair (i, i) left out by position); 0 in the row of a position that is no point.
        scratch_bytes: the caller's scratch (None: gcnhip_silhouette_plan's bytes).  The outputs are uploaded as garbage."""
        tb, nb, n_table, dim, ld = self._embed_inputs(table, ld, inv_norm)
        rb, n = self._kmeans_rows(rows, n_table)
        k = int(k)
        lab = np.ascontiguousarray(labels, np.int32).ravel()
        assert lab.size == n, (lab.size, n)
        lb = self.buf(lab if n else np.zeros(1, np.int32))
        sbytes = self.silhouette_plan(n, k, dim)["bytes"] if scratch_bytes is None else int(scratch_bytes)
        sb = self.buf(np.full(max(sbytes // 4, 4), 0x7fc12345, np.uint32))
        ob = self.buf(np.full(max(n * max(k, 1), 1), np.nan, np.float64))
        zb = self.buf(np.full(max(k, 1), -777, np.int32))
        rc = self.lib.gcnhip_silhouette_sums(self.ctx, tb.ptr, ld, n_table, dim, nb.ptr if nb else None, rb.ptr if rb else None, n, lb.ptr, k, ob.ptr,
                                             zb.ptr, sb.ptr, sbytes)
        if rc != 0:
            self._embed_fail("gcnhip_silhouette_sums", rc)
        return ob.download()[:n * k].reshape(n, k), zb.download()[:k]

    def silhouette_rows(self, sums, labels, sizes, n_table, rows=None):
        """gcnhip_silhouette_rows: dict(s, a, b float64 [n], neighbor int32 [n], cluster_sum float64 [k], total, points, excluded,
        nonempty) from the sums and sizes of silhouette_sums; NaN / -1 at a position that is no point."""
        sums = np.ascontiguousarray(sums, np.float64)
        n, k = sums.shape
        rb, n_list = self._kmeans_rows(rows, int(n_table))
        lab = np.ascontiguousarray(labels, np.int32).ravel()
        assert lab.size == n == n_list, (lab.size, n, n_list)
        ub = self.buf(sums.ravel() if sums.size else np.zeros(1, np.float64))
        lb = self.buf(lab if n else np.zeros(1, np.int32))
        zb = self.buf(np.ascontiguousarray(sizes, np.int32).ravel())
        sb, ab, bb = (self.buf(np.full(max(n, 1), 7.5, np.float64)) for _ in range(3))
        nbb = self.buf(np.full(max(n, 1), 12345, np.int32))
        cb, tb = self.buf(np.full(k, np.nan, np.float64)), self.buf(np.full(1, np.nan, np.float64))
        kb = self.buf(np.full(3, -777, np.int32))
        rc = self.lib.gcnhip_silhouette_rows(self.ctx, ub.ptr, lb.ptr, zb.ptr, rb.ptr if rb else None, int(n_table), n, k, sb.ptr, ab.ptr, bb.ptr,
                                             nbb.ptr, cb.ptr, tb.ptr, kb.ptr)
        if rc != 0:
            self._embed_fail("gcnhip_silhouette_rows", rc)
        cnt = kb.download()
        return dict(s=sb.download()[:n], a=ab.download()[:n], b=bb.download()[:n], neighbor=nbb.download()[:n], cluster_sum=cb.download()[:k],
                    total=float(tb.download()[0]), points=int(cnt[0]), excluded=int(cnt[1]), nonempty=int(cnt[2]))

    # ---- principal components of the rows of a table (csrc/pca.hip): the table is uploaded with its row stride and NaN padding,
    # every output as garbage
    def pca_plan(self, n, dim):
        """gcnhip_pca_plan: dict(bytes_full, bytes_min) of device scratch for pca_mean / pca_scatter"""
        a, b = C.c_size_t(), C.c_size_t()
        rc = self.lib.gcnhip_pca_plan(int(n), int(dim), C.byref(a), C.byref(b))
        if rc != 0:
            self._embed_fail("gcnhip_pca_plan", rc)
        return dict(bytes_full=a.value, bytes_min=b.value)

    def _pca_scratch(self, n, dim, scratch_bytes):
        sbytes = self.pca_plan(n, dim)["bytes_full"] if scratch_bytes is None else int(scratch_bytes)
        return self.buf(np.full(max(sbytes // 4, 4), 0x7fc12345, np.uint32)), sbytes

    def pca_mean(self, table, rows=None, inv_norm=None, ld=None, scratch_bytes=None):
        """gcnhip_pca_mean: (mean float64 [dim], count) — the float64 mean of the listed rows (None: every row) and the number of
        list positions that name a row of the table"""
        tb, nb, n_table, dim, ld = self._embed_inputs(table, ld, inv_norm)
        rb, n = self._kmeans_rows(rows, n_table)
        sb, sbytes = self._pca_scratch(n, dim, scratch_bytes)
        mb, cb = self.buf(np.full(dim, np.nan, np.float64)), self.buf(np.full(1, -777, np.int32))
        rc = self.lib.gcnhip_pca_mean(self.ctx, tb.ptr, ld, n_table, dim, nb.ptr if nb else None, rb.ptr if rb else None, n, mb.ptr, cb.ptr, sb.ptr, sbytes)
        if rc != 0:
            self._embed_fail("gcnhip_pca_mean", rc)
        return mb.download(), int(cb.download()[0])

    def pca_scatter(self, table, mean=None, rows=None, inv_norm=None, ld=None, scratch_bytes=None):
        """gcnhip_pca_scatter: float64 [dim, dim] = sum over the listed rows of c c^T, c = (double)x - mean (mean None: x)"""
        tb, nb, n_table, dim, ld = self._embed_inputs(table, ld, inv_norm)
        rb, n = self._kmeans_rows(rows, n_table)
        sb, sbytes = self._pca_scratch(n, dim, scratch_bytes)
        mb = None if mean is None else self.buf(np.ascontiguousarray(mean, np.float64).ravel())
        ob = self.buf(np.full(dim * dim, np.nan, np.float64))
        rc = self.lib.gcnhip_pca_scatter(self.ctx, tb.ptr, ld, n_table, dim, nb.ptr if nb else None, rb.ptr if rb else None, n, mb.ptr if mb else None,
                                         ob.ptr, sb.ptr, sbytes)
        if rc != 0:
            self._embed_fail("gcnhip_pca_scatter", rc)
        return ob.download().reshape(dim, dim)

    def pca_project(self, table, components, mean=None, scale=None, rows=None, inv_norm=None, ld=None, ldv=None, ldy=None):
        """gcnhip_pca_project: f32 [n, k] = (float)(scale[j] . sum_a c[i, a] . components[j, a]); components float64 [k, dim] (ROW j
        = component j; uploaded as the basis [dim x ldv] with NaN padding); a list position outside the table gives a NaN row"""
        tb, nb, n_table, dim, ld = self._embed_inputs(table, ld, inv_norm)
        rb, n = self._kmeans_rows(rows, n_table)
        comp = np.ascontiguousarray(components, np.float64)
        k = comp.shape[0]
        ldv, ldy = int(ldv or k), int(ldy or k)
        basis = np.full((comp.shape[1], max(ldv, 1)), np.nan, np.float64)
        basis[:, :min(k, ldv)] = comp.T[:, :min(k, ldv)]
        vb = self.buf(basis)
        mb = None if mean is None else self.buf(np.ascontiguousarray(mean, np.float64).ravel())
        cb = None if scale is None else self.buf(np.ascontiguousarray(scale, np.float64).ravel())
        ob = self.buf(np.full((max(n, 1), max(ldy, 1)), 12345.0, np.float32))
        rc = self.lib.gcnhip_pca_project(self.ctx, tb.ptr, ld, n_table, dim, nb.ptr if nb else None, rb.ptr if rb else None, n, mb.ptr if mb else None,
                                         vb.ptr, ldv, k, cb.ptr if cb else None, ob.ptr, ldy)
        if rc != 0:
            self._embed_fail("gcnhip_pca_project", rc)
        return ob.download().reshape(max(n, 1), max(ldy, 1))[:n, :k].copy()

    # ---- label structure of a graph (csrc/structure.hip): every output is uploaded as garbage, the calls zero their own
    def nbr_agreement(self, g, lab, num_classes, rows=None, n=None, want=("deg", "same", "known", "mix"), group=0, flush_every=0):
        """gcnhip_nbr_agreement(_ex) on a Graph: dict(deg, same, known int32 [n] by list position, mix int64 [C, C], class_rows int64
        [C], totals int64 [8], skipped) — the outputs not named in `want` are passed as NULL and come back as None.  rows: int32
        list of rows (None: positions 0 .. n - 1, n default the graph's rows).  group / flush_every: the lane group per row and
        the flush interval of the LDS histogram (0: the library's choice; anything else goes through gcnhip_nbr_agreement_ex)."""
        c = int(num_classes)
        lab = np.ascontiguousarray(lab, np.int32).ravel()
        assert lab.size == g.n_cols, (lab.size, g.n_cols)
        r = None if rows is None else np.ascontiguousarray(rows, np.int32).ravel()
        n = (g.n_rows if n is None else int(n)) if r is None else int(r.size)
        rb = None if r is None else self.buf(r if n > 0 else np.zeros(1, np.int32))
        lb = self.buf(lab if lab.size else np.zeros(1, np.int32))
        per = {k: (self.buf(np.full(max(n, 1), 0x5A5A5A5A, np.int32)) if k in want else None) for k in ("deg", "same", "known")}
        cc = max(c, 1) if 1 <= c <= 64 else 1
        mb = self.buf(np.full(cc * cc, 0x5A5A5A5A5A5A5A5A, np.int64)) if "mix" in want else None
        cb, tb, sb = self.buf(np.full(cc, -777, np.int64)), self.buf(np.full(8, -777, np.int64)), self.buf(np.full(1, -777, np.int64))
        args = (self.ctx, g.h, lb.ptr, c, rb.ptr if rb else None, n, per["deg"].ptr if per["deg"] else None, per["same"].ptr if per["same"] else None,
                per["known"].ptr if per["known"] else None, mb.ptr if mb else None, cb.ptr, tb.ptr, sb.ptr)
        if group or flush_every:
            rc = self.lib.gcnhip_nbr_agreement_ex(*args, int(group), int(flush_every))
        else:
            rc = self.lib.gcnhip_nbr_agreement(*args)
        if rc != 0:
            self._embed_fail("gcnhip_nbr_agreement", rc)
        out = {k: (b.download()[:n] if b is not None else None) for k, b in per.items()}
        out.update(mix=mb.download().reshape(c, c) if mb else None, class_rows=cb.download(), totals=tb.download(), skipped=int(sb.download()[0]))
        return out

    def strata_counts(self, deg, same, known, pred, truth, num_classes, bins, rows=None):
        """gcnhip_strata_counts: (strata int64 [32, bins + 1, 2], unlabelled) — pred and truth by row, deg / same / known by list
        position (rows None: position i is row i)"""
        pred, truth = np.ascontiguousarray(pred, np.int32).ravel(), np.ascontiguousarray(truth, np.int32).ravel()
        assert pred.size == truth.size
        d, s, k = (np.ascontiguousarray(a, np.int32).ravel() for a in (deg, same, known))
        n = int(d.size)
        assert s.size == n and k.size == n
        r = None if rows is None else np.ascontiguousarray(rows, np.int32).ravel()
        assert r is None or r.size == n
        one = np.zeros(1, np.int32)
        db, sb, kb = (self.buf(a if n else one) for a in (d, s, k))
        pb, tb = self.buf(pred if pred.size else one), self.buf(truth if truth.size else one)
        rb = None if r is None else self.buf(r if n else one)
        b = int(bins)
        cells = 32 * (b + 1) * 2 if 1 <= b <= 32 else 64
        ob, ub = self.buf(np.full(cells, 0x5A5A5A5A5A5A5A5A, np.int64)), self.buf(np.full(1, -777, np.int64))
        rc = self.lib.gcnhip_strata_counts(self.ctx, db.ptr, sb.ptr, kb.ptr, pb.ptr, tb.ptr, int(truth.size), rb.ptr if rb else None, n, int(num_classes), b,
                                           ob.ptr, ub.ptr)
        if rc != 0:
            self._embed_fail("gcnhip_strata_counts", rc)
        return ob.download().reshape(32, b + 1, 2), int(ub.download()[0])

    # ---- reach of a seed set and components (csrc/reach.hip): every output is uploaded as garbage, the calls write all of it
    REACH_SCRATCH = 64

    def hop_distance(self, g, seeds, max_hops=0, nearest=True, capacity=None, group=0, levels_per_sync=0):
        """gcnhip_hop_distance(_ex) on a Graph: dict(dist int32 [n_rows], nearest int32 [n_rows] or None, levels, level_counts int64
        [levels + 1] (cut at `capacity` entries when given), skipped).  group / levels_per_sync: the lane group per row and the
        level launches between two read-backs (0: the library's choice; anything else goes through gcnhip_hop_distance_ex)."""
        s = np.ascontiguousarray(seeds, np.int32).ravel()
        n = g.n_rows
        sb = self.buf(s if s.size else np.zeros(1, np.int32))
        db = self.buf(np.full(max(n, 1), 0x5A5A5A5A, np.int32))
        nb = self.buf(np.full(max(n, 1), 0x5A5A5A5A, np.int32)) if nearest else None
        scratch = self.buf(np.full(self.REACH_SCRATCH, -777, np.int64))
        cap = n + 1 if capacity is None else int(capacity)
        counts = np.full(max(cap, 1), -777, np.int64)
        levels, skipped = C.c_int(-777), C.c_int64(-777)
        args = (self.ctx, g.h, sb.ptr, int(s.size), int(max_hops), db.ptr, nb.ptr if nb else None, scratch.ptr, C.byref(levels),
                counts.ctypes.data if cap > 0 else None, cap, C.byref(skipped))
        if group or levels_per_sync:
            rc = self.lib.gcnhip_hop_distance_ex(*args, int(group), int(levels_per_sync) if levels_per_sync else 8)
        else:
            rc = self.lib.gcnhip_hop_distance(*args)
        if rc != 0:
            self._embed_fail("gcnhip_hop_distance", rc)
        assert capacity is not None or not counts[levels.value + 1:cap].any()
        return dict(dist=db.download()[:n], nearest=nb.download()[:n] if nb else None, levels=levels.value,
                    level_counts=counts[:min(levels.value + 1, cap)].copy(), skipped=skipped.value)

    def components(self, g):
        """gcnhip_components on a Graph: (comp int32 [n_rows], rounds)"""
        n = g.n_rows
        cb = self.buf(np.full(max(n, 1), 0x5A5A5A5A, np.int32))
        scratch = self.buf(np.full(self.REACH_SCRATCH, -777, np.int64))
        rounds = C.c_int(-777)
        rc = self.lib.gcnhip_components(self.ctx, g.h, cb.ptr, scratch.ptr, C.byref(rounds))
        if rc != 0:
            self._embed_fail("gcnhip_components", rc)
        return cb.download()[:n], rounds.value

    def component_counts(self, comp, mark=None):
        """gcnhip_component_counts: (size int32 [n], marked int32 [n], totals int64 [6])"""
        c = np.ascontiguousarray(comp, np.int32).ravel()
        n = int(c.size)
        one = np.zeros(1, np.int32)
        cb = self.buf(c if n else one)
        mb = None if mark is None else self.buf(np.ascontiguousarray(mark, np.int32).ravel() if n else one)
        assert mark is None or np.size(mark) == n
        sb, kb = self.buf(np.full(max(n, 1), 0x5A5A5A5A, np.int32)), self.buf(np.full(max(n, 1), 0x5A5A5A5A, np.int32))
        tb = self.buf(np.full(6, -777, np.int64))
        rc = self.lib.gcnhip_component_counts(self.ctx, cb.ptr, mb.ptr if mb else None, n, sb.ptr, kb.ptr, tb.ptr)
        if rc != 0:
            self._embed_fail("gcnhip_component_counts", rc)
        return sb.download()[:n], kb.download()[:n], tb.download()

    def distance_strata(self, dist, truth, num_classes, hops, nearest=None, pred=None, rows=None):
        """gcnhip_distance_strata: (strata int64 [hops + 2, 4], unlabelled) — dist / nearest / pred / truth by row, rows None:
        position i is row i"""
        d, t = np.ascontiguousarray(dist, np.int32).ravel(), np.ascontiguousarray(truth, np.int32).ravel()
        n_rows = int(d.size)
        assert t.size == n_rows
        one = np.zeros(1, np.int32)
        up = lambda a: None if a is None else self.buf(np.ascontiguousarray(a, np.int32).ravel() if np.size(a) else one)
        assert all(a is None or np.size(a) == n_rows for a in (nearest, pred))
        db, tb, nb, pb = up(d), up(t), up(nearest), up(pred)
        r = None if rows is None else np.ascontiguousarray(rows, np.int32).ravel()
        n = n_rows if r is None else int(r.size)
        rb = up(r)
        h = int(hops)
        cells = (h + 2) * 4 if 1 <= h <= 32 else 8
        ob, ub = self.buf(np.full(cells, 0x5A5A5A5A5A5A5A5A, np.int64)), self.buf(np.full(1, -777, np.int64))
        rc = self.lib.gcnhip_distance_strata(self.ctx, db.ptr, nb.ptr if nb else None, pb.ptr if pb else None, tb.ptr, n_rows, rb.ptr if rb else None, n,
                                             int(num_classes), h, ob.ptr, ub.ptr)
        if rc != 0:
            self._embed_fail("gcnhip_distance_strata", rc)
        return ob.download().reshape(h + 2, 4), int(ub.download()[0])

    # ---- new nodes attached to a trained graph (csrc/attach.hip): tables are uploaded with their row stride and NaN padding
    def attach_gather(self, ptr, col, coef, table_a, table_b, epilogue="none", beta=1.0, ld_a=None, ld_b=None, ld_out=None, logp=False,
                      store=True):
        """gcnhip_attach_gather: out f32 [m, dim] = epilogue(sum of coef[e] * row(col[e]) over ptr[i] <= e < ptr[i + 1]), row(c) = table_a[c]
        for c < n_a, else table_b[c - n_a].  epilogue "none" / "relu": returns out.  "predict": returns dict(pred int32 [m], prob f32 [m],
        logp f32 [m, dim] with logp=True, z = the stored logits unless store=False), the softmax taken of beta * z.  The outputs are
        uploaded as NaN / garbage.  m = len(ptr) - 1; table_b may hold more than m rows (some rows of a batch launched on their own)."""
        ptr, col = np.ascontiguousarray(ptr, np.int32).ravel(), np.ascontiguousarray(col, np.int32).ravel()
        coef = np.ascontiguousarray(coef, np.float32).ravel()
        ta, tb = np.ascontiguousarray(table_a, np.float32), np.ascontiguousarray(table_b, np.float32)
        m, n_a, dim = int(ptr.size) - 1, int(ta.shape[0]), int(tb.shape[1])
        assert tb.shape[0] >= m and ta.shape[1] == dim and col.size == coef.size == int(ptr[-1])
        ld_a, ld_b, ld_out = int(ld_a or dim), int(ld_b or dim), int(ld_out or dim)
        code = {"none": 0, "relu": 1, "predict": 2}[epilogue]
        pb = self.buf(ptr)
        cb, fb = self.buf(col if col.size else np.zeros(1, np.int32)), self.buf(coef if coef.size else np.zeros(1, np.float32))
        ab = self.padded(ta, ld_a) if n_a else None
        bb = self.padded(tb, ld_b) if m else self.buf(np.zeros(4, np.float32))
        ob = self.buf(np.full((max(m, 1), ld_out), np.nan, np.float32)) if (store or code != 2) else None
        qb = self.buf(np.full(max(m, 1), 12345, np.int32)) if code == 2 else None
        rb = self.buf(np.full(max(m, 1), np.nan, np.float32)) if code == 2 else None
        lb = self.buf(np.full((max(m, 1), dim), np.nan, np.float32)) if code == 2 and logp else None
        rc = self.lib.gcnhip_attach_gather(self.ctx, pb.ptr, cb.ptr, fb.ptr, m, ab.ptr if ab else None, ld_a, n_a, bb.ptr, ld_b, dim, code,
                                           ob.ptr if ob else None, ld_out, qb.ptr if qb else None, rb.ptr if rb else None, lb.ptr if lb else None, dim,
                                           float(beta))
        if rc != 0:
            self._embed_fail("gcnhip_attach_gather", rc)
        self.sync()
        if code != 2:
            return ob.download()[:m, :dim]
        res = dict(pred=qb.download()[:m], prob=rb.download()[:m])
        if lb:
            res["logp"] = lb.download()[:m]
        if ob:
            res["z"] = ob.download()[:m, :dim]
        return res

    # ---- explaining a logit (csrc/explain.hip): tables are uploaded with their row stride and NaN padding
    def _explain_inputs(self, q_row, q_class, h1, w2, ld_h1, ld_w2):
        qr, qc = np.ascontiguousarray(q_row, np.int32).ravel(), np.ascontiguousarray(q_class, np.int32).ravel()
        assert qr.size == qc.size
        nq = int(qr.size)
        h1, w2 = np.ascontiguousarray(h1, np.float32), np.ascontiguousarray(w2, np.float32)
        h, c = w2.shape
        assert h1.shape[1] == h
        ld_h1, ld_w2 = int(ld_h1 or h), int(ld_w2 or c)
        z = np.zeros(1, np.int32)
        return (self.buf(qr if nq else z), self.buf(qc if nq else z), nq, self.padded(h1, ld_h1), ld_h1, h, self.padded(w2, ld_w2), ld_w2, c)

    def explain_hops(self, g: "Graph", q_row, q_class, h1, w2, scaling=0, ld_h1=None, ld_w2=None, ld_out=None, nbr_ptr=None):
        """gcnhip_explain_hops: dict(logit f32 [nq], hidden f32 [nq, h], nbr_ptr int64 [nq + 1], nbr_row int32, nbr_val f32) of the
        listed (row, class) queries.  nbr_ptr: the exclusive scan handed to the library (None: made from the object's rows)."""
        qr, qc, nq, hb, ld_h1, h, wb, ld_w2, c = self._explain_inputs(q_row, q_class, h1, w2, ld_h1, ld_w2)
        indptr = g.csr()[0].astype(np.int64)
        rows = np.ascontiguousarray(q_row, np.int64).ravel()
        ok = (rows >= 0) & (rows < g.n_rows)
        length = np.where(ok, indptr[np.clip(rows, 0, g.n_rows - 1) + 1] - indptr[np.clip(rows, 0, g.n_rows - 1)], 0)
        ptr = np.concatenate([[0], np.cumsum(length)]) if nbr_ptr is None else np.asarray(nbr_ptr, np.int64)
        total = int(ptr[-1])
        ld_out = int(ld_out or h)
        pb = self.buf(ptr[:max(nq, 1)].astype(np.int32))
        lb = self.buf(np.full(max(nq, 1), np.nan, np.float32))
        ob = self.buf(np.full((max(nq, 1), ld_out), np.nan, np.float32))
        rb = self.buf(np.full(max(total, 1), -12345, np.int32))
        vb = self.buf(np.full(max(total, 1), np.nan, np.float32))
        rc = self.lib.gcnhip_explain_hops(self.ctx, g.h, qr.ptr, qc.ptr, nq, hb.ptr, ld_h1, h, wb.ptr, ld_w2, c, int(scaling), lb.ptr, ob.ptr, ld_out,
                                          pb.ptr, rb.ptr, vb.ptr, total)
        if rc != 0:
            self._embed_fail("gcnhip_explain_hops", rc)
        return dict(logit=lb.download()[:nq], hidden=ob.download()[:nq, :h], nbr_ptr=ptr, nbr_row=rb.download()[:total], nbr_val=vb.download()[:total])

    def explain_features_agg(self, g: "Graph", q_row, q_class, h1, w2, w1, s, scaling=0, ld_h1=None, ld_w2=None, ld_w1=None, ld_s=None, ld_f=None):
        """gcnhip_explain_features_agg: f32 [nq, F], the feature shares from dense rows of S = A^.X"""
        qr, qc, nq, hb, ld_h1, h, wb, ld_w2, c = self._explain_inputs(q_row, q_class, h1, w2, ld_h1, ld_w2)
        w1, s = np.ascontiguousarray(w1, np.float32), np.ascontiguousarray(s, np.float32)
        nf = w1.shape[0]
        assert w1.shape[1] == h and s.shape[1] == nf
        ld_w1, ld_s, ld_f = int(ld_w1 or h), int(ld_s or nf), int(ld_f or nf)
        w1b, sb = self.padded(w1, ld_w1), self.padded(s, ld_s)
        fb = self.buf(np.full((max(nq, 1), ld_f), np.nan, np.float32))
        rc = self.lib.gcnhip_explain_features_agg(self.ctx, g.h, qr.ptr, qc.ptr, nq, hb.ptr, ld_h1, h, wb.ptr, ld_w2, c, w1b.ptr, ld_w1, nf, sb.ptr, ld_s,
                                                  int(scaling), fb.ptr, ld_f)
        if rc != 0:
            self._embed_fail("gcnhip_explain_features_agg", rc)
        return fb.download()[:nq, :nf]

    def explain_features_walk(self, g: "Graph", x: "Feat", q_row, q_class, h1, w2, w1, scaling=0, ld_h1=None, ld_w2=None, ld_w1=None, ld_f=None):
        """gcnhip_explain_features_walk: f32 [nq, F], the feature shares by the two-hop walk over a feature object"""
        qr, qc, nq, hb, ld_h1, h, wb, ld_w2, c = self._explain_inputs(q_row, q_class, h1, w2, ld_h1, ld_w2)
        w1 = np.ascontiguousarray(w1, np.float32)
        nf = x.n_cols
        assert w1.shape == (nf, h)
        ld_w1, ld_f = int(ld_w1 or h), int(ld_f or nf)
        w1b = self.padded(w1, ld_w1)
        fb = self.buf(np.full((max(nq, 1), ld_f), np.nan, np.float32))
        rc = self.lib.gcnhip_explain_features_walk(self.ctx, g.h, x.h, qr.ptr, qc.ptr, nq, hb.ptr, ld_h1, h, wb.ptr, ld_w2, c, w1b.ptr, ld_w1, int(scaling),
                                                   fb.ptr, ld_f)
        if rc != 0:
            self._embed_fail("gcnhip_explain_features_walk", rc)
        return fb.download()[:nq, :nf]

    def explain_abs_colsum(self, batches, num_classes, ld_f=None):
        """gcnhip_explain_abs_colsum over `batches` = [(feat f32 [nq, F], q_class [nq]), ...] accumulated in order into zeroed sums:
        (acc float64 [C, F], count int32 [C])"""
        nf = int(np.asarray(batches[0][0]).shape[1])
        ld_f = int(ld_f or nf)
        ab = self.buf(np.zeros((num_classes, nf), np.float64))
        cb = self.buf(np.zeros(max(num_classes, 1), np.int32))
        for feat, cls in batches:
            feat = np.ascontiguousarray(feat, np.float32)
            cls = np.ascontiguousarray(cls, np.int32).ravel()
            nq = int(cls.size)
            fb = self.padded(feat, ld_f) if nq else self.buf(np.zeros((1, ld_f), np.float32))
            qb = self.buf(cls if nq else np.zeros(1, np.int32))
            rc = self.lib.gcnhip_explain_abs_colsum(self.ctx, fb.ptr, ld_f, qb.ptr, nq, nf, int(num_classes), ab.ptr, cb.ptr)
            if rc != 0:
                self._embed_fail("gcnhip_explain_abs_colsum", rc)
        return ab.download(), cb.download()[:num_classes]

    def graphsum(self, g: "Graph", x, ld_in=None, ld_out=None, row_nonzero=None):
        x = np.asarray(x, np.float32)
        dim = x.shape[1]
        ld_in = ld_in or dim
        ld_out = ld_out or dim
        xin = self.padded(x, ld_in)
        out = self.buf(np.full((g.n_rows, ld_out), np.nan, np.float32))
        g.reserve(dim)
        if row_nonzero is None:
            _ck(self.lib, self.lib.gcnhip_graphsum(self.ctx, g.h, xin.ptr, ld_in, out.ptr, ld_out, dim), "gcnhip_graphsum")
        else:
            bb = self._bits(row_nonzero)
            _ck(self.lib, self.lib.gcnhip_graphsum_rowmask(self.ctx, g.h, xin.ptr, ld_in, out.ptr, ld_out, dim, bb.ptr), "gcnhip_graphsum_rowmask")
        return out.download()[:, :dim]

    def gather_rows(self, x, rows):
        """dst[i] = x[rows[i]] through gcnhip_gather_rows (the packing step of the halo exchange)"""
        x = np.ascontiguousarray(x, np.float32)
        rows = np.ascontiguousarray(rows, np.int32)
        xb, rb = self.buf(x), self.buf(rows if rows.size else np.zeros(1, np.int32))
        out = self.buf(np.full((max(rows.size, 1), x.shape[1]), np.nan, np.float32))
        _ck(self.lib, self.lib.gcnhip_gather_rows(self.ctx, xb.ptr, x.shape[1], rb.ptr, int(rows.size), out.ptr), "gcnhip_gather_rows")
        return out.download()[:rows.size]

    def to_bf16(self, x, ld_dst=None):
        """f32 rows -> bf16 table (uint16 [rows, ld_dst]) through gcnhip_f32_to_bf16"""
        x = np.asarray(x, np.float32)
        rows, dim = x.shape
        ld_dst = ld_dst or (dim + 7) // 8 * 8
        xb = self.buf(np.ascontiguousarray(x))
        dst = self.buf(np.full((rows, ld_dst), 0xFFFF, np.uint16))
        _ck(self.lib, self.lib.gcnhip_f32_to_bf16(self.ctx, xb.ptr, dim, dst.ptr, ld_dst, rows, dim), "gcnhip_f32_to_bf16")
        return dst.download()

    def graphsum_bf16(self, g: "Graph", table_u16, dim, ld_out=None, row_nonzero=None, relu_dropout=None, out_rows=None, fill=np.nan):
        """GraphSum over a bf16 table (uint16 [n_cols, ld]); relu_dropout = dict(training, p, seed, epoch, elem_offset, keep_mask);
        out_rows: a handle from Graph.add_rowset (only those rows are computed, the others keep `fill`)"""
        t = np.ascontiguousarray(table_u16, np.uint16)
        ld_in = t.shape[1]
        ld_out = ld_out or dim
        tb = self.buf(t)
        out = self.buf(np.full((g.n_rows, ld_out), fill, np.float32))
        bb = self._bits(row_nonzero) if row_nonzero is not None else None
        rd = relu_dropout or {}
        g.reserve(dim)
        ep = self.buf(np.array([rd.get("epoch", 0)], np.uint32))
        km = self.buf(np.ascontiguousarray(rd["keep_mask"], np.uint8)) if rd.get("keep_mask") is not None else None
        _ck(self.lib, self.lib.gcnhip_graphsum_bf16(self.ctx, g.h, tb.ptr, ld_in, out.ptr, ld_out, dim, bb.ptr if bb else None,
                                                     out_rows,
                                                     1 if relu_dropout is not None else 0, int(rd.get("training", 0)), float(rd.get("p", 0.0)),
                                                     int(rd.get("seed", 0)), ep.ptr, int(rd.get("elem_offset", 0)), km.ptr if km else None),
            "gcnhip_graphsum_bf16")
        return out.download()[:, :dim]

    def graphsum_relu_dropout(self, g, x, training, p, seed=0, epoch=0, elem_offset=0, keep_mask=None, ld=None):
        x = np.asarray(x, np.float32)
        dim = x.shape[1]
        ld = ld or dim
        xin = self.padded(x, ld)
        out = self.buf(np.full((g.n_rows, ld), np.nan, np.float32))
        g.reserve(dim)
        ep = self.buf(np.array([epoch], np.uint32))
        km = self.buf(np.ascontiguousarray(keep_mask, np.uint8)) if keep_mask is not None else None
        _ck(self.lib, self.lib.gcnhip_graphsum_relu_dropout(self.ctx, g.h, xin.ptr, ld, out.ptr, ld, dim, int(training), p,
                                                             seed, ep.ptr, elem_offset, km.ptr if km else None), "graphsum_relu_dropout")
        return out.download()[:, :dim]

    def graphsum_relu_dropout_bits(self, g, x, training, p, seed=0, epoch=0, elem_offset=0, keep_mask=None, ld=None):
        """-> (out, bits [n_rows x dim/32] uint32): gcnhip_graphsum_relu_dropout_bits"""
        x = np.asarray(x, np.float32)
        dim = x.shape[1]
        ld = ld or dim
        wpr = (dim + 31) // 32
        xin = self.padded(x, ld)
        out = self.buf(np.full((g.n_rows, ld), np.nan, np.float32))
        bits = self.buf(np.full((g.n_rows, wpr), 0xDEADBEEF, np.uint32))
        g.reserve(dim)
        ep = self.buf(np.array([epoch], np.uint32))
        km = self.buf(np.ascontiguousarray(keep_mask, np.uint8)) if keep_mask is not None else None
        _ck(self.lib, self.lib.gcnhip_graphsum_relu_dropout_bits(self.ctx, g.h, xin.ptr, ld, out.ptr, ld, dim, int(training), p, seed, ep.ptr,
                                                                  elem_offset, km.ptr if km else None, bits.ptr, wpr), "graphsum_relu_dropout_bits")
        return out.download()[:, :dim], bits.download()

    # ---- the first-layer products.  Beside the operands: vals (a value array of the caller's instead of the object's own), a
    # row stride per table, shift = {operand name: floats} (that operand starts so many floats into its allocation: an
    # address that is not a multiple of 16 bytes), whole / fill (return the WHOLE written table, uploaded as `fill`, padding
    # columns included, as graphsum_blend does; with it `.base` of the result is the flat allocation: `shift` floats in
    # front of the table and SLACK_ROWS rows behind it, which no launch may touch)
    SLACK_ROWS = 2

    def _operand(self, arr, ld, shift=0, fill=np.nan):
        """a 2-D float table with row stride ld (padding = fill), `shift` floats into an allocation with SLACK_ROWS rows of slack
        behind it -> (Buf, device address of element [0, 0], floats of the table)"""
        arr = np.asarray(arr, np.float32)
        rows, cols = arr.shape
        flat = np.full(shift + (rows + self.SLACK_ROWS) * ld + 4, fill, np.float32)
        table = flat[shift:shift + rows * ld].reshape(rows, ld)
        table[:, :cols] = arr
        b = self.buf(flat)
        return b, b.ptr + 4 * shift, rows * ld

    @staticmethod
    def _table(buf, shift, rows, ld, cols, whole):
        flat = buf.download()
        table = flat[shift:shift + rows * ld].reshape(rows, ld)
        return table if whole else table[:, :cols].copy()

    def _vals(self, f, vals, shift):
        if vals is None:
            return None, f.values_ptr
        b, ptr, _ = self._operand(np.ascontiguousarray(vals, np.float32).reshape(1, -1), max(int(np.size(vals)), 1), shift)
        return b, ptr

    def spmm_fwd(self, f: "Feat", w, p_drop=0.0, seed=0, epoch=0, nnz_offset=0, keep_mask=None, vals=None, ld_w=None, ld_out=None,
                 whole=False, fill=np.nan, shift=None):
        w = np.asarray(w, np.float32)
        p = w.shape[1]
        ld_w = ld_w or p
        ld_out = ld_out or p
        sh = shift or {}
        wb, wptr, _ = self._operand(w, ld_w, sh.get("w", 0))
        out, optr, _ = self._operand(np.zeros((f.n_rows, 0), np.float32), ld_out, sh.get("out", 0), fill)
        ep = self.buf(np.array([epoch], np.uint32))
        km = self.buf(np.ascontiguousarray(keep_mask, np.uint8)) if keep_mask is not None else None
        vb, vptr = self._vals(f, vals, sh.get("vals", 0))
        _ck(self.lib, self.lib.gcnhip_spmm_fwd(self.ctx, f.h, vptr, wptr, ld_w, optr, ld_out, p, p_drop, seed, ep.ptr,
                                                nnz_offset, km.ptr if km else None), "gcnhip_spmm_fwd")
        return self._table(out, sh.get("out", 0), f.n_rows, ld_out, p, whole)

    def spmm_fwd_relu(self, f: "Feat", w, ld_w=None, ld_out=None, vals=None, whole=False, fill=np.nan, shift=None):
        """ReLU(X . w) through gcnhip_spmm_fwd_relu (the evaluation form on an aggregated feature object)"""
        w = np.asarray(w, np.float32)
        p = w.shape[1]
        ld_w, ld_out = ld_w or p, ld_out or p
        sh = shift or {}
        wb, wptr, _ = self._operand(w, ld_w, sh.get("w", 0))
        out, optr, _ = self._operand(np.zeros((f.n_rows, 0), np.float32), ld_out, sh.get("out", 0), fill)
        vb, vptr = self._vals(f, vals, sh.get("vals", 0))
        _ck(self.lib, self.lib.gcnhip_spmm_fwd_relu(self.ctx, f.h, vptr, wptr, ld_w, optr, ld_out, p), "gcnhip_spmm_fwd_relu")
        return self._table(out, sh.get("out", 0), f.n_rows, ld_out, p, whole)

    def spmm_fwd_relu_matmul(self, f: "Feat", w, w2, ld_z=None, vals=None, ld_w=None, ld_w2=None, whole=False, fill=np.nan, shift=None):
        """gcnhip_spmm_fwd_relu_matmul: ReLU(X . w) . w2 in one launch; returns None when the fused form is not available"""
        w, w2 = np.asarray(w, np.float32), np.asarray(w2, np.float32)
        p, p2 = w.shape[1], w2.shape[1]
        ld_z = ld_z or (p2 + 3) // 4 * 4
        ld_w, ld_w2 = ld_w or p, ld_w2 or ld_z
        sh = shift or {}
        wb, wptr, _ = self._operand(w, ld_w, sh.get("w", 0))
        w2b, w2ptr, _ = self._operand(w2, ld_w2, sh.get("w2", 0))
        z, zptr, _ = self._operand(np.zeros((f.n_rows, 0), np.float32), ld_z, sh.get("out", 0), fill)
        vb, vptr = self._vals(f, vals, sh.get("vals", 0))
        rc = self.lib.gcnhip_spmm_fwd_relu_matmul(self.ctx, f.h, vptr, wptr, ld_w, p, w2ptr, ld_w2, p2, zptr, ld_z)
        if rc == -2:
            return None
        _ck(self.lib, rc, "gcnhip_spmm_fwd_relu_matmul")
        return self._table(z, sh.get("out", 0), f.n_rows, ld_z, p2, whole)

    def spmm_bwd(self, f: "Feat", dout, p_drop=0.0, seed=0, epoch=0, nnz_offset=0, keep_mask=None, vals=None, ld_dout=None, ld_dw=None,
                 whole=False, fill=np.nan, shift=None):
        dout = np.asarray(dout, np.float32)
        p = dout.shape[1]
        ld_dout = ld_dout or p
        ld_dw = ld_dw or p
        sh = shift or {}
        db, dptr, _ = self._operand(dout, ld_dout, sh.get("dout", 0))
        dw, wptr, _ = self._operand(np.zeros((f.n_cols, 0), np.float32), ld_dw, sh.get("out", 0), fill)
        ep = self.buf(np.array([epoch], np.uint32))
        km = self.buf(np.ascontiguousarray(keep_mask, np.uint8)) if keep_mask is not None else None
        vb, vptr = self._vals(f, vals, sh.get("vals", 0))
        _ck(self.lib, self.lib.gcnhip_spmm_bwd(self.ctx, f.h, vptr, dptr, ld_dout, wptr, ld_dw, p, p_drop, seed, ep.ptr,
                                                nnz_offset, km.ptr if km else None), "gcnhip_spmm_bwd")
        return self._table(dw, sh.get("out", 0), f.n_cols, ld_dw, p, whole)

    def spmm_bwd_plan(self, f: "Feat", p):
        rps, ns = C.c_int(), C.c_int()
        _ck(self.lib, self.lib.gcnhip_spmm_bwd_plan(self.ctx, f.h, p, C.byref(rps), C.byref(ns)), "gcnhip_spmm_bwd_plan")
        return rps.value, ns.value

    def spmm_bwd_parts(self, f: "Feat", dout, cuts, p_drop=0.0, seed=0, epoch=0, nnz_offset=0, order=None, make_first=True, keep_mask=None,
                       vals=None, ld_dout=None, ld_dw=None, whole=False, fill=np.nan, shift=None):
        """the weight gradient as gcnhip_spmm_bwd_part calls on the split ranges between `cuts` (in `order`), then _finish;
        make_first=False: no part makes the keep decisions (a forward with the same arguments left them in the feature object)"""
        dout = np.asarray(dout, np.float32)
        p = dout.shape[1]
        ld_dout, ld_dw = ld_dout or p, ld_dw or p
        sh = shift or {}
        db, dptr, _ = self._operand(dout, ld_dout, sh.get("dout", 0))
        dw, wptr, _ = self._operand(np.zeros((f.n_cols, 0), np.float32), ld_dw, sh.get("out", 0), fill)
        ep = self.buf(np.array([epoch], np.uint32))
        km = self.buf(np.ascontiguousarray(keep_mask, np.uint8)) if keep_mask is not None else None
        vb, vptr = self._vals(f, vals, sh.get("vals", 0))
        ranges = list(zip(cuts[:-1], cuts[1:]))
        for k, i in enumerate(order if order is not None else range(len(ranges))):
            _ck(self.lib, self.lib.gcnhip_spmm_bwd_part(self.ctx, f.h, vptr, dptr, ld_dout, p, p_drop, seed, ep.ptr, nnz_offset,
                                                         km.ptr if km else None, ranges[i][0], ranges[i][1],
                                                         1 if (k == 0 and make_first) else 0), "gcnhip_spmm_bwd_part")
        _ck(self.lib, self.lib.gcnhip_spmm_bwd_finish(self.ctx, f.h, wptr, ld_dw, p), "gcnhip_spmm_bwd_finish")
        return self._table(dw, sh.get("out", 0), f.n_cols, ld_dw, p, whole)

    # ---- the Matmul products.  As above: a row stride per operand, shift = {operand name: floats} ("a", "b", "c", "dc", "da",
    # "db", "rowscale"; "bits": words), whole / fill for every output; da=False / db=False / bits=None pass NULL where the
    # entry point takes it.
    def matmul_fwd(self, a, b, lda=None, ldb=None, ldc=None, shift=None, whole=False, fill=np.nan):
        a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
        m, n = a.shape
        p = b.shape[1]
        lda, ldb, ldc = lda or n, ldb or p, ldc or p
        sh = shift or {}
        ab, aptr, _ = self._operand(a, lda, sh.get("a", 0))
        bb, bptr, _ = self._operand(b, ldb, sh.get("b", 0))
        cb, cptr, _ = self._operand(np.zeros((m, 0), np.float32), ldc, sh.get("c", 0), fill)
        _ck(self.lib, self.lib.gcnhip_matmul_fwd(self.ctx, aptr, lda, bptr, ldb, cptr, ldc, m, n, p), "gcnhip_matmul_fwd")
        return self._table(cb, sh.get("c", 0), m, ldc, p, whole)

    def _matmul_bwd_call(self, entry, a, b, dc, m, n, p, ld, scale=None, bits=None, rowscale=None, da=True, db=True, shift=None,
                         whole=False, fill=np.nan):
        """one call of gcnhip_matmul_<entry>; ld = dict(a, b, dc, da, db) -> (da, db) tables (None where not asked for)"""
        sh = shift or {}
        aptr = None
        if a is not None:
            ab, aptr, _ = self._operand(a, ld["a"], sh.get("a", 0))
        bb, bptr, _ = self._operand(b, ld["b"], sh.get("b", 0))
        dcb, dcptr, _ = self._operand(dc, ld["dc"], sh.get("dc", 0))
        dab = dbb = daptr = dbptr = btptr = rsptr = None
        if da:
            dab, daptr, _ = self._operand(np.zeros((m, 0), np.float32), ld["da"], sh.get("da", 0), fill)
        if db:
            dbb, dbptr, _ = self._operand(np.zeros((n, 0), np.float32), ld["db"], sh.get("db", 0), fill)
        wpr = 0
        if bits is not None:
            bits = np.ascontiguousarray(bits, np.uint32)
            wpr = bits.shape[1]
            s = sh.get("bits", 0)
            flat = np.full(s + (bits.shape[0] + self.SLACK_ROWS) * wpr + 4, 0xDEADBEEF, np.uint32)
            flat[s:s + bits.size] = bits.ravel()
            bt = self.buf(flat)
            btptr = bt.ptr + 4 * s
        if rowscale is not None:
            rs, rsptr, _ = self._operand(np.ascontiguousarray(rowscale, np.float32).reshape(1, -1), max(int(np.size(rowscale)), 1), sh.get("rowscale", 0))
        lib, x = self.lib, self.ctx
        head = (x, aptr, ld["a"], bptr, ld["b"], dcptr, ld["dc"], daptr, ld["da"], dbptr, ld["db"], m, n, p)
        if entry == "bwd":
            rc = lib.gcnhip_matmul_bwd(*head)
        elif entry == "bwd_fused":
            rc = lib.gcnhip_matmul_bwd_fused(*head, scale)
        elif entry == "bwd_fused_bits":
            rc = lib.gcnhip_matmul_bwd_fused_bits(*head, scale, btptr, wpr)
        elif entry == "bwd_ex":
            rc = lib.gcnhip_matmul_bwd_ex(*head, scale, btptr, wpr, rsptr)
        else:
            assert entry == "bwd_da_bits"
            rc = lib.gcnhip_matmul_bwd_da_bits(x, bptr, ld["b"], dcptr, ld["dc"], daptr, ld["da"], m, n, p, btptr, wpr, scale)
        _ck(lib, rc, "gcnhip_matmul_" + entry)
        return (self._table(dab, sh.get("da", 0), m, ld["da"], n, whole) if da else None,
                self._table(dbb, sh.get("db", 0), n, ld["db"], p, whole) if db else None)

    def matmul_bwd(self, a, b, dc, lda=None, ldb=None, lddc=None, fused_scale=None, ldda=None, lddb=None, da=True, db=True, **kw):
        """gcnhip_matmul_bwd, or gcnhip_matmul_bwd_fused when fused_scale is given (mask = a > 0)"""
        a, b, dc = (np.asarray(t, np.float32) for t in (a, b, dc))
        m, n = a.shape
        p = b.shape[1]
        lda, ldb, lddc = lda or n, ldb or p, lddc or p
        ld = dict(a=lda, b=ldb, dc=lddc, da=ldda or lda, db=lddb or ldb)
        return self._matmul_bwd_call("bwd" if fused_scale is None else "bwd_fused", a, b, dc, m, n, p, ld, scale=fused_scale, da=da, db=db, **kw)

    def matmul_bwd_fused_bits(self, a, b, dc, scale, bits, lda=None, ldb=None, lddc=None, ldda=None, lddb=None, db=True, **kw):
        a, b, dc = (np.asarray(t, np.float32) for t in (a, b, dc))
        m, n = a.shape
        p = b.shape[1]
        ldp = (p + 3) // 4 * 4
        ld = dict(a=lda or n, b=ldb or ldp, dc=lddc or ldp, da=ldda or n, db=lddb or ldp)
        return self._matmul_bwd_call("bwd_fused_bits", a, b, dc, m, n, p, ld, scale=scale, bits=bits, db=db, **kw)

    def matmul_bwd_ex(self, a, b, dc, scale, bits, rowscale=None, ldp=None, p=None, lda=None, ldb=None, lddc=None, ldda=None, lddb=None,
                      db=True, **kw):
        """gcnhip_matmul_bwd_ex: da = mask . (scale * rowscale[r]) . (dc . b^T), mask = bits (None: a > 0), db = a^T . dc; dc may
        come with its padding columns (p = the real width); a = None with db=False and bits given"""
        b, dc = np.asarray(b, np.float32), np.asarray(dc, np.float32)
        a = np.asarray(a, np.float32) if a is not None else None
        m, n = dc.shape[0], b.shape[0]
        p = p or b.shape[1]
        ldp = ldp or (p + 3) // 4 * 4
        ld = dict(a=lda or n, b=ldb or ldp, dc=lddc or ldp, da=ldda or n, db=lddb or ldp)
        return self._matmul_bwd_call("bwd_ex", a, b, dc, m, n, p, ld, scale=scale, bits=bits, rowscale=rowscale, db=db, **kw)

    def pack_positive(self, h, ld=None):
        """bit (r, c) = h[r, c] > 0, 32 columns per little-endian word -> uint32 [rows, ceil(dim/32)]"""
        h = np.asarray(h, np.float32)
        rows, dim = h.shape
        ld = ld or dim
        wpr = (dim + 31) // 32
        hb = self.padded(h, ld)
        bits = self.buf(np.full((rows, wpr), 0xFFFFFFFF, np.uint32))
        _ck(self.lib, self.lib.gcnhip_pack_positive(self.ctx, hb.ptr, ld, rows, dim, bits.ptr, wpr), "gcnhip_pack_positive")
        return bits.download()

    def matmul_bwd_da_bits(self, b, dc, bits, scale, ldb=None, lddc=None, ldda=None, **kw):
        b, dc = np.asarray(b, np.float32), np.asarray(dc, np.float32)
        n, p = b.shape
        m = dc.shape[0]
        ld = dict(a=0, b=ldb or p, dc=lddc or p, da=ldda or n, db=0)
        return self._matmul_bwd_call("bwd_da_bits", None, b, dc, m, n, p, ld, scale=scale, bits=bits, db=False, **kw)[0]

    def relu_fwd(self, x, training=True):
        x = np.ascontiguousarray(x, np.float32).reshape(-1)
        xb = self.buf(x)
        mb = self.buf(np.zeros(x.size, np.uint8))
        _ck(self.lib, self.lib.gcnhip_relu_fwd(self.ctx, xb.ptr, mb.ptr, x.size, int(training)), "gcnhip_relu_fwd")
        return xb.download(), mb.download()

    def relu_bwd(self, grad, mask):
        g = self.buf(np.ascontiguousarray(grad, np.float32).reshape(-1))
        mb = self.buf(np.ascontiguousarray(mask, np.uint8))
        _ck(self.lib, self.lib.gcnhip_relu_bwd(self.ctx, g.ptr, mb.ptr, g.shape[0]), "gcnhip_relu_bwd")
        return g.download()

    def dropout_fwd(self, x, p, seed=0, epoch=0, elem_offset=0, keep_in=None, want_mask=True):
        x = np.ascontiguousarray(x, np.float32).reshape(-1)
        xb = self.buf(x)
        mb = self.buf(np.zeros(x.size, np.int32)) if want_mask else None
        ep = self.buf(np.array([epoch], np.uint32))
        kb = self.buf(np.ascontiguousarray(keep_in, np.uint8)) if keep_in is not None else None
        _ck(self.lib, self.lib.gcnhip_dropout_fwd(self.ctx, xb.ptr, mb.ptr if mb else None, x.size, p, seed, ep.ptr, elem_offset,
                                                   kb.ptr if kb else None), "gcnhip_dropout_fwd")
        return xb.download(), (mb.download() if mb else None)

    def dropout_bwd(self, grad, mask, p):
        g = self.buf(np.ascontiguousarray(grad, np.float32).reshape(-1))
        mb = self.buf(np.ascontiguousarray(mask, np.int32))
        _ck(self.lib, self.lib.gcnhip_dropout_bwd(self.ctx, g.ptr, mb.ptr, g.shape[0], p), "gcnhip_dropout_bwd")
        return g.download()

    def relu_dropout_bwd(self, grad, h, scale, ld_grad=None, ld_h=None, dim=None):
        """gcnhip_relu_dropout_bwd.  Packed by default (grad and h are [rows, dim]).  With ld_grad / ld_h given, grad is the WHOLE
        buffer [rows, ld_grad] and h the whole buffer [rows, ld_h], padding included, `dim` (required then) the logical width;
        the whole grad buffer comes back, so the padding can be inspected."""
        grad, h = np.asarray(grad, np.float32), np.asarray(h, np.float32)
        if ld_grad is None and ld_h is None and dim is None:
            ld_grad, ld_h, dim = grad.shape[1], h.shape[1], grad.shape[1]
        else:
            ld_grad, ld_h = ld_grad or grad.shape[1], ld_h or h.shape[1]
            if dim is None or grad.shape[1] != ld_grad or h.shape[1] != ld_h or grad.shape[0] != h.shape[0]:
                raise ValueError("relu_dropout_bwd: the strided form takes whole buffers [rows, ld_grad], [rows, ld_h] and dim")
        g, hb = self.buf(np.ascontiguousarray(grad)), self.buf(np.ascontiguousarray(h))
        _ck(self.lib, self.lib.gcnhip_relu_dropout_bwd(self.ctx, g.ptr, ld_grad, hb.ptr, ld_h, grad.shape[0], dim, scale), "relu_dropout_bwd")
        return g.download()

    # ---- the strided forms (module.cpp's calls: ld > cols).  x / grad are WHOLE buffers [rows, ld], padding included, and come
    # back whole; masks and keep decisions are flat [rows . cols], keyed by r . cols + c
    def relu_fwd_2d(self, x, cols, training=True, mask_fill=0):
        """gcnhip_relu_fwd_2d -> (buffer [rows, ld], mask uint8 [rows . cols], uploaded as mask_fill)"""
        x = np.ascontiguousarray(x, np.float32)
        rows, ld = x.shape
        xb = self.buf(x)
        mb = self.buf(np.full(max(rows * cols, 1), mask_fill, np.uint8))
        _ck(self.lib, self.lib.gcnhip_relu_fwd_2d(self.ctx, xb.ptr, ld, rows, int(cols), mb.ptr, int(training)), "gcnhip_relu_fwd_2d")
        return xb.download(), mb.download()[:rows * cols]

    def relu_bwd_2d(self, grad, cols, mask):
        grad = np.ascontiguousarray(grad, np.float32)
        rows, ld = grad.shape
        gb, mb = self.buf(grad), self.buf(np.ascontiguousarray(mask, np.uint8))
        _ck(self.lib, self.lib.gcnhip_relu_bwd_2d(self.ctx, gb.ptr, ld, rows, int(cols), mb.ptr), "gcnhip_relu_bwd_2d")
        return gb.download()

    def dropout_fwd_2d(self, x, cols, p, seed=0, epoch=0, elem_offset=0, keep_in=None, want_mask=True):
        """gcnhip_dropout_fwd_2d -> (buffer [rows, ld], mask int32 [rows . cols] or None)"""
        x = np.ascontiguousarray(x, np.float32)
        rows, ld = x.shape
        xb = self.buf(x)
        mb = self.buf(np.full(max(rows * cols, 1), -1, np.int32)) if want_mask else None
        ep = self.buf(np.array([epoch], np.uint32))
        kb = self.buf(np.ascontiguousarray(keep_in, np.uint8)) if keep_in is not None else None
        _ck(self.lib, self.lib.gcnhip_dropout_fwd_2d(self.ctx, xb.ptr, ld, rows, int(cols), mb.ptr if mb else None, p, seed, ep.ptr, elem_offset,
                                                      kb.ptr if kb else None), "gcnhip_dropout_fwd_2d")
        return xb.download(), (mb.download()[:rows * cols] if mb else None)

    def dropout_bwd_2d(self, grad, cols, mask, p):
        grad = np.ascontiguousarray(grad, np.float32)
        rows, ld = grad.shape
        gb, mb = self.buf(grad), self.buf(np.ascontiguousarray(mask, np.int32))
        _ck(self.lib, self.lib.gcnhip_dropout_bwd_2d(self.ctx, gb.ptr, ld, rows, int(cols), mb.ptr, p), "gcnhip_dropout_bwd_2d")
        return gb.download()

    def xent_fwd(self, logits, truth, training=True, count=0, shift_in_place=True, ld=None):
        """returns dict(loss_sum, count, correct, total, logits, grad)"""
        logits = np.asarray(logits, np.float32)
        n, c = logits.shape
        ld = ld or c
        lb = self.padded(logits, ld)
        gb = self.buf(np.full((n, ld), np.nan, np.float32))
        tb = self.buf(np.ascontiguousarray(truth, np.int32))
        res = self.buf(np.zeros(4, np.float32))
        resi = self.buf(np.zeros(2, np.int32))
        _ck(self.lib, self.lib.gcnhip_xent_fwd(self.ctx, lb.ptr, ld, gb.ptr, ld, tb.ptr, n, c, int(training), int(count),
                                                int(shift_in_place), res.ptr, resi.ptr), "gcnhip_xent_fwd")
        r, ri = res.download(), resi.download()
        return dict(loss_sum=float(r[0]), count=float(r[1]), correct=int(ri[0]), total=int(ri[1]),
                    logits=lb.download()[:, :c], grad=gb.download()[:, :c] if training else None)

    def xent_fwd_rows(self, logits, truth, training=True, shift_in_place=False, ld=None, grad_fill=0.0):
        """gcnhip_xent_fwd_rows over the list of labelled rows; grad rows outside the list keep grad_fill"""
        logits = np.asarray(logits, np.float32)
        truth = np.ascontiguousarray(truth, np.int32)
        n, c = logits.shape
        ld = ld or c
        rows = np.flatnonzero(truth >= 0).astype(np.int32)
        lb = self.padded(logits, ld)
        gb = self.buf(np.full((n, ld), grad_fill, np.float32))
        tb, rb = self.buf(truth), self.buf(rows if rows.size else np.zeros(1, np.int32))
        res, resi = self.buf(np.zeros(4, np.float32)), self.buf(np.zeros(2, np.int32))
        _ck(self.lib, self.lib.gcnhip_xent_fwd_rows(self.ctx, lb.ptr, ld, gb.ptr, ld, tb.ptr, rb.ptr, int(rows.size), c, int(training),
                                                     max(int(rows.size), 1), int(shift_in_place), res.ptr, resi.ptr), "gcnhip_xent_fwd_rows")
        r, ri = res.download(), resi.download()
        return dict(loss_sum=float(r[0]), count=float(r[1]), correct=int(ri[0]), total=int(ri[1]),
                    logits=lb.download()[:, :c], grad=gb.download()[:, :c] if training else None)

    def xent_call(self, entry, table, truth, c, grad=None, rows=None, training=True, count=0, shift_in_place=False, grad_row_scale=None,
                  weight=None, weight_sum=0.0, offset=0, grad_offset=0, result_fill=0x5A5A5A5A):
        """One call of a softmax loss entry point on tables exactly as the caller laid them out.  entry: "fwd" (gcnhip_xent_fwd),
        "rows" (gcnhip_xent_fwd_rows), "scaled" (gcnhip_xent_fwd_rows_scaled), "weighted" (gcnhip_wxent_fwd_rows), "accuracy"
        (gcnhip_accuracy).  table f32 [n, ld] and grad f32 [n, ld_grad] are WHOLE tables, padding columns included (their strides
        are the leading dimensions); offset / grad_offset: the table starts that many floats into its allocation.  rows: the
        list for the list forms.  Nothing is raised: returns dict(rc, result f32 [4], result_i int32 [2] — `result_fill` bits
        where the call wrote nothing —, table, grad: the whole tables after the call)."""
        table = np.ascontiguousarray(table, np.float32)
        n, ld = table.shape
        truth = np.ascontiguousarray(truth, np.int32)

        def place(arr, off):
            flat = np.full(arr.size + off + 4, np.nan, np.float32)
            flat[off:off + arr.size] = arr.ravel()
            b = self.buf(flat)
            return b, C.c_void_p(b.ptr + 4 * off)
        lb, lp = place(table, offset)
        gb, gp, ld_grad = None, None, 0
        if grad is not None:
            grad = np.ascontiguousarray(grad, np.float32)
            ld_grad = grad.shape[1]
            gb, gp = place(grad, grad_offset)
        tb = self.buf(truth if truth.size else np.zeros(1, np.int32))
        rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
        rb = self.buf(rows if rows.size else np.zeros(1, np.int32)) if rows is not None else None
        sb = self.buf(np.ascontiguousarray(grad_row_scale, np.float32)) if grad_row_scale is not None else None
        wb = self.buf(np.ascontiguousarray(weight, np.float32)) if weight is not None else None
        res, resi = self.buf(np.full(4, result_fill, np.uint32).view(np.float32)), self.buf(np.full(2, result_fill, np.uint32).view(np.int32))
        lib, listed = self.lib, int(rows.size) if rows is not None else 0
        head = (self.ctx, lp, ld, gp, ld_grad, tb.ptr)
        tail = (int(c), int(training), int(count), int(shift_in_place), res.ptr, resi.ptr)
        if entry == "fwd":
            rc = lib.gcnhip_xent_fwd(*head, n, *tail)
        elif entry == "rows":
            rc = lib.gcnhip_xent_fwd_rows(*head, rb.ptr, listed, *tail)
        elif entry == "scaled":
            rc = lib.gcnhip_xent_fwd_rows_scaled(*head, rb.ptr, listed, *tail, sb.ptr if sb else None)
        elif entry == "weighted":
            rc = lib.gcnhip_wxent_fwd_rows(*head, rb.ptr, listed, *tail, sb.ptr if sb else None, wb.ptr, float(weight_sum))
        elif entry == "accuracy":
            rc = lib.gcnhip_accuracy(self.ctx, lp, ld, tb.ptr, n, int(c), resi.ptr)
        else:
            raise ValueError(entry)
        self.sync()
        return dict(rc=rc, result=res.download(), result_i=resi.download(),
                    table=lb.download()[offset:offset + table.size].reshape(n, ld),
                    grad=gb.download()[grad_offset:grad_offset + grad.size].reshape(n, ld_grad) if gb else None)

    def bce_fwd_rows(self, logits, truth, rows=None, training=True, count=None, grad_row_scale=None, ld=None, grad_fill=np.nan, words=None):
        """gcnhip_bce_fwd_rows: per-class sigmoid cross-entropy over the listed rows (None: every row).  truth: bool [n, C] (packed
        here into multi-hot words).  Returns dict(loss_sum, denom (rows * C), f1_num (2 TP), f1_den (2 TP + FP + FN), tp, fp, fn,
        rows, loss, f1, grad [n, C] or None); grad rows outside the list keep grad_fill.  words: the multi-hot words themselves,
        uint32 [n, words_per_row], in place of the ones packed from truth (more words than C needs, bits past C set)."""
        logits = np.asarray(logits, np.float32)
        n, c = logits.shape
        ld = ld or c
        rows = np.arange(n, dtype=np.int32) if rows is None else np.ascontiguousarray(rows, np.int32)
        words = pack_multihot(truth) if words is None else np.ascontiguousarray(words, np.uint32)
        lb = self.padded(logits, ld)
        gb = self.buf(np.full((n, ld), grad_fill, np.float32))
        tb, rb = self.buf(words), self.buf(rows if rows.size else np.zeros(1, np.int32))
        sb = self.buf(np.ascontiguousarray(grad_row_scale, np.float32)) if grad_row_scale is not None else None
        res, resi = self.buf(np.zeros(4, np.float32)), self.buf(np.zeros(4, np.int32))
        _ck(self.lib, self.lib.gcnhip_bce_fwd_rows(self.ctx, lb.ptr, ld, gb.ptr, ld, tb.ptr, words.shape[1], rb.ptr, int(rows.size), c,
                                                    int(training), int(count if count is not None else max(rows.size, 1)),
                                                    sb.ptr if sb else None, res.ptr, resi.ptr), "gcnhip_bce_fwd_rows")
        r, ri = res.download(), resi.download()
        return dict(loss_sum=float(r[0]), denom=float(r[1]), f1_num=float(r[2]), f1_den=float(r[3]),
                    tp=int(ri[0]), fp=int(ri[1]), fn=int(ri[2]), rows=int(ri[3]),
                    loss=float(r[0]) / float(r[1]) if r[1] else 0.0, f1=float(r[2]) / float(r[3]) if r[3] else 0.0,
                    grad=gb.download()[:, :c] if training else None)

    def wxent_fwd_rows(self, logits, truth, weight, rows=None, weight_sum=None, training=True, count=None, grad_row_scale=None,
                       shift_in_place=False, ld=None, grad_fill=np.nan):
        """gcnhip_wxent_fwd_rows: class-weighted softmax cross-entropy over the listed rows (None: the rows with truth >= 0).
        weight: f32 [C]; weight_sum: the gradient's divisor (None: sum of weight[truth] over the listed rows, in float64).
        Returns dict(loss_sum, weight_sum (of this call's rows), correct, total, loss, result (f32 [4]), result_i (int32 [2]),
        logits, grad [n, C] or None); grad rows outside the list keep grad_fill."""
        logits = np.asarray(logits, np.float32)
        truth = np.ascontiguousarray(truth, np.int32)
        weight = np.ascontiguousarray(weight, np.float32)
        n, c = logits.shape
        ld = ld or c
        rows = np.flatnonzero(truth >= 0).astype(np.int32) if rows is None else np.ascontiguousarray(rows, np.int32)
        if weight_sum is None:
            t = truth[rows]
            weight_sum = float(weight.astype(np.float64)[t[(t >= 0) & (t < c)]].sum())
        lb = self.padded(logits, ld)
        gb = self.buf(np.full((n, ld), grad_fill, np.float32))
        tb, rb, wb = self.buf(truth), self.buf(rows if rows.size else np.zeros(1, np.int32)), self.buf(weight)
        sb = self.buf(np.ascontiguousarray(grad_row_scale, np.float32)) if grad_row_scale is not None else None
        res, resi = self.buf(np.zeros(4, np.float32)), self.buf(np.zeros(2, np.int32))
        _ck(self.lib, self.lib.gcnhip_wxent_fwd_rows(self.ctx, lb.ptr, ld, gb.ptr, ld, tb.ptr, rb.ptr, int(rows.size), c, int(training),
                                                      int(count if count is not None else max(rows.size, 1)), int(shift_in_place),
                                                      res.ptr, resi.ptr, sb.ptr if sb else None, wb.ptr, float(weight_sum)),
            "gcnhip_wxent_fwd_rows")
        r, ri = res.download(), resi.download()
        return dict(loss_sum=float(r[0]), weight_sum=float(r[1]), correct=int(ri[0]), total=int(ri[1]),
                    loss=float(r[0]) / float(r[1]) if r[1] else 0.0, result=r, result_i=ri,
                    logits=lb.download()[:, :c], grad=gb.download()[:, :c] if training else None)

    def wbce_fwd_rows(self, logits, truth, pos_weight, rows=None, training=True, count=None, grad_row_scale=None, ld=None,
                      grad_fill=np.nan):
        """gcnhip_wbce_fwd_rows: bce_fwd_rows with a weight per class on the positive term (pos_weight: f32 [C]); the same dict"""
        logits = np.asarray(logits, np.float32)
        n, c = logits.shape
        ld = ld or c
        rows = np.arange(n, dtype=np.int32) if rows is None else np.ascontiguousarray(rows, np.int32)
        words = pack_multihot(truth)
        lb = self.padded(logits, ld)
        gb = self.buf(np.full((n, ld), grad_fill, np.float32))
        tb, rb = self.buf(words), self.buf(rows if rows.size else np.zeros(1, np.int32))
        wb = self.buf(np.ascontiguousarray(pos_weight, np.float32))
        sb = self.buf(np.ascontiguousarray(grad_row_scale, np.float32)) if grad_row_scale is not None else None
        res, resi = self.buf(np.zeros(4, np.float32)), self.buf(np.zeros(4, np.int32))
        _ck(self.lib, self.lib.gcnhip_wbce_fwd_rows(self.ctx, lb.ptr, ld, gb.ptr, ld, tb.ptr, words.shape[1], rb.ptr, int(rows.size), c,
                                                     int(training), int(count if count is not None else max(rows.size, 1)),
                                                     sb.ptr if sb else None, res.ptr, resi.ptr, wb.ptr), "gcnhip_wbce_fwd_rows")
        r, ri = res.download(), resi.download()
        return dict(loss_sum=float(r[0]), denom=float(r[1]), f1_num=float(r[2]), f1_den=float(r[3]),
                    tp=int(ri[0]), fp=int(ri[1]), fn=int(ri[2]), rows=int(ri[3]),
                    loss=float(r[0]) / float(r[1]) if r[1] else 0.0, f1=float(r[2]) / float(r[3]) if r[3] else 0.0,
                    grad=gb.download()[:, :c] if training else None)

    def bce_predict_rows(self, logits, rows=None, prob=True, ld=None):
        """gcnhip_bce_predict_rows: (bool [len(rows), C] = logit > 0, sigmoid [len(rows), C] or None)"""
        logits = np.asarray(logits, np.float32)
        n, c = logits.shape
        ld = ld or c
        rows = np.arange(n, dtype=np.int32) if rows is None else np.ascontiguousarray(rows, np.int32)
        m, wpr = rows.size, (c + 31) // 32
        lb = self.padded(logits, ld)
        rb = self.buf(rows if m else np.zeros(1, np.int32))
        bb = self.buf(np.full((max(m, 1), wpr), 0xFFFFFFFF, np.uint32))
        qb = self.buf(np.full((max(m, 1), c), np.nan, np.float32)) if prob else None
        _ck(self.lib, self.lib.gcnhip_bce_predict_rows(self.ctx, lb.ptr, ld, rb.ptr, m, c, bb.ptr, wpr, qb.ptr if qb else None, c),
            "gcnhip_bce_predict_rows")
        return unpack_multihot(bb.download()[:m], c), (qb.download()[:m] if qb else None)

    def bce_predict_rows_thr(self, logits, thr, rows=None, prob=True, ld=None):
        """gcnhip_bce_predict_rows_thr: (bool [len(rows), C] = logit >= thr[c] by the integer keys, sigmoid [len(rows), C] or None)"""
        logits = np.asarray(logits, np.float32)
        n, c = logits.shape
        ld = ld or c
        rows = np.arange(n, dtype=np.int32) if rows is None else np.ascontiguousarray(rows, np.int32)
        m, wpr = rows.size, (c + 31) // 32
        lb = self.padded(logits, ld)
        rb = self.buf(rows if m else np.zeros(1, np.int32))
        tb = self.buf(np.ascontiguousarray(thr, np.float32))
        bb = self.buf(np.full((max(m, 1), wpr), 0xFFFFFFFF, np.uint32))
        qb = self.buf(np.full((max(m, 1), c), np.nan, np.float32)) if prob else None
        rc = self.lib.gcnhip_bce_predict_rows_thr(self.ctx, lb.ptr, ld, rb.ptr, m, c, tb.ptr, bb.ptr, wpr, qb.ptr if qb else None, c)
        if rc != 0:
            raise GcnHipError(f"gcnhip_bce_predict_rows_thr: error {rc}: {self.lib.gcnhip_last_error().decode()}")
        return unpack_multihot(bb.download()[:m], c), (qb.download()[:m] if qb else None)

    def confusion_rows(self, pred, truth, c, rows=None):
        """gcnhip_confusion_rows: (int32 [C, C] with [t, p] = listed rows of truth t predicted as p, listed rows in no cell).  pred,
        truth: int32 [n_table]; rows: the listed rows (repeats allowed), None: every row.  The output buffers are uploaded as
        garbage: the launch zeroes them."""
        pred, truth = np.ascontiguousarray(pred, np.int32), np.ascontiguousarray(truth, np.int32)
        assert pred.shape == truth.shape and pred.ndim == 1
        rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
        n = pred.size if rows is None else rows.size
        pb, tb = self.buf(pred if pred.size else np.zeros(1, np.int32)), self.buf(truth if truth.size else np.zeros(1, np.int32))
        rb = self.buf(rows if rows.size else np.zeros(1, np.int32)) if rows is not None else None
        cb = self.buf(np.full(max(c * c, 1), 0x5A5A5A5A, np.int32))
        ob = self.buf(np.full(1, 0x5A5A5A5A, np.int32))
        _ck(self.lib, self.lib.gcnhip_confusion_rows(self.ctx, pb.ptr, tb.ptr, int(pred.size), rb.ptr if rb else None, int(n), int(c),
                                                      cb.ptr, ob.ptr), "gcnhip_confusion_rows")
        return cb.download()[:c * c].reshape(c, c), int(ob.download()[0])

    def bce_class_counts_rows(self, logits, truth, rows=None, ld=None):
        """gcnhip_bce_class_counts_rows: int32 [3, C] = TP, FP, FN per class over the listed rows (None: every row) of a logit
        table; truth: bool [n, C] (packed here into multi-hot words); class c is predicted when its logit is above 0."""
        logits = np.asarray(logits, np.float32)
        n, c = logits.shape
        ld = ld or c
        rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
        m = n if rows is None else rows.size
        words = pack_multihot(truth)
        lb, tb = self.padded(logits, ld), self.buf(words)
        rb = self.buf(rows if rows.size else np.zeros(1, np.int32)) if rows is not None else None
        cb = self.buf(np.full(3 * c, 0x5A5A5A5A, np.int32))
        _ck(self.lib, self.lib.gcnhip_bce_class_counts_rows(self.ctx, lb.ptr, ld, tb.ptr, words.shape[1], rb.ptr if rb else None, int(m), c,
                                                             cb.ptr), "gcnhip_bce_class_counts_rows")
        return cb.download().reshape(3, c)

    def bce_class_counts_rows_thr(self, logits, truth, thr, rows=None, ld=None):
        """gcnhip_bce_class_counts_rows_thr: int32 [3, C] = TP, FP, FN per class over the listed rows (None: every row) of a logit
        table; truth: bool [n, C] (packed here into multi-hot words); class c is predicted when its logit is >= thr[c] by the
        integer keys."""
        logits = np.asarray(logits, np.float32)
        n, c = logits.shape
        ld = ld or c
        rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
        m = n if rows is None else rows.size
        words = pack_multihot(truth)
        lb, tb = self.padded(logits, ld), self.buf(words)
        rb = self.buf(rows if rows.size else np.zeros(1, np.int32)) if rows is not None else None
        hb = self.buf(np.ascontiguousarray(thr, np.float32))
        cb = self.buf(np.full(3 * c, 0x5A5A5A5A, np.int32))
        rc = self.lib.gcnhip_bce_class_counts_rows_thr(self.ctx, lb.ptr, ld, tb.ptr, words.shape[1], rb.ptr if rb else None, int(m), c, hb.ptr, cb.ptr)
        if rc != 0:
            raise GcnHipError(f"gcnhip_bce_class_counts_rows_thr: error {rc}: {self.lib.gcnhip_last_error().decode()}")
        return cb.download().reshape(3, c)

    def accuracy(self, logits, truth, ld=None):
        logits = np.asarray(logits, np.float32)
        n, c = logits.shape
        ld = ld or c
        lb = self.padded(logits, ld)
        tb = self.buf(np.ascontiguousarray(truth, np.int32))
        resi = self.buf(np.zeros(2, np.int32))
        _ck(self.lib, self.lib.gcnhip_accuracy(self.ctx, lb.ptr, ld, tb.ptr, n, c, resi.ptr), "gcnhip_accuracy")
        ri = resi.download()
        return int(ri[0]), int(ri[1])

    def set_truth(self, split, label, s):
        sb, lb = self.buf(np.ascontiguousarray(split, np.int32)), self.buf(np.ascontiguousarray(label, np.int32))
        tb = self.buf(np.zeros(sb.shape[0], np.int32))
        _ck(self.lib, self.lib.gcnhip_set_truth(self.ctx, tb.ptr, sb.ptr, lb.ptr, sb.shape[0], s), "gcnhip_set_truth")
        return tb.download()

    def sumsq(self, x):
        xb = self.buf(np.ascontiguousarray(x, np.float32).reshape(-1))
        ob = self.buf(np.zeros(1, np.float32))
        _ck(self.lib, self.lib.gcnhip_sumsq(self.ctx, xb.ptr, xb.shape[0], ob.ptr), "gcnhip_sumsq")
        return float(ob.download()[0])

    def adam_steps(self, ws, grads_per_step, decays, lr, weight_decay, beta1=0.9, beta2=0.999, eps=1e-8, epoch_words=None):
        """ws: list of arrays; grads_per_step: list (steps) of lists (vars). Returns (ws, sumsq of ws[0]).
        epoch_words: a device buffer of two uint32 [counter, done] -> gcnhip_adam_step_advance moves them with every step"""
        bufs = []
        for w in ws:
            w = np.ascontiguousarray(w, np.float32).reshape(-1)
            bufs.append(dict(w=self.buf(w), g=self.buf(np.zeros_like(w)), m=self.buf(np.zeros_like(w)), v=self.buf(np.zeros_like(w)), n=w.size))
        arr = (_lib.AdamVar * len(ws))()
        for k, b in enumerate(bufs):
            arr[k] = _lib.AdamVar(b["w"].ptr, b["g"].ptr, b["m"].ptr, b["v"].ptr, b["n"], int(decays[k]))
        sq = self.buf(np.zeros(1, np.float32))
        b1, b2 = np.float32(beta1), np.float32(beta2)
        for t, grads in enumerate(grads_per_step, start=1):
            for k, g in enumerate(grads):
                bufs[k]["g"].upload(np.ascontiguousarray(g, np.float32).reshape(-1))
            # optim.cpp:26 in float arithmetic
            step = np.float32(lr) * np.sqrt(np.float32(1) - np.power(b2, np.float32(t), dtype=np.float32)) / (np.float32(1) - np.power(b1, np.float32(t), dtype=np.float32))
            if epoch_words is not None:
                _ck(self.lib, self.lib.gcnhip_adam_step_advance(self.ctx, arr, len(ws), float(step), None, None, beta1, beta2, eps, weight_decay, sq.ptr,
                                                                epoch_words.ptr, epoch_words.ptr + 4), "gcnhip_adam_step_advance")
            else:
                _ck(self.lib, self.lib.gcnhip_adam_step(self.ctx, arr, len(ws), float(step), None, None, beta1, beta2, eps, weight_decay, sq.ptr), "gcnhip_adam_step")
        return [b["w"].download() for b in bufs], float(sq.download()[0])

    def adam_step_state(self, ws=None, gs=None, ms=None, vs=None, decays=None, step_size=0.0, weight_decay=0.0, beta1=0.9, beta2=0.999,
                        eps=1e-8, step_table=None, epoch_words=None, advance=False, want_sumsq=True, state=None):
        """ONE launch of gcnhip_adam_step (advance=False) or gcnhip_adam_step_advance (advance=True) from GIVEN state: ws, gs, ms,
        vs are lists of arrays, one per variable, uploaded as they are.  step_table: a device Buf of f32 step sizes (then
        epoch_words is required: the launch reads step_table[*d_epoch], d_epoch = the first word of epoch_words, and the scalar
        step_size is ignored); epoch_words: a device Buf of two uint32 [counter, done] — with advance=True the launch moves
        them, and d_epoch is that same counter word, as HipAdam::step passes it.  want_sumsq=False passes d_sumsq = NULL.
        Returns dict(w, m, v: lists of arrays, sumsq: f32 value or None, state).  Passing the returned `state` back in keeps the
        device buffers (w, m, v carry on; ws / ms / vs are then ignored, gs — if given — is uploaded as the new gradients)."""
        if state is None:
            bufs = []
            for w, g, m, v in zip(ws, gs, ms, vs):
                w, g, m, v = (np.ascontiguousarray(t, np.float32).reshape(-1) for t in (w, g, m, v))
                assert w.size == g.size == m.size == v.size
                bufs.append(dict(w=self.buf(w), g=self.buf(g), m=self.buf(m), v=self.buf(v), n=w.size))
            arr = (_lib.AdamVar * len(bufs))()
            for k, b in enumerate(bufs):
                arr[k] = _lib.AdamVar(b["w"].ptr, b["g"].ptr, b["m"].ptr, b["v"].ptr, b["n"], int(decays[k]))
            state = dict(bufs=bufs, arr=arr, sq=self.buf(np.full(1, np.nan, np.float32)))
        elif gs is not None:
            for b, g in zip(state["bufs"], gs):
                b["g"].upload(np.ascontiguousarray(g, np.float32).reshape(-1))
        bufs, arr, sq = state["bufs"], state["arr"], state["sq"]
        if (step_table is not None or advance) and epoch_words is None:
            raise ValueError("adam_step_state: step_table and advance need epoch_words")
        tab = step_table.ptr if step_table is not None else None
        d_epoch = epoch_words.ptr if step_table is not None else None
        d_sq = sq.ptr if want_sumsq else None
        if advance:
            _ck(self.lib, self.lib.gcnhip_adam_step_advance(self.ctx, arr, len(bufs), float(step_size), tab, d_epoch, beta1, beta2, eps, weight_decay,
                                                            d_sq, epoch_words.ptr, epoch_words.ptr + 4), "gcnhip_adam_step_advance")
        else:
            _ck(self.lib, self.lib.gcnhip_adam_step(self.ctx, arr, len(bufs), float(step_size), tab, d_epoch, beta1, beta2, eps, weight_decay, d_sq),
                "gcnhip_adam_step")
        return dict(w=[b["w"].download() for b in bufs], m=[b["m"].download() for b in bufs], v=[b["v"].download() for b in bufs],
                    sumsq=sq.download()[0] if want_sumsq else None, state=state)


RANK_SENTINEL = 0xFFFFFFFF          # the padding of the key tables of csrc/ranking.hip: no score's key
RANK_STATS_BLOCKS = 32              # GCNHIP_RANK_STATS_BLOCKS of include/gcnhip_driver.h
THRESHOLD_SCAN_BLOCKS = 32          # GCNHIP_THRESHOLD_SCAN_BLOCKS of include/gcnhip_driver.h


def __getattr__(name):
    if name == "SORT_TILE":         # the keys a workgroup of gcnhip_sort_segments_u32 sorts at a time, asked of the library
        return int(_lib.gcnhip().gcnhip_sort_tile())
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def rank_key_host(x):
    """The order-preserving uint32 image of float32 scores, as gcnhip_rank_keys forms it: -0.0 is +0.0; with b the bits, ~b when
    the sign bit is set, else b | 0x80000000.  Non-NaN scores compare as their keys; a NaN gets RANK_SENTINEL here (the kernel
    gives it no key)."""
    x = np.ascontiguousarray(x, np.float32)
    b = x.view(np.uint32).copy()
    b[b == 0x80000000] = 0
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(x)] = RANK_SENTINEL
    return k


def pack_multihot(y):
    """bool [n, C] -> uint32 [n, ceil(C / 32)]: bit (c & 31) of word c >> 5 = y[:, c] (the layout of gcnhip_bce_fwd_rows)"""
    y = np.asarray(y).astype(bool)
    n, c = y.shape
    wpr = (c + 31) // 32
    pad = np.zeros((n, wpr * 32), bool)
    pad[:, :c] = y
    b = np.packbits(pad.reshape(n, wpr, 4, 8)[..., ::-1], axis=-1).reshape(n, wpr, 4)   # byte k of a word = bits 8k .. 8k+7
    return np.ascontiguousarray(b.astype(np.uint32) @ (1 << (8 * np.arange(4, dtype=np.uint32)))).astype(np.uint32)


def unpack_multihot(words, c):
    """uint32 [n, ceil(C / 32)] -> bool [n, C]"""
    w = np.ascontiguousarray(words, np.uint32)
    bits = (w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    return bits.reshape(w.shape[0], w.shape[1] * 32)[:, :c].astype(bool)      # (-1 cannot be inferred for zero rows)


class Graph:
    def __init__(self, dev: Device, indptr, indices, n_cols=None, col_deg=None, row_group=None):
        self.dev = dev
        indptr = np.ascontiguousarray(indptr, np.int32)
        indices = np.ascontiguousarray(indices, np.int32)
        self.n_rows = indptr.size - 1
        self.n_cols = int(n_cols) if n_cols is not None else self.n_rows
        cd = np.ascontiguousarray(col_deg, np.int32) if col_deg is not None else None
        rg = np.ascontiguousarray(row_group, np.int32) if row_group is not None else None
        h = C.c_void_p()
        _ck(dev.lib, dev.lib.gcnhip_graph_create_grouped(dev.ctx, C.byref(h), indptr.ctypes.data, indices.ctypes.data, self.n_rows, self.n_cols,
                                                          cd.ctypes.data if cd is not None else None,
                                                          rg.ctypes.data if rg is not None else None), "gcnhip_graph_create_grouped")
        self.h = h

    def set_schedule(self, mode, row_group=None, n_groups=0):
        rg = np.ascontiguousarray(row_group, np.int32) if row_group is not None else None
        _ck(self.dev.lib, self.dev.lib.gcnhip_graph_set_schedule(self.dev.ctx, self.h, mode, rg.ctypes.data if rg is not None else None,
                                                                  n_groups), "gcnhip_graph_set_schedule")

    def remove_rowset(self, h):
        """gcnhip_graph_remove_rowset: unregister a subset made by add_rowset"""
        _ck(self.dev.lib, self.dev.lib.gcnhip_graph_remove_rowset(self.dev.ctx, self.h, h), "gcnhip_graph_remove_rowset")

    def add_rowset(self, wanted):
        """register a subset of the rows (boolean per row); returns the handle gcnhip_graphsum_rowset takes"""
        bits = np.packbits(np.asarray(wanted, bool), bitorder="little")
        bits = np.concatenate([bits, np.zeros((-bits.size) % 4 + 8, np.uint8)]).view(np.uint32)
        h = C.c_void_p()
        _ck(self.dev.lib, self.dev.lib.gcnhip_graph_add_rowset(self.dev.ctx, self.h, bits.ctypes.data, C.byref(h)), "gcnhip_graph_add_rowset")
        return h

    def restricted(self, keep_cols):
        """a second adjacency object without the edges whose source row is outside `keep_cols` (boolean per column)"""
        bits = np.packbits(np.asarray(keep_cols, bool), bitorder="little")
        bits = np.concatenate([bits, np.zeros((-bits.size) % 4 + 8, np.uint8)]).view(np.uint32)
        h = C.c_void_p()
        _ck(self.dev.lib, self.dev.lib.gcnhip_graph_create_restricted(self.dev.ctx, C.byref(h), self.h, bits.ctypes.data), "gcnhip_graph_create_restricted")
        g = Graph.__new__(Graph)
        g.dev, g.n_rows, g.n_cols, g.h = self.dev, self.n_rows, self.n_cols, h
        return g

    def clone(self):
        """a second, independent object with the same edges, coefficients and current row order (gcnhip_graph_clone); row
        subsets are not copied"""
        h = C.c_void_p()
        _ck(self.dev.lib, self.dev.lib.gcnhip_graph_clone(self.dev.ctx, C.byref(h), self.h), "gcnhip_graph_clone")
        g = Graph.__new__(Graph)
        g.dev, g.n_rows, g.n_cols, g.h = self.dev, self.n_rows, self.n_cols, h
        return g

    def reserve(self, dim):
        """segment scratch for aggregations up to `dim` columns (256 are reserved when the object is built)"""
        if dim > 256:
            _ck(self.dev.lib, self.dev.lib.gcnhip_graph_reserve_width(self.dev.ctx, self.h, int(dim)), "gcnhip_graph_reserve_width")

    def scales(self):
        """(dinv_row, dinv2_row, dinv_col, dinv2_col) of gcnhip_graph_scales, as numpy"""
        ps = [C.c_void_p() for _ in range(4)]
        _ck(self.dev.lib, self.dev.lib.gcnhip_graph_scales(self.h, *[C.byref(q) for q in ps]), "gcnhip_graph_scales")
        out = []
        for q, n in zip(ps, (self.n_rows, self.n_rows, self.n_cols, self.n_cols)):
            a = np.empty(n, np.float32)
            _ck(self.dev.lib, self.dev.lib.gcnhip_d2h(self.dev.ctx, a.ctypes.data, q, a.nbytes), "d2h")
            out.append(a)
        return out

    def coef(self):
        pc = C.c_void_p()
        nr, nnz = C.c_int(), C.c_int()
        _ck(self.dev.lib, self.dev.lib.gcnhip_graph_arrays(self.h, None, None, C.byref(pc), C.byref(nr), C.byref(nnz)), "graph_arrays")
        out = np.empty(nnz.value, np.float32)
        _ck(self.dev.lib, self.dev.lib.gcnhip_d2h(self.dev.ctx, out.ctypes.data, pc, out.nbytes), "d2h")
        return out

    def csr(self):
        """(indptr int32 [n_rows + 1], indices int32 [nnz], coef f32 [nnz]) as the device object stores them: every row's
        neighbours in the order the kernels add them, with the f32 coefficients they multiply by"""
        pp, pi, pc = C.c_void_p(), C.c_void_p(), C.c_void_p()
        nr, nnz = C.c_int(), C.c_int()
        _ck(self.dev.lib, self.dev.lib.gcnhip_graph_arrays(self.h, C.byref(pp), C.byref(pi), C.byref(pc), C.byref(nr), C.byref(nnz)), "graph_arrays")
        out = [np.empty(nr.value + 1, np.int32), np.empty(nnz.value, np.int32), np.empty(nnz.value, np.float32)]
        for a, q in zip(out, (pp, pi, pc)):
            if a.nbytes:
                _ck(self.dev.lib, self.dev.lib.gcnhip_d2h(self.dev.ctx, a.ctypes.data, q, a.nbytes), "d2h")
        return tuple(out)

    def free(self):
        if self.h and self.dev.ctx:
            self.dev.lib.gcnhip_graph_destroy(self.dev.ctx, self.h)
        self.h = None


class Feat:
    @classmethod
    def aggregated(cls, dev: Device, g: "Graph", x: "Feat"):
        """the feature object of A^.X (gcnhip_feat_create_aggregated)"""
        self = cls.__new__(cls)
        self.dev = dev
        self.n_rows, self.n_cols = g.n_rows, x.n_cols
        h = C.c_void_p()
        _ck(dev.lib, dev.lib.gcnhip_feat_create_aggregated(dev.ctx, C.byref(h), g.h, x.h), "gcnhip_feat_create_aggregated")
        self.h = h
        self.values_ptr = dev.lib.gcnhip_feat_values(h)
        self.dense = True
        return self

    def values(self):
        out = np.empty((self.n_rows, self.n_cols), np.float32)
        _ck(self.dev.lib, self.dev.lib.gcnhip_d2h(self.dev.ctx, out.ctypes.data, self.values_ptr, out.nbytes), "d2h")
        return out

    def __init__(self, dev: Device, indptr, indices, values, n_cols):
        self.dev = dev
        indptr = np.ascontiguousarray(indptr, np.int32)
        indices = np.ascontiguousarray(indices, np.int32) if indices is not None else None
        values = np.ascontiguousarray(values, np.float32)
        self.n_rows = indptr.size - 1
        self.n_cols = int(n_cols)
        h = C.c_void_p()
        _ck(dev.lib, dev.lib.gcnhip_feat_create(dev.ctx, C.byref(h), indptr.ctypes.data, indices.ctypes.data if indices is not None else None,
                                                 values.ctypes.data, self.n_rows, self.n_cols), "gcnhip_feat_create")
        self.h = h
        self.values_ptr = dev.lib.gcnhip_feat_values(h)
        self.dense = bool(dev.lib.gcnhip_feat_is_dense(h))

    def scale_rows(self, scale):
        """gcnhip_feat_scale_rows: X[r, :] *= scale[r] in every copy the object keeps (values, the padded copy, the CSC copy)"""
        scale = np.ascontiguousarray(scale, np.float32).ravel()
        assert scale.size == self.n_rows
        sb = self.dev.buf(scale if scale.size else np.zeros(1, np.float32))
        _ck(self.dev.lib, self.dev.lib.gcnhip_feat_scale_rows(self.dev.ctx, self.h, sb.ptr), "gcnhip_feat_scale_rows")

    def free(self):
        if self.h and self.dev.ctx:
            self.dev.lib.gcnhip_feat_destroy(self.dev.ctx, self.h)
        self.h = None
