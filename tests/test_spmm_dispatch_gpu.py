"""Every branch of the first-layer product dispatch (spmm_fwd_impl, dense_bwd_part, gcnhip_spmm_bwd: csrc/spmm.hip) against
float64: the rows of tests/spmm_ref.PATHS, each naming the kernel gate() says it reaches (proved on the CPU by
test_spmm_dispatch_cpu.py), run through gcnhip_spmm_fwd, _fwd_relu, _fwd_relu_matmul, _bwd and _bwd_part / _bwd_finish with
row strides above p, operands that start one or two floats into their allocation, a value array of the caller's, every
gemm_bf16x3 x co-run combination, and per row no dropout, an injected keep mask, and Philox decisions at p = 0.5 (offsets 0
and 128 * 5) and p = 0.3 (offset 77: not block-aligned, several bit planes).

Checks per accepted case: within test_ops_gpu.close_mag, k = 8, of float64 (k = 9 at p = 0.3, where a kernel may fold the
scale 1 / 0.7 into W instead of X: one more rounding per term; the fused call: fused_ref's bound); every float outside the
written columns keeps its fill bits — padding columns, the floats in front of a shifted table, the rows behind it; an empty
row of X gives an exact zero row, an empty column an exact zero row of dW; the same call twice gives the same bits; ReLU is
max(., 0) of the plain call's bits; the weight gradient in parts, in any order, is the one-call form bit for bit.

Identities between paths: the persistent form and the tile kernels; the co-running bf16x3 lane and the plain one.
Inequalities (the gate was crossed): bf16x3 / f32 MFMA, sliced / unsliced, narrow / general.  Refusals launch nothing.

Found by this file: spmm_general = -1 ("narrow kernels at any size") never reached the narrow kernels — the predicate read
`!spmm_general && (nnz >= 262144 || spmm_general < 0)`; it now reads `spmm_general <= 0 && ...`.

Measured on an MI355X: 345 cases in 9.7 s, the slowest 0.53 s (sparse-bwd-vec-256-256-nw1; its float64 reference is most of
it).  Every case is inside its bound as it stands.  Worst |got - want| / (eps . mag) per path family, over every row, dropout
kind and the scale_rows cases: fwd_bf16x3 4.59, fwd_persist 3.78, fwd_t128w8 3.68, fwd_t128 3.57, fwd_dense 3.08, fwd_csr
2.52, fwd_csr_q 2.36, fwd_csr_sliced 1.72, bwd_csc 4.04, bwd_bf16x3 2.56, bwd_csc_q 1.09, bwd_t128 1.08, bwd_atb 0.92; the
fused call 0.24 in the same unit of its own bound (8 allowed everywhere, 9 at p = 0.3).
"""
import contextlib

import numpy as np
import pytest

from tests import spmm_ref as R
from tests.test_ops_gpu import EPS, close_mag

pytestmark = pytest.mark.gpu

FILL = np.float32(-777.25)
FILL_BITS = int(np.array([FILL]).view(np.uint32)[0])
WORST = {}                                                   # path family -> worst |got - want| / (eps . mag) seen


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


class World:
    """one device, the feature objects of the table (made on first use, kept) and the float64 answers"""

    def __init__(self):
        from cuda_gcn_amd.ops import Device
        self.dev = Device(0)
        self.data, self.feats, self.refs, self.keeps = {}, {}, {}, {}

    def close(self):
        for f in self.feats.values():
            f.free()
        self.dev.close()

    def layout(self, row):
        key = (row["layout"], row["N"], row["F"])
        if key not in self.data:
            if row["layout"] == "dense":
                fp, fi = R.dense_layout(row["N"], row["F"])
                F = row["F"]
            else:
                F = R.SPARSE_BIG_F if row["layout"] == "sparse_big" else R.SPARSE["F"]
                fp, fi = R.sparse_layout(F=F)
            nnz = int(fp[-1])
            rng = np.random.default_rng(nnz + F)
            mk = lambda: (rng.standard_normal(nnz) * np.exp(rng.uniform(-2, 2, nnz))).astype(np.float32)
            self.data[key] = dict(fp=fp, fi=fi, F=F, n=fp.size - 1, nnz=nnz, vals=mk(), vals2=mk(), mask=rng.integers(0, 2, nnz).astype(np.uint8))
        return key, self.data[key]

    def feat(self, row):
        key, d = self.layout(row)
        key = key + (row["nw"],)
        if key not in self.feats:
            self.dev.set_option("spmm_nw", row["nw"])        # read by gcnhip_feat_create
            try:
                idx = d["fi"] if d["fi"] is not None else np.tile(np.arange(d["F"], dtype=np.int32), d["n"])
                self.feats[key] = self.dev.feat(d["fp"], idx, d["vals"], d["F"])
            finally:
                self.dev.set_option("spmm_nw", 0)
            assert self.feats[key].dense == (row["layout"] == "dense")
        return self.feats[key], d

    def operand(self, row, d):
        """w [F, p] of a forward, dout [n, p] of a weight gradient"""
        shape = (d["F"], row["p"]) if row["op"] == "fwd" else (d["n"], row["p"])
        return np.random.default_rng(shape[0] * 1000 + shape[1]).standard_normal(shape).astype(np.float32)

    def keep(self, row, drop):
        key, d = self.layout(row)
        if (key, drop) not in self.keeps:
            self.keeps[(key, drop)] = R.keep_of(R.DROPS[drop], d["nnz"], d["mask"])
        return self.keeps[(key, drop)]

    def reference(self, row, drop):
        key, d = self.layout(row)
        rk = (key, row["ext"], row["p"], row["op"], drop)
        if rk not in self.refs:
            vals = d["vals2"] if row["ext"] else d["vals"]
            keep = self.keep(row, drop)
            scale = R.drop_scale(R.DROPS[drop]["p"]) if keep is not None else 1
            if row["op"] == "fwd":
                self.refs[rk] = R.fwd_ref(d["fp"], d["fi"], vals, self.operand(row, d), keep, scale)
            else:
                self.refs[rk] = R.bwd_ref(d["fp"], d["fi"], vals, self.operand(row, d), d["F"], keep, scale)
        return self.refs[rk]


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()
    print("\nworst |got - want| / (eps . mag) per path family:", {k: round(v, 3) for k, v in sorted(WORST.items())})


@contextlib.contextmanager
def options(dev, row):
    old = {k: dev.get_option(k) for k in row["opts"]}
    try:
        for k, v in row["opts"].items():
            dev.set_option(k, v)
        dev.lib.gcnhip_ctx_set_corun(dev.ctx, row["corun"])
        yield
    finally:
        dev.lib.gcnhip_ctx_set_corun(dev.ctx, 0)
        for k, v in old.items():
            dev.set_option(k, v)


def family(name):
    return name.split("<")[0]


def untouched(table, shift, p, what):
    """every float of the allocation outside columns [0, p) of the table keeps its fill bits"""
    flat = table.base
    assert flat is not None and flat.ndim == 1
    keep = np.ones(flat.size, bool)
    keep[shift:shift + table.size].reshape(table.shape)[:, :p] = False
    assert np.all(u32(flat)[keep] == FILL_BITS), f"{what}: a float outside the written columns changed"


def held(got, want, mag, k, fam, what):
    ratio = float((np.abs(got.astype(np.float64) - want) / (EPS * mag + 1e-30)).max()) if got.size else 0.0
    WORST[fam] = max(WORST.get(fam, 0.0), ratio)
    try:
        close_mag(got, want, mag, k=k)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e} (worst ratio {ratio:.3f}, allowed {k})") from None


def call(w, row, f, d, drop="none", relu=False, cuts=None, order=None, w2=None):
    """one call of the row's entry point -> the whole table (None: the fused form answered GCNHIP_NOT_AVAILABLE)"""
    from cuda_gcn_amd.ops import GcnHipError
    try:
        return _call(w, row, f, d, drop, relu, cuts, order, w2)
    except GcnHipError as e:
        if ": error -" in str(e):                            # the library turned the call away: this case fails
            raise
        pytest.exit(f"{row['name']} dropout={drop}: {e}", returncode=3)     # a HIP error: nothing more runs on that device


def _call(w, row, f, d, drop, relu, cuts, order, w2):
    dev = w.dev
    kw = dict(vals=d["vals2"] if row["ext"] else None, whole=True, fill=FILL, shift=row["shift"])
    x = w.operand(row, d)
    if row["op"] == "bwd":
        kw.update(R.drop_kwargs(R.DROPS[drop], d["mask"]), ld_dout=row["ld"], ld_dw=row["ldo"])
        if cuts is not None:
            return dev.spmm_bwd_parts(f, x, cuts, order=order, **kw)
        return dev.spmm_bwd(f, x, **kw)
    if w2 is not None:
        ldz = R.cdiv(w2.shape[1], 4) * 4
        return dev.spmm_fwd_relu_matmul(f, x, w2, ld_z=ldz, ld_w=row["ld"], **kw)
    if relu:
        return dev.spmm_fwd_relu(f, x, ld_w=row["ld"], ld_out=row["ldo"], **kw)
    return dev.spmm_fwd(f, x, ld_w=row["ld"], ld_out=row["ldo"], **kw, **R.drop_kwargs(R.DROPS[drop], d["mask"]))


@pytest.mark.parametrize("path", list(R.PATHS))
def test_every_path(world, path):
    w, row = world, R.PATHS[path]
    f, d = w.feat(row)
    p, sh = row["p"], row["shift"].get("out", 0)
    assert R.gate_of(row) == row["name"]
    with options(w.dev, row):
        if row["fused"]:
            w2 = (np.random.default_rng(row["fused"]).standard_normal((128 if p == 128 else p, row["fused"])) * 0.3).astype(np.float32)
            z = call(w, row, f, d, w2=w2)
            if row["name"] == "NOT_AVAILABLE":
                assert z is None, f"{path}: the fused form ran"
                return
            assert z is not None, f"{path}: the fused form answered GCNHIP_NOT_AVAILABLE"
            X = (d["vals2"] if row["ext"] else d["vals"]).reshape(d["n"], d["F"])
            want, bound = R.fused_ref(X, w.operand(row, d), w2)
            got = z[:, :row["fused"]]
            ratio = float((np.abs(got - want) / (bound / 8)).max())
            WORST["fused"] = max(WORST.get("fused", 0.0), ratio)
            assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= bound), f"{path}: worst ratio {ratio:.3f} of 8"
            untouched(z, sh, row["fused"], path)
            assert np.array_equal(u32(call(w, row, f, d, w2=w2).base), u32(z.base)), f"{path}: two runs differ"
            return
        dense = row["layout"] == "dense"
        plan = w.dev.spmm_bwd_plan(f, p) if row["op"] == "bwd" else None
        if plan is not None:
            assert plan == (R.dense_bwd_plan(dense, d["n"], d["F"], p) or (0, 0)), f"{path}: the split-K plan is not the restated one"
        for drop in R.DROPS:
            name = R.gate_of(row, drop)
            what = f"{path} [{name}] dropout={drop}"
            assert family(name) == family(row["name"]) or name.endswith(",fast>") or row["name"].endswith(",fast>"), what
            got = call(w, row, f, d, drop)
            want, mag = w.reference(row, drop)
            k = 8.0 if drop == "none" or float(R.drop_scale(R.DROPS[drop]["p"])) == 2.0 else 9.0
            held(got[:, :p], want, mag, k, family(name), what)
            untouched(got, sh, p, what)
            assert np.array_equal(u32(call(w, row, f, d, drop).base), u32(got.base)), f"{what}: two runs differ"
            if not dense:
                empty = got[5, :p] if row["op"] == "fwd" else got[-3:, :p]
                assert np.all(u32(empty) == 0), f"{what}: an empty {'row' if row['op'] == 'fwd' else 'column'} of X is not an exact zero row"
            if row["op"] == "fwd" and drop == "none":
                r = call(w, row, f, d, relu=True)
                assert np.array_equal(r[:, :p], np.maximum(got[:, :p], 0)) and not np.signbit(r[:, :p]).any(), f"{what}: ReLU is not max(., 0) of the plain call"
                untouched(r, sh, p, what + " relu")
            if plan and plan[1] and drop in ("none", "philox.3@77", "mask"):
                S = plan[1]
                cuts = sorted({0, S // 3, S // 2, S - 1, S})
                order = list(range(len(cuts) - 1))[::-1]
                for o in (None, order):
                    parts = call(w, row, f, d, drop, cuts=cuts, order=o)
                    assert np.array_equal(u32(parts.base), u32(got.base)), f"{what}: the gradient in parts (order {o}) differs from the one-call form"


def _dense_row(F, n=289, **kw):
    return R._row(kw.pop("op", "fwd"), "dense", n, F, 128, "", **kw)


@pytest.mark.parametrize("K", [96, 130, 321, 2721, 4096])
def test_persistent_form_and_tile_kernels_give_the_same_bits(world, K):
    """gemm_bf16x3 = 0: the persistent f32 form (not co-running) and the eight-wave tiles (co-running) add the same products in
    the same order, with and without ReLU, at p_drop 0 and 0.5 (the scale 2 folds exactly into either operand)"""
    w = world
    got = {}
    for co in (0, 1):
        row = _dense_row(K, opts=dict(gemm_bf16x3=0), corun=co)
        assert R.gate_of(row) == ("fwd_t128w8" if co else "fwd_persist")
        f, d = w.feat(row)
        with options(w.dev, row):
            got[co] = [call(w, row, f, d), call(w, row, f, d, relu=True), call(w, row, f, d, "philox.5@0"), call(w, row, f, d, "philox.5@640"),
                       call(w, row, f, d, "mask")]
    for a, b in zip(got[0], got[1]):
        assert np.array_equal(u32(a), u32(b))


@pytest.mark.parametrize("K", [64, 97, 320, 2720])
def test_co_running_bf16x3_lane_equals_the_plain_one(world, K):
    w = world
    got = {}
    for co in (0, 1):
        for op in ("fwd", "bwd"):
            row = _dense_row(K, op=op, opts=dict(gemm_bf16x3=2), corun=co)
            assert R.gate_of(row) == op + "_bf16x3"
            f, d = w.feat(row)
            with options(w.dev, row):
                got[(co, op)] = [call(w, row, f, d, drop) for drop in ("none", "philox.3@77")] + ([call(w, row, f, d, relu=True)] if op == "fwd" else [])
    for op in ("fwd", "bwd"):
        for a, b in zip(got[(0, op)], got[(1, op)]):
            assert np.array_equal(u32(a), u32(b)), op


def test_paths_that_associate_differently_give_other_bits(world):
    """bf16x3 against the f32 MFMA kernels, the sliced sparse forward against the unsliced, the narrow sparse kernels against
    the general ones: equal inside the bound (test_every_path), not bit for bit — the option did move the call to another kernel"""
    w = world
    pairs = [("bx2-corun0-fwd", "bx0-corun0-fwd"), ("bx2-corun0-bwd", "bx0-corun0-bwd"), ("sparse-fwd-sliced", "sparse-fwd-unsliced"),
             ("sparse-fwd-q-16-16", "sparse-fwd-vec-16-16"), ("sparse-fwd-q-41-44", "sparse-fwd-vec-41-44"),
             ("sparse-bwd-q-16-16-nw1", "sparse-bwd-vec-16-16-nw1"), ("sparse-bwd-q-41-44-nw4", "sparse-bwd-vec-41-44-nw4"),
             ("sparse-bwd-q-7-8-nw16", "sparse-bwd-vec-7-8-nw16")]
    for a, b in pairs:
        ra, rb = R.PATHS[a], R.PATHS[b]
        assert ra["name"] != rb["name"] and all(ra[k] == rb[k] for k in ("op", "layout", "N", "F", "p", "ld", "ldo", "ext", "nw"))
        out = []
        for row in (ra, rb):
            f, d = w.feat(row)
            with options(w.dev, row):
                out.append(call(w, row, f, d))
        assert not np.array_equal(u32(out[0]), u32(out[1])), f"{a} and {b} gave the same bits: one kernel served both"


def test_refusals_launch_nothing_and_write_nothing(world):
    w = world
    dev, lib = w.dev, w.dev.lib
    out_fill = np.full(300 * 160, FILL, np.float32)
    out, wide = dev.buf(out_fill), dev.buf(np.ones(5000 * 160, np.float32))
    ep = dev.buf(np.array([R.EPOCH], np.uint32))

    def nothing_written(what):
        dev.sync()
        assert np.all(u32(out.download()) == FILL_BITS), f"{what}: out written"

    # the fused call: sparse X, p != 128, and the window where only the plain call still fits its packed W
    for path in ("fused-refused-sparse", "fused-refused-p16", "fused-refused-p256", f"k{R.K_FUSED + 1}-fused", f"k{R.K_BF16X3}-fused",
                 f"k{R.K_PERSIST}-fused", "bx0-corun0-fused"):
        row = R.PATHS[path]
        f, d = w.feat(row)
        with options(dev, row):
            rc = lib.gcnhip_spmm_fwd_relu_matmul(dev.ctx, f.h, f.values_ptr, wide.ptr, row["ld"], row["p"], wide.ptr, 8, 7, out.ptr, 8)
        assert rc == -2 and b"not available" in lib.gcnhip_error_string(rc), (path, rc)
        nothing_written(path)
    for K in (R.K_FUSED + 1, R.K_BF16X3):                     # ... while the plain call there takes bf16x3
        assert R.PATHS[f"k{K}-fwd"]["name"] == "fwd_bf16x3"
    # dropout on an aggregated feature object (no keep-bit array): every dense branch
    n = 64
    gp = np.arange(n + 1, dtype=np.int32)
    g = dev.graph(gp, np.arange(n, dtype=np.int32))
    for F in (96, 40):
        x = dev.feat((np.arange(n + 1) * F).astype(np.int32), np.tile(np.arange(F, dtype=np.int32), n), np.ones(n * F, np.float32), F)
        from cuda_gcn_amd.ops import Feat
        agg = Feat.aggregated(dev, g, x)
        for p in (128, 16):
            assert R.gate("fwd", True, n, F, n * F, p, p, drop=R.DROPS["philox.5@0"], keep_bits=False) == "refused"
            rc = lib.gcnhip_spmm_fwd(dev.ctx, agg.h, agg.values_ptr, wide.ptr, p, out.ptr, p, p, 0.5, R.SEED, ep.ptr, 0, None)
            assert rc != 0 and b"keep-bit" in lib.gcnhip_last_error(), (F, p, rc)
            nothing_written(f"dropout on an aggregated object, forward F={F} p={p}")
            rc = lib.gcnhip_spmm_bwd(dev.ctx, agg.h, agg.values_ptr, wide.ptr, p, out.ptr, p, p, 0.5, R.SEED, ep.ptr, 0, None)
            assert rc != 0, (F, p, rc)
            nothing_written(f"dropout on an aggregated object, weight gradient F={F} p={p}")
            assert lib.gcnhip_spmm_fwd(dev.ctx, agg.h, agg.values_ptr, wide.ptr, p, out.ptr, p, p, 0.0, 0, ep.ptr, 0, None) == 0   # evaluation passes
            dev.sync()
            out.upload(out_fill)
        agg.free(); x.free()
    g.free()
    # gcnhip_spmm_bwd_part / _finish without a plan: sparse X, p <= 64, fewer than 64 columns
    for path, p in (("sparse-bwd-vec-16-16-nw1", 16), ("sparse-bwd-vec-128-132-nw1", 128), ("bwd-atb-F40", 128), ("ld-41-44-dense-bwd", 41)):
        f, d = w.feat(R.PATHS[path])
        assert dev.spmm_bwd_plan(f, p) == (0, 0)
        assert lib.gcnhip_spmm_bwd_part(dev.ctx, f.h, f.values_ptr, wide.ptr, 132, p, 0.0, 0, ep.ptr, 0, None, 0, 1, 1) != 0, path
        assert lib.gcnhip_spmm_bwd_finish(dev.ctx, f.h, out.ptr, 132, p) != 0, path
        nothing_written(path)
    # a split range outside the plan
    f, d = w.feat(R.PATHS["bx2-corun0-bwd"])
    S = dev.spmm_bwd_plan(f, 128)[1]
    for s0, s1 in ((-1, 1), (0, S + 1), (2, 1)):
        assert lib.gcnhip_spmm_bwd_part(dev.ctx, f.h, f.values_ptr, wide.ptr, 128, 128, 0.0, 0, ep.ptr, 0, None, s0, s1, 1) != 0
    nothing_written("split range outside the plan")
    row = R.PATHS["bx2-corun0-fwd"]                          # the context still works
    f, d = w.feat(row)
    got = call(w, row, f, d)
    held(got[:, :128], *w.reference(row, "none"), 8.0, "fwd_bf16x3", "after the refusals")


@pytest.mark.parametrize("layout,F", [("sparse", 0), ("dense", 96), ("dense", 40), ("dense", 128)])
def test_scale_rows_moves_every_copy_together(world, layout, F):
    """gcnhip_feat_scale_rows: values, the padded copy (dense, F = 96) and the CSC copy (sparse) are scaled alike — the forward
    and the weight gradient from the object's own values, and from a value array of the caller's that holds the scaled
    values, meet float64 on the scaled X, and agree bit for bit where gate() names the same kernel for both"""
    w = world
    base = R._row("fwd", layout, 289 if layout == "dense" else 0, F, 128, "")
    _, d = w.layout(base)
    idx = d["fi"] if d["fi"] is not None else np.tile(np.arange(d["F"], dtype=np.int32), d["n"])
    f = w.dev.feat(d["fp"], idx, d["vals"], d["F"])          # an object of this test's own: it is changed
    try:
        s = np.random.default_rng(7).uniform(0.25, 3.0, d["n"]).astype(np.float32)
        f.scale_rows(s)
        scaled = (d["vals"] * s[R.row_of(d["fp"])]).astype(np.float32)
        for op, p, ld, drop in (("fwd", 128, 128, "none"), ("bwd", 128, 128, "none"), ("fwd", 16, 16, "none"), ("bwd", 16, 16, "none"),
                                ("fwd", 128, 128, "philox.5@0"), ("bwd", 128, 128, "philox.3@77"), ("fwd", 41, 44, "mask"), ("bwd", 41, 44, "mask")):
            x = np.random.default_rng(p).standard_normal((d["F"], p) if op == "fwd" else (d["n"], p)).astype(np.float32)
            keep = R.keep_of(R.DROPS[drop], d["nnz"], d["mask"])
            scale = R.drop_scale(R.DROPS[drop]["p"]) if keep is not None else 1
            want, mag = (R.fwd_ref(d["fp"], d["fi"], scaled, x, keep, scale) if op == "fwd" else R.bwd_ref(d["fp"], d["fi"], scaled, x, d["F"], keep, scale))
            got, names = {}, {}
            for ext in (False, True):
                kw = dict(vals=scaled if ext else None, whole=True, fill=FILL, **R.drop_kwargs(R.DROPS[drop], d["mask"]))
                row = R._row(op, layout, base["N"], F, p, "", ld=ld, ext=ext, drop=drop)
                names[ext] = R.gate_of(row)
                got[ext] = w.dev.spmm_fwd(f, x, ld_w=ld, ld_out=ld, **kw) if op == "fwd" else w.dev.spmm_bwd(f, x, ld_dout=ld, ld_dw=ld, **kw)
                what = f"{layout} F={d['F']} {op} p={p} dropout={drop} {'external' if ext else 'own'} values [{names[ext]}]"
                held(got[ext][:, :p], want, mag, 9.0 if drop == "philox.3@77" else 8.0, family(names[ext]), what)
                untouched(got[ext], 0, p, what)
            if names[False] == names[True]:
                assert np.array_equal(u32(got[False]), u32(got[True])), f"{layout} F={d['F']} {op} p={p} {drop}: own and external values differ on {names[True]}"
    finally:
        f.free()
