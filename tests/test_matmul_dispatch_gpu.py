"""Every branch of the class-layer product dispatch (csrc/matmul.hip, launch_rowstream / launch_atb / launch_slab_reduce of
dense_kernels.h, the two bf16x3 kernels of class_bf16x3.h) against float64: the rows of tests/matmul_ref.PATHS, each naming
the kernels gate() says it launches (proved on the CPU by test_matmul_dispatch_cpu.py), run through gcnhip_matmul_fwd, _bwd,
_bwd_fused, _bwd_fused_bits, _bwd_ex and _bwd_da_bits with one row stride per operand, operands that start one to three floats
into their allocation, NaN in every padding column of an input, and H1 half zeros with a -0.0 and a denormal in it.

Checks per accepted case: within test_ops_gpu.close_mag, k = 8, of float64 (da against the magnitudes scaled by the same row
factors); da exactly +0.0 wherever the mask is off; every float outside the written columns of every output keeps its fill
bits — padding columns, the floats in front of a shifted table, the rows behind it; the same call twice gives the same bits;
a row factor of all ones gives the bits of no row factor.  A bf16x3 case gives other bits than the same call under
gemm_bf16x3 = 0 and its worst error stays within 2 x the f32 kernels' + eps; a fallback case gives the same bits under
options 0 and 2.  Identities between paths: all row-stream variants of one product, and the three (two) entry points that
ask for the same masked product.  Refusals return -1 and write nothing; m == 0 zeroes db and touches nothing else.

Found by this file: a backward call whose da product is refused (p > 288 with n > 64: W2 does not fit in LDS) had already
launched the weight gradient and written db before it returned -1.  The entry points now ask launch_rowstream's plan
(rowstream_plan, dense_kernels.h; da_product in matmul.hip hands the same arguments to the question and to the launch) before
the first launch; a refused call writes nothing.

Every identity the code promises held on the first run: no pair had to be moved to the float64 bound.

Measured on an MI355X: 628 tests in 3.0 s; the 614 accepted rows of the table take 1.7 s of it, the slowest 0.39 s
(class-fwd-past-the-cap: 98 341 rows, most of it the upload and the float64 product), the next 0.31 s
(class-bwd-past-the-cap), rows-past-the-cap 0.04 s, every other case 0.02 s or less.  Every case is inside its bound as it
stands.  Worst |got - want| / (eps . mag) per path family, over every row, every variant of the identity tests and both
options (8 allowed): class_fwd 4.07, rowstream 3.92, class_bwd da 2.33, atb 2.09, class_bwd db 0.56.
"""
import contextlib
import ctypes as C
import time

import numpy as np
import pytest

from tests import matmul_ref as R
from tests.test_ops_gpu import EPS, close_mag

pytestmark = pytest.mark.gpu

FILL = np.float32(-777.25)
FILL_BITS = int(np.array([FILL]).view(np.uint32)[0])
WORST = {}                                                   # path family -> worst |got - want| / (eps . mag) seen
TIMES = {}                                                   # case -> seconds
K_BOUND = 8.0


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


class World:
    """one device, the operands of the table's shapes (made on first use, kept) and the float64 answers"""

    def __init__(self):
        from cuda_gcn_amd.ops import Device
        self.dev = Device(0)
        self.data, self.refs = {}, {}
        n_cu = C.c_int()
        assert self.dev.lib.gcnhip_ctx_compute_units(self.dev.ctx, C.byref(n_cu)) == 0 and n_cu.value > 0
        self.n_cu = n_cu.value

    def close(self):
        self.dev.close()

    def operands(self, m, n, p):
        key = (m, n, p)
        if key not in self.data:
            rng = np.random.default_rng(m * 1000003 + n * 1009 + p)
            rows = lambda r, c: (rng.standard_normal((r, c)) * np.exp(rng.uniform(-2, 2, (r, 1)))).astype(np.float32)
            a = np.where(rng.random((m, n)) < 0.5, rows(m, n), np.float32(0)).astype(np.float32)       # H1: about half zeros
            if a.size:
                a.flat[0] = np.float32(-0.0)
            if a.size > 1:
                a.flat[a.size // 2] = np.float32(1e-40)      # a positive denormal: a > 0 holds
            self.data[key] = dict(a=a, b=rows(n, p), dc=rows(m, p), rowscale=rng.uniform(0.25, 3.0, m).astype(np.float32),
                                  junk=rng.integers(0, 1 << 32, (m, 8), dtype=np.uint64).astype(np.uint32))
        return self.data[key]

    def bits(self, d, n, wpr):
        """the mask words of a > 0; bits past column n and words past ceil(n / 32) hold noise"""
        bits = d["junk"][:, np.arange(wpr) % 8].copy()
        good = R.pack_bits(R.positive(d["a"]))
        for w in range(good.shape[1]):
            live = np.uint32(0xFFFFFFFF) if (w + 1) * 32 <= n else np.uint32((1 << (n - 32 * w)) - 1)
            bits[:, w] = (good[:, w] & live) | (bits[:, w] & ~live)
        return bits

    def reference(self, row):
        m, n, p = row["m"], row["n"], row["p"]
        rs = row["rowscale"]
        key = (m, n, p, row["entry"] == "fwd", row["mask"], row["scale"] if row["mask"] != "none" else None, rs)
        if key not in self.refs:
            d = self.operands(m, n, p)
            if row["entry"] == "fwd":
                self.refs[key] = R.fwd_ref(d["a"], d["b"])
            else:
                masked = row["mask"] != "none"
                self.refs[key] = R.bwd_ref(d["a"], d["b"], d["dc"], R.positive(d["a"]) if masked else None, row["scale"] if masked else None,
                                           d["rowscale"] if rs else None)
        return self.refs[key]


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()
    print("\nworst |got - want| / (eps . mag) per path family:", {k: round(v, 3) for k, v in sorted(WORST.items())})
    if TIMES:
        slow = max(TIMES, key=TIMES.get)
        print(f"{len(TIMES)} cases in {sum(TIMES.values()):.1f} s, the slowest {TIMES[slow]:.2f} s ({slow})")


@contextlib.contextmanager
def option(dev, value):
    old = dev.get_option("gemm_bf16x3")
    try:
        dev.set_option("gemm_bf16x3", value)
        yield
    finally:
        dev.set_option("gemm_bf16x3", old)


def family(kernel):
    return kernel.split("<")[0].split("/")[0]


def untouched(table, shift, cols, what):
    """every float of the allocation outside columns [0, cols) of the table keeps its fill bits"""
    flat = table.base
    assert flat is not None and flat.ndim == 1
    keep = np.ones(flat.size, bool)
    keep[shift:shift + table.size].reshape(table.shape)[:, :cols] = False
    assert np.all(u32(flat)[keep] == FILL_BITS), f"{what}: a float outside the written columns changed"


def held(got, want, mag, fam, what):
    if not got.size:
        return 0.0
    ratio = float((np.abs(got.astype(np.float64) - want) / (EPS * mag + 1e-30)).max())
    WORST[fam] = max(WORST.get(fam, 0.0), ratio)
    try:
        close_mag(got, want, mag, k=K_BOUND)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e} (worst ratio {ratio:.3f}, allowed {K_BOUND})") from None
    return ratio


def call(w, row, opt=None, rowscale="row"):
    """one call of the row's entry point -> {output name: the whole table}"""
    from cuda_gcn_amd.ops import GcnHipError
    try:
        with option(w.dev, row["opt"] if opt is None else opt):
            return _call(w, row, rowscale)
    except GcnHipError as e:
        if ": error -" in str(e):                            # the library turned the call away: this case fails
            raise
        pytest.exit(f"{row['name']}: {e}", returncode=3)     # a HIP error: nothing more runs on that device


def _call(w, row, rowscale):
    dev, ld, e = w.dev, row["ld"], row["entry"]
    d = w.operands(row["m"], row["n"], row["p"])
    kw = dict(whole=True, fill=FILL, shift=row["shift"])
    if e == "fwd":
        return dict(c=dev.matmul_fwd(d["a"], d["b"], lda=ld["a"], ldb=ld["b"], ldc=ld["c"], **kw))
    bits = w.bits(d, row["n"], ld["wpr"]) if row["mask"] == "bits" else None
    st = dict(ldb=ld["b"], lddc=ld["dc"], ldda=ld["da"])
    if e == "bwd_da_bits":
        return dict(da=dev.matmul_bwd_da_bits(d["b"], d["dc"], bits, row["scale"], **st, **kw))
    st.update(lda=ld["a"], lddb=ld["db"], db=row["db"])
    if e in ("bwd", "bwd_fused"):
        da, db = dev.matmul_bwd(d["a"], d["b"], d["dc"], fused_scale=row["scale"] if e == "bwd_fused" else None, da=row["da"], **st, **kw)
    elif e == "bwd_fused_bits":
        da, db = dev.matmul_bwd_fused_bits(d["a"], d["b"], d["dc"], row["scale"], bits, **st, **kw)
    else:
        rs = row["rowscale"] if isinstance(rowscale, str) else rowscale          # "row": as the table says; else an array or False
        rs = d["rowscale"] if rs is True else rs if rs is not False else None
        da, db = dev.matmul_bwd_ex(d["a"], d["b"], d["dc"], row["scale"], bits, rowscale=rs, **st, **kw)
    return {k: v for k, v in (("da", da), ("db", db)) if v is not None}


def same_bits(x, y):
    return x.keys() == y.keys() and all(np.array_equal(u32(x[k].base), u32(y[k].base)) for k in x)


def check(w, row, out, what):
    """value, exact zeros and untouched memory of one accepted call -> {output: worst |got - want| / mag}"""
    m, n, p, sh = row["m"], row["n"], row["p"], row["shift"]
    kernels = R.kernels_of(row["name"])
    errs = {}
    if row["entry"] == "fwd":
        want, mag = w.reference(row)
        held(out["c"][:, :p], want, mag, family(kernels[0]) if kernels else "", what)
        untouched(out["c"], sh.get("c", 0), p, what + " c")
        errs["c"] = (np.abs(out["c"][:, :p] - want) / (mag + 1e-30)).max() if m else 0.0
        return errs
    (da, mag_da), (db, mag_db) = w.reference(row)
    cls = kernels and kernels[0].startswith("class_bwd")
    if "da" in out:
        got = out["da"][:, :n]
        if m:
            held(got, da, mag_da, "class_bwd.da" if cls else family(kernels[-1]), what + " da")
            errs["da"] = (np.abs(got - da) / (mag_da + 1e-30)).max()
            if row["mask"] != "none":
                off = ~R.positive(w.operands(m, n, p)["a"])
                assert np.all(u32(got)[off] == 0), f"{what}: da is not +0.0 where the mask is off"
        untouched(out["da"], sh.get("da", 0), n if m else 0, what + " da")
    if "db" in out:
        got = out["db"][:, :p]
        if m:
            held(got, db, mag_db, "class_bwd.db" if cls else family(kernels[0]), what + " db")
            errs["db"] = (np.abs(got - db) / (mag_db + 1e-30)).max()
        else:
            assert np.all(u32(got) == 0), f"{what}: db of an empty product is not zero"
        untouched(out["db"], sh.get("db", 0), p, what + " db")
    return errs


ACCEPTED = [k for k, r in R.PATHS.items() if r["name"] != "refused"]
REFUSED = [k for k, r in R.PATHS.items() if r["name"] == "refused"]


@pytest.mark.parametrize("path", ACCEPTED)
def test_every_path(world, path):
    w, row = world, R.PATHS[path]
    t0 = time.perf_counter()
    assert R.gate_of(row) == row["name"]
    if "past-the-cap" in path:                               # the device's own CU count, not the table's
        cap = {"rows": R.rowstream_cap_rows(0, w.n_cu), "class-bwd": R.cls_bwd_cap_rows(w.n_cu), "class-fwd": R.cls_fwd_cap_rows(w.n_cu)}
        assert row["m"] > next(v for k, v in cap.items() if path.startswith(k)), f"{path}: {row['m']} rows are inside the grid cap at {w.n_cu} CUs"
    out = call(w, row)
    errs = check(w, row, out, f"{path} [{row['name']}]")
    assert same_bits(call(w, row), out), f"{path}: two runs differ"
    if row["rowscale"]:
        ones = np.ones(row["m"], np.float32)
        assert same_bits(call(w, row, rowscale=ones), call(w, row, rowscale=False)), f"{path}: a row factor of ones changes the bits"
    if path.startswith("class-"):                            # the class layer: on either side of its gates, every reason to fall back
        if "class_" in R.gate_of(row, option=2) and not row["opt"]:
            pass                                             # what the f32 kernels give here: compared by the rows under options 1 and 2
        elif "class_" in row["name"]:
            f32 = call(w, row, opt=0)
            assert not same_bits(f32, out), f"{path}: same bits as the f32-MFMA kernels: the bf16x3 kernel did not run"
            e32 = check(w, dict(row, opt=0, name=R.gate_of(row, option=0)), f32, f"{path} under gemm_bf16x3 = 0")
            for k in errs:
                assert errs[k] <= 2 * e32[k] + EPS, f"{path} {k}: bf16x3 error {errs[k]:.3e} against f32 {e32[k]:.3e}"
        else:
            for o in (0, 2):
                assert R.gate_of(row, option=o) == row["name"]
                assert same_bits(call(w, row, opt=o), out), f"{path}: other bits under gemm_bf16x3 = {o}: the gate let this case through"
    TIMES[path] = time.perf_counter() - t0


# ------------------------------------------------------------------------------------------------------ identities
def _variants(entry, mask, m, K, Nc, rowscale):
    """rows of one logical product over every form a row-stream launch of it can take"""
    rows = {}
    for vec, epi in ((True, "sw4"), (True, "sw1"), (False, "plain")) + (((False, "staged"),) if Nc >= 64 else ()):
        for i in range(4):
            for wide in ((False, True) if vec else (False,)):
                r = R.rowstream_row(entry, mask, m, K, Nc, vec, epi, i, rowscale=rowscale, wide_a=wide)
                rows[(R.kernels_of(r["name"])[-1], r["ld"].get("a" if entry == "fwd" else "dc"), i)] = r
    return rows


@pytest.mark.parametrize("entry,mask,m,K,Nc", [("fwd", "none", 65, 128, 100), ("fwd", "none", 17, 33, 47), ("fwd", "none", 33, 12, 130),
                                                ("bwd", "none", 33, 41, 130), ("bwd_fused", "H", 17, 64, 65), ("bwd_ex", "H", 33, 17, 129),
                                                ("bwd_ex", "bits", 65, 41, 130), ("bwd_fused_bits", "bits", 16, 128, 64),
                                                ("bwd_da_bits", "bits", 15, 48, 33)])
def test_row_stream_variants_of_one_product_give_the_same_bits(world, entry, mask, m, K, Nc):
    """any stride, any shift, vector or scalar A (K = 128: KCH = 8 or the generic loop), the KCH loads together or one by one,
    16-byte, single, staged or per-lane stores: the same products added in the same k order (dense_kernels.h:49-51)"""
    w = world
    rows = _variants(entry, mask, m, K, Nc, rowscale=True)
    names = {k[0] for k in rows}
    assert len(names) >= 3, names
    out_key, cols = ("c", Nc) if entry == "fwd" else ("da", Nc)
    first = None
    for key, row in rows.items():
        out = call(w, row)
        got = out[out_key][:, :cols]
        check(w, row, out, f"variant {key}")
        if first is None:
            first = (key, got)
        assert np.array_equal(u32(got), u32(first[1])), f"{entry} m={m} K={K} Nc={Nc}: {key} and {first[0]} differ"


@pytest.mark.parametrize("m,n,p,ld", [(33, 130, 41, {}), (17, 47, 16, dict(da=49)), (65, 64, 100, dict(dc=101)), (2049, 128, 41, dict(dc=48, wpr=4))])
def test_entry_points_that_ask_for_the_same_product_agree(world, m, n, p, ld):
    """on the f32 path: gcnhip_matmul_bwd_da_bits = _bwd_fused_bits = _bwd_ex without a row factor (mask words), _bwd_fused = _bwd_ex
    with the mask from a > 0 — which is the mask the words hold, so all five da agree, and so do the four db"""
    w = world
    outs = {}
    for entry, mask in (("bwd_da_bits", None), ("bwd_fused_bits", None), ("bwd_ex", "bits"), ("bwd_ex", "H"), ("bwd_fused", None)):
        row = R._row(entry, m, n, p, "", ld=ld, mask=mask, opt=0)
        row["name"] = R.gate_of(row)
        assert "class" not in row["name"]
        outs[(entry, mask)] = call(w, row)
        check(w, row, outs[(entry, mask)], f"{entry} {mask}")
    ref = outs[("bwd_ex", "bits")]
    for k, o in outs.items():
        assert np.array_equal(u32(o["da"][:, :n]), u32(ref["da"][:, :n])), f"da of {k} differs from gcnhip_matmul_bwd_ex's"
        if "db" in o:
            assert np.array_equal(u32(o["db"][:, :p]), u32(ref["db"][:, :p])), f"db of {k} differs from gcnhip_matmul_bwd_ex's"


# -------------------------------------------------------------------------------------------------------- refusals
def test_refusals_return_minus_one_and_write_nothing(world):
    w = world
    dev, lib = w.dev, w.dev.lib
    src = dev.buf(np.ones(1 << 16, np.float32))              # every input, large enough for every refused shape
    words = dev.buf(np.full(1 << 12, 0xFFFFFFFF, np.uint32))
    fill = np.full(1 << 15, FILL, np.float32)
    da, db = dev.buf(fill), dev.buf(fill)
    for path in REFUSED:
        row = R.PATHS[path]
        assert R.gate_of(row) == "refused", path
        m, n, p, ld, e = row["m"], row["n"], row["p"], row["ld"], row["entry"]
        assert max(m * ld["a"], n * ld["b"], m * ld.get("dc", 0)) <= 1 << 16 and max(m * ld.get("c", 0), m * ld.get("da", 0), n * ld.get("db", 0)) <= 1 << 15
        bt = words.ptr if row["mask"] == "bits" else None
        sc = C.c_float(row["scale"])
        if e == "fwd":
            rc = lib.gcnhip_matmul_fwd(dev.ctx, src.ptr, ld["a"], src.ptr, ld["b"], da.ptr, ld["c"], m, n, p)
        else:
            head = (dev.ctx, src.ptr, ld["a"], src.ptr, ld["b"], src.ptr, ld["dc"], da.ptr, ld["da"], db.ptr if row["db"] else None, ld["db"], m, n, p)
            if e == "bwd":
                rc = lib.gcnhip_matmul_bwd(*head)
            elif e == "bwd_fused":
                rc = lib.gcnhip_matmul_bwd_fused(*head, sc)
            elif e == "bwd_fused_bits":
                rc = lib.gcnhip_matmul_bwd_fused_bits(*head, sc, bt, ld["wpr"])
            elif e == "bwd_ex":
                rc = lib.gcnhip_matmul_bwd_ex(*head, sc, bt, ld["wpr"], None)
            else:
                rc = lib.gcnhip_matmul_bwd_da_bits(dev.ctx, src.ptr, ld["b"], src.ptr, ld["dc"], da.ptr, ld["da"], m, n, p, bt, ld["wpr"], sc)
        dev.sync()
        assert rc == -1, (path, rc)
        for name, b in (("da / c", da), ("db", db)):
            assert np.all(u32(b.download()) == FILL_BITS), f"{path}: {name} written by a refused call"
    # the last K that fits runs, on the same context, after all of that
    row = R.PATHS["lds-K288-bwd"]
    check(w, row, call(w, row), "after the refusals")
