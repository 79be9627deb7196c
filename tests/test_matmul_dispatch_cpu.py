"""tests/matmul_ref.py before a GPU sees it: the float64 restatements against the oracle's Matmul and against plain dense
formulas, the mask and factor algebra, and the table of paths against gate()."""
import itertools

import numpy as np
import pytest

from tests import matmul_ref as R
from tests.test_ops_gpu import close_mag


def _operands(m, n, p, seed=0):
    rng = np.random.default_rng(seed + m + 10 * n + 100 * p)
    a = (rng.standard_normal((m, n)) * rng.choice([0.0, 1.0], (m, n))).astype(np.float32)
    a.flat[0], a.flat[-1] = np.float32(-0.0), np.float32(1e-40)
    return a, rng.standard_normal((n, p)).astype(np.float32), rng.standard_normal((m, p)).astype(np.float32)


@pytest.mark.parametrize("m,n,p", [(5, 3, 2), (97, 128, 41), (33, 16, 7), (64, 100, 130)])
def test_restatements_against_the_oracle(oracle, m, n, p):
    a, b, dc = _operands(m, n, p)
    want, mag = R.fwd_ref(a, b)
    close_mag(oracle.matmul_fwd(a, b, m, n, p), want, mag)
    assert np.allclose(mag, oracle.matmul_fwd(np.abs(a), np.abs(b), m, n, p), rtol=1e-5)
    (da, mag_da), (db, mag_db) = R.bwd_ref(a, b, dc)
    oa, ob = oracle.matmul_bwd(a, b, dc, m, n, p)
    ma, mb = oracle.matmul_bwd(np.abs(a), np.abs(b), np.abs(dc), m, n, p)
    close_mag(oa, da, mag_da)
    close_mag(ob, db, mag_db)
    assert np.allclose(mag_da, ma, rtol=1e-5) and np.allclose(mag_db, mb, rtol=1e-5)
    # the fused form, as test_matmul_vs_oracle states it: the oracle's dA under the ReLU mask, times the scale
    (fa, fmag), _ = R.bwd_ref(a, b, dc, R.positive(a), 2.0)
    close_mag(np.where(a > 0, oa * np.float32(2), 0), fa, fmag)
    assert np.allclose(fmag, 2 * ma, rtol=1e-5)


def test_mask_and_factor_algebra_against_a_plain_formula():
    m, n, p = 37, 70, 9
    a, b, dc = _operands(m, n, p, seed=5)
    rs = np.random.default_rng(1).uniform(0.25, 3, m).astype(np.float32)
    pos = R.positive(a)
    assert not pos.flat[0] and pos.flat[-1] and np.array_equal(pos, a > 0)        # -0.0 is off, a positive denormal is on
    for wpr in (3, 4):
        bits = R.pack_bits(pos, wpr)
        assert bits.shape == (m, wpr) and np.array_equal(R.unpack_bits(bits, n), pos)
        assert all(((int(bits[r, c >> 5]) >> (c & 31)) & 1) == int(pos[r, c]) for r in (0, 5, m - 1) for c in (0, 31, 32, 63, 64, n - 1))
        assert np.all(bits[:, 2] >> np.uint32(n - 64) == 0) and np.all(bits[:, 3:] == 0)
    a64, b64, d64 = (t.astype(np.float64) for t in (a, b, dc))
    (da, mag), (db, mag_db) = R.bwd_ref(a, b, dc, pos, 1.5, rs)
    f = (np.float32(1.5) * rs).astype(np.float64)[:, None]                        # the factor is formed in float32
    assert np.array_equal(f, R.row_factor(m, 1.5, rs)) and np.array_equal(R.row_factor(m), np.ones((m, 1)))
    assert np.allclose(da, np.where(a > 0, (d64 @ b64.T) * f, 0), rtol=1e-13, atol=1e-13) and np.all(da[~pos] == 0) and not np.signbit(da[~pos]).any()
    assert np.allclose(mag, (np.abs(d64) @ np.abs(b64).T) * f, rtol=1e-13)
    assert np.allclose(db, a64.T @ d64, rtol=1e-13, atol=1e-13) and np.allclose(mag_db, np.abs(a64).T @ np.abs(d64), rtol=1e-13)
    ones = R.bwd_ref(a, b, dc, pos, 1.5, np.ones(m, np.float32))[0]
    assert np.array_equal(ones[0], R.bwd_ref(a, b, dc, pos, 1.5)[0][0]) and np.array_equal(ones[1], R.bwd_ref(a, b, dc, pos, 1.5)[0][1])
    (na, _), (nb, _) = R.bwd_ref(None, b, dc, pos, 1.5)                           # gcnhip_matmul_bwd_da_bits: no a, no db
    assert nb is None and np.array_equal(na, R.bwd_ref(a, b, dc, pos, 1.5)[0][0])
    # NaN in dc's padding columns never reaches the reference: it takes the p real columns
    assert np.all(np.isfinite(da)) and np.all(np.isfinite(db))


def test_the_table_names_the_path_the_gate_takes():
    for pid, row in R.PATHS.items():
        assert R.gate_of(row) == row["name"], (pid, R.gate_of(row))
        assert set(R.kernels_of(row["name"])) <= R.every_name() | {"refused"}, pid
    named = set().union(*(R.kernels_of(r["name"]) for r in R.PATHS.values())) - {"refused"}
    assert named == R.every_name(), (sorted(R.every_name() - named), sorted(named - R.every_name()))
    assert len(R.rowstream_names()) == 351
    # every (NT, VEC, mask source, KCH) combination of gemm_rowstream_kernel, once per entry point that reaches it
    combos = {}
    for row in R.PATHS.values():
        for k in R.kernels_of(row["name"]):
            if k.startswith("rowstream"):
                combos.setdefault(k.split("/")[0], set()).add(row["entry"])
    assert len(combos) == 165
    for combo, entries in combos.items():
        mask = combo.split(",")[2]
        assert entries >= set(R.MASK_ENTRIES[mask]), (combo, entries)
    # the shapes the table draws them from
    rs = [r for k, r in R.PATHS.items() if k.startswith("rs-")]
    K_of = lambda r: r["n"] if r["entry"] == "fwd" else r["p"]
    Nc_of = lambda r: r["p"] if r["entry"] == "fwd" else r["n"]
    assert {K_of(r) for r in rs} == {1, 12, 16, 17, 33, 48, 64, 65, 100, 128, 130, 288}
    assert {Nc_of(r) for r in rs} == {1, 3, 16, 17, 33, 47, 48, 64, 65, 100, 129, 130}
    assert {r["m"] for r in rs} == {1, 15, 16, 17, 65}
    # what varies beside the kernel's name does meet it: a row factor on and off at every (mask source, epilogue) of
    # gcnhip_matmul_bwd_ex; scalar A by an odd stride and by a shifted table; single-float stores by every way into them
    tail = lambda r: R.kernels_of(r["name"])[-1]
    ex = [r for r in rs if r["entry"] == "bwd_ex"]
    for mask, epi in itertools.product(("H", "bits"), ("sw4", "sw1", "staged", "plain")):
        assert {r["rowscale"] for r in ex if r["mask"] == mask and tail(r).split("/")[1] == epi} == {True, False}, (mask, epi)
    for mask in ("none", "H", "bits"):
        scalar = [r for r in rs if r["mask"] == mask and ",scalar," in tail(r)]
        A = lambda r: "a" if r["entry"] == "fwd" else "dc"
        assert any(r["ld"][A(r)] % 4 for r in scalar) and any(r["shift"].get(A(r), 0) % 2 for r in scalar), mask
        sw1 = [r for r in rs if r["mask"] == mask and "/sw1" in tail(r)]
        Cn = lambda r: "c" if r["entry"] == "fwd" else "da"
        assert any(r["ld"][Cn(r)] % 4 for r in sw1) and any(r["shift"].get(Cn(r), 0) % 4 for r in sw1), mask
        if mask == "H":
            assert any(r["ld"]["a"] % 4 and not r["ld"]["da"] % 4 for r in sw1) and any(r["shift"].get("a", 0) % 4 for r in sw1)
    # the class layer: each bf16x3 option meets every row count, every stride of H1 and dH1, every form of W2's stride
    for opt, (entry, kernel) in itertools.product((1, 2), (("fwd", "class_fwd"), ("bwd_ex", "class_bwd"))):
        rows = [R.PATHS[f"class-{entry[:3]}-p{p}-opt{opt}"] for p in R.CLS_P]
        assert len(rows) == 8 and all(kernel in r["name"] for r in rows)
        assert {r["m"] for r in rows} == set(R.CLS_M) == {2048, 2049, 2079} and {r["ld"]["a"] for r in rows} == set(R.CLS_LD) == {128, 132, 160}
        assert {r["ld"]["b"] - r["p"] for r in rows} >= {0, 1, 3} and any(r["ld"]["b"] == R.ceil4(r["p"]) > r["p"] + 1 for r in rows)
        assert {r["ld"]["c" if entry == "fwd" else "dc"] - R.ceil16(r["p"]) for r in rows} == {0, 4, 16}
        assert {bool(r["shift"].get("b")) for r in rows} == {True, False}
        if entry == "bwd_ex":
            assert {r["ld"]["da"] for r in rows} == set(R.CLS_LD) and {r["rowscale"] for r in rows} == {True, False}
            assert {(R.cdiv(r["p"], 16), r["rowscale"]) for r in rows} == set(itertools.product((1, 2, 3, 4), (True, False)))
    # both A-load paths behind vector A, and KCH = 8 refused to scalar A
    for K in (12, 17, 33):
        lo, hi = R.PATHS[f"a-load4-K{K}"], R.PATHS[f"a-batched-K{K}"]
        assert lo["name"] == hi["name"]
        assert not R.rowstream_plan(K, 16, lo["ld"]["a"], lo["ld"]["c"])["batched"] and R.rowstream_plan(K, 16, hi["ld"]["a"], hi["ld"]["c"])["batched"]
    assert ",0>" in R.PATHS["a-kch8-scalar"]["name"] and ",8>" in R.PATHS["a-kch8-vec"]["name"]
    # the four ways into single-float stores behind vector A
    ways = [R.PATHS[f"sw1-way{i}"] for i in range(4)]
    assert all(r["name"].endswith("/sw1") for r in ways)
    assert ways[0]["ld"]["da"] % 4 and ways[1]["shift"].get("da") and ways[2]["ld"]["a"] % 4 and ways[3]["shift"].get("a")
    # every reason a class gate has to say no, once
    assert {k[len("class-fwd-no-"):] for k in R.PATHS if k.startswith("class-fwd-no-")} == {
        "m2047", "p65", "n132", "n64", "lda130", "ldc42", "a-shift1", "a-shift2", "c-shift1", "c-shift2"}
    assert {k[len("class-bwd-no-"):] for k in R.PATHS if k.startswith("class-bwd-no-")} == {
        "m2047", "p65", "n132", "wpr5", "lddc44", "lddc50", "ldda130", "dc-shift2", "da-shift1", "bits-shift1", "bits-shift2", "no-db", "no-bits"}
    for k, r in R.PATHS.items():
        if k.startswith(("class-fwd-no-", "class-bwd-no-")):
            assert "class" not in r["name"] and all(R.gate_of(r, option=o) == r["name"] for o in (0, 1, 2)), k
    for p, opt in itertools.product((1, 16, 17, 32, 33, 48, 49, 64), (0, 1, 2)):
        f, b = R.PATHS[f"class-fwd-p{p}-opt{opt}"], R.PATHS[f"class-bwd-p{p}-opt{opt}"]
        assert ("class_fwd" in f["name"]) == (opt > 0) == ("class_bwd" in b["name"])
        assert f["name"].endswith("/p>32") == (opt > 0 and p > 32)
    assert {R.PATHS[f"class-bwd-p{p}-opt2"]["name"] for p in (1, 16, 17, 32, 33, 48, 49, 64)} == {f"class_bwd<{k}>" for k in (1, 2, 3, 4)}


def test_a_wide_sweep_of_the_gate_gives_every_name_and_no_other():
    seen = set()
    add = lambda name: seen.update(R.kernels_of(name))
    Ks = (1, 12, 16, 17, 33, 48, 64, 65, 100, 128, 130, 288, 304)
    Ncs = (1, 3, 16, 17, 33, 47, 48, 64, 65, 100, 129, 130)
    lds = lambda x: (x, x + 1, x + 2, R.ceil4(x), R.ceil4(x) + 4, R.ceil16(x))
    shapes = [(K, Nc, 17) for K in Ks for Nc in Ncs] + [(41, 48, m) for m in (0, 1, 2100, 8321)]
    for K, Nc, m in shapes:
        for ldA, ldC, aA, aC, aH in itertools.product(lds(K), lds(Nc)[:4], (16, 8, 4), (16, 4), (16, 4)):
            add(R.gate("fwd", m, K, Nc, dict(a=ldA, b=Nc, c=ldC), dict(a=aA, c=aC)))
            st = dict(a=R.ceil4(Nc) + (aH == 4), b=K, dc=ldA, da=ldC, db=K, wpr=R.cdiv(Nc, 32))
            al = dict(a=aH, dc=aA, da=aC)
            add(R.gate("bwd", m, Nc, K, st, al))
            add(R.gate("bwd_fused", m, Nc, K, st, al))
            add(R.gate("bwd_fused_bits", m, Nc, K, st, al))
            add(R.gate("bwd_da_bits", m, Nc, K, st, al))
            for mk in ("H", "bits"):
                add(R.gate("bwd_ex", m, Nc, K, st, al, mask_kind=mk, has_rowscale=bool(m & 1)))
    for m, p, opt, lda, ldp, ldda, wpr, al, db, mk in itertools.product((2047, 2048, 40000), (1, 16, 17, 33, 41, 49, 64, 65), (0, 1, 2), (128, 130, 132),
                                                                        (0, 1, 4, 16), (128, 130), (4, 5), (16, 8), (True, False), ("H", "bits")):
        ldc = R.ceil4(p) + ldp
        add(R.gate("fwd", m, 128, p, dict(a=lda, b=p, c=ldc), dict(a=al), option=opt))
        add(R.gate("fwd", m, 128, p, dict(a=lda, b=p, c=ldc), dict(c=al), option=opt))
        for which in ("dc", "da", "bits", "a"):
            add(R.gate("bwd_ex", m, 128, p, dict(a=lda, b=p, dc=ldc, da=ldda, db=p, wpr=wpr), {which: al}, option=opt, has_db=db, mask_kind=mk))
    assert seen - {"refused"} <= R.every_name(), sorted(seen - R.every_name())
    assert R.every_name() <= seen, sorted(R.every_name() - seen)
    assert "refused" in seen


def test_the_gate_at_the_edges_the_issue_names():
    fwd = lambda m=2048, p=41, lda=128, ldc=48, opt=2, **al: R.gate("fwd", m, 128, p, dict(a=lda, b=p, c=ldc), al, option=opt)
    ex = lambda m=2048, p=41, lddc=48, opt=2, db=True, mk="bits", wpr=4, ldda=128, **al: R.gate(
        "bwd_ex", m, 128, p, dict(a=128, b=p, dc=lddc, da=ldda, db=p, wpr=wpr), al, option=opt, has_db=db, mask_kind=mk)
    # 2047 / 2048 rows, 64 / 65 classes
    assert fwd() == "class_fwd/p>32" and "class" not in fwd(m=2047) and fwd(p=32) == "class_fwd" and fwd(p=33) == "class_fwd/p>32"
    assert fwd(p=64, ldc=64) == "class_fwd/p>32" and "class" not in fwd(p=65, ldc=68) and "class" not in fwd(opt=0) and fwd(opt=1) == fwd()
    assert ex() == "class_bwd<3>" and "class" not in ex(m=2047) and ex(p=64, lddc=64) == "class_bwd<4>" and "class" not in ex(p=65, lddc=80)
    # lddc = 44, which is what (p + 3) / 4 * 4 gives for 41 classes, against 48: whole k-steps of 16 classes are read
    assert "class" not in ex(lddc=44) and ex(lddc=48) == ex(lddc=52) == ex(lddc=64) == "class_bwd<3>" and "class" not in ex(lddc=50)
    assert all("class" not in x for x in (ex(wpr=5), ex(ldda=130), ex(db=False), ex(mk="H"), ex(dc=4), ex(da=8), ex(bits=4), ex(opt=0)))
    assert ex(a=4) == "class_bwd<3>"                                                  # H1 is read dword by dword
    assert all("class" not in x for x in (fwd(lda=130), fwd(ldc=42), fwd(a=8), fwd(c=4)))
    assert not R.cls_fwd_fits(1 << 23, 128, 41, 128, 48) and R.cls_fwd_fits((1 << 23) - 1, 128, 41, 128, 48)      # 32-bit buffer offsets
    # K = 288 is the last that fits beside 8 tiles of columns, K = 304 is refused; with the staged epilogue's 33 KiB: K = 224 / 240
    lds = lambda K, **kw: R.rowstream_plan(K, 100, kw.pop("lda", R.ceil4(K)), 100, **kw)["lds"]
    assert lds(288) == 288 * 132 * 4 <= R.LDS_LIMIT < lds(304)
    assert lds(224, lda=225) == (224 * 132 + 64 * 132) * 4 <= R.LDS_LIMIT < lds(240, lda=241)
    g = lambda K, lda=None: R.gate("fwd", 17, K, 100, dict(a=lda or K, b=100, c=100))
    assert g(288) == "rowstream<8,vec,none,0>/sw4" and g(304) == "refused" and g(224, 225).endswith("/staged") and g(240, 241) == "refused"
    assert R.gate("fwd", 17, 304, 64, dict(a=304, b=64, c=64)) == "rowstream<4,vec,none,0>/sw4"       # fewer columns: a longer K fits
    bw = lambda e, **kw: R.gate(e, 17, 65, 304, dict(a=68, b=304, dc=304, da=68, db=304, wpr=3), **kw)
    assert all(bw(e) == "refused" for e in R.ENTRIES[1:]) and bw("bwd", has_da=False) == "atb<4,4>+reduce<64>"
    tiers = [R.rowstream_plan(K, 100, R.ceil4(K), 100) for K in (48, 64, 128, 160, 288)]
    assert [(q["per_cu"], q["attribute"]) for q in tiers] == [(4, False), (2, False), (2, True), (1, True), (1, True)]
    assert [R.PATHS[f"lds-K{K}"]["n"] for K in (48, 64, 128, 160, 288)] == [48, 64, 128, 160, 288]
    # KCH: chunks of 16 up to 4, then 8 for K in (112, 128] behind vector A with 128 floats per row
    assert [R.rowstream_plan(K, 16, R.ceil16(K), 16)["kch"] for K in (1, 16, 17, 32, 33, 48, 49, 64, 65, 96, 112, 113, 128, 129)] == [
        1, 1, 2, 2, 3, 3, 4, 4, 0, 0, 0, 8, 8, 0]
    assert R.rowstream_plan(113, 16, 116, 16)["kch"] == 0 and R.rowstream_plan(128, 16, 129, 16)["kch"] == 0
    # the three slab sums
    assert [R.slab_reduce_opb(t, s) for t, s in ((32768, 500), (32767, 16), (32767, 17), (8192, 500), (8191, 64), (8191, 65))] == [64, 64, 16, 16, 16, 8]
    assert R.atb_plan(8321, 128, 41, 4, 4)["n_slabs"] == 66 and R.atb_name(8321, 128, 41, 128, 16, 44, 16) == "atb<4,4>+reduce<8>"
    assert R.atb_plan(1, 48, 41, 4, 4) == dict(gy=1, gz=1, rows_per_worker=4, n_workers=1, n_slabs=1)
    # 129 rows: 5 workers asked for, 8 after rounding, 20 rows each: 7 have rows, the second workgroup has three live waves
    assert R.atb_plan(129, 100, 70, 4, 4) == dict(gy=2, gz=2, rows_per_worker=20, n_workers=7, n_slabs=2)
    assert [R.atb_vec(ld, al) for ld, al in ((48, 16), (48, 8), (48, 4), (50, 16), (49, 16), (50, 4))] == [4, 2, 1, 2, 1, 1]
    # the three grid caps as functions of the CU count, and the table's three cases past them
    for n_cu in (64, 256, 304):
        assert R.rowstream_cap_rows(0, n_cu) == 4 * 64 * n_cu and R.rowstream_cap_rows(33 << 10, n_cu) == 2 * 64 * n_cu and R.rowstream_cap_rows(77 << 10, n_cu) == 64 * n_cu
        assert R.cls_bwd_cap_rows(n_cu) == 4 * 32 * n_cu and R.cls_fwd_cap_rows(n_cu) == 3 * 4 * 32 * n_cu
    assert R.PATHS["rows-past-the-cap"]["m"] > R.rowstream_cap_rows(0) and R.PATHS["class-bwd-past-the-cap"]["m"] > R.cls_bwd_cap_rows()
    assert R.PATHS["class-fwd-past-the-cap"]["m"] == 3 * 4 * 32 * 256 + 37 > R.cls_fwd_cap_rows()
    assert sorted(r["m"] for r in R.PATHS.values() if r["m"] > 10000) == [R.BIG_CLS_BWD_M, R.BIG_ROWSTREAM_M, R.BIG_CLS_FWD_M]
    # argument checks: every entry point
    st = dict(a=48, b=44, c=44, dc=44, da=48, db=44, wpr=2)
    for e in R.ENTRIES:
        assert R.gate(e, 0, 48, 41, st) == ("" if e in ("fwd", "bwd_da_bits") else "zero_rows")
        assert R.gate(e, 17, 48, 41, dict(st, b=40)) == "refused" and R.gate(e, -1, 48, 41, st) == "refused"
        if e != "bwd_da_bits":
            assert R.gate(e, 17, 48, 41, dict(st, a=47), mask_kind="H" if e == "bwd_ex" else None) == "refused"
        if R.MASK_OF[e] in ("bits", None):
            assert R.gate(e, 17, 48, 41, dict(st, wpr=1)) == "refused"
    assert R.gate("bwd_ex", 17, 48, 41, dict(st, a=47), has_db=False, mask_kind="bits") != "refused"      # a is not read at all
    assert all(R.gate("bwd_ex", 17, 48, 41, st, scale=s) == "refused" for s in (0.0, -1.0, float("nan")))
