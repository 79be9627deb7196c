"""One Matmul call in float64, the choice of its kernels as a pure function, and the table of paths.

fwd_ref / bwd_ref restate gcnhip_matmul_fwd and the five backward entry points (csrc/matmul.hip); gate() restates what each of
them launches — launch_rowstream, launch_atb and launch_slab_reduce (csrc/dense_kernels.h), cls_fwd_fits, cls_bwd_fits and the
two class-layer launchers (csrc/class_bf16x3.h, matmul.hip).  PATHS gives every name a smallest shape that reaches it.
test_matmul_dispatch_cpu.py proves all three before a GPU sees them, test_matmul_dispatch_gpu.py holds every row of the
table to the float64 product.

A name says which kernel template runs and which of its run-time forms:
    rowstream<NT,vec|scalar,none|H|bits,KCH>/sw4|sw1|staged|plain[/y>1]
        NT 16-column tiles per workgroup, 16-byte or scalar loads of A, the mask source, KCH chunks of 16 along K (0: the
        generic loop); the epilogue: the transposed tile's 16-byte row stores (sw4) or single floats (sw1) behind vector A, the
        LDS-staged row stores (staged) or one float per lane (plain) behind scalar A; y>1: a second column block
    atb<VA,VB>+reduce<OPB>      the split-K weight gradient and the slab sum behind it
    class_fwd[/p>32], class_bwd<NKS>   the bf16x3 class-layer kernels
    zero_rows                   m == 0 with a db: one memset per row of db
A call's names are joined with " | " in launch order; "" says nothing is launched, "refused" that the call returns -1.
"""
import itertools

import numpy as np

EPS = float(np.finfo(np.float32).eps)
N_CU = 256                                               # compute units of an MI355X (the launchers read the device's count)
LDS_LIMIT = 156 * 1024                                   # launch_rowstream refuses above this
ENTRIES = ("fwd", "bwd", "bwd_fused", "bwd_fused_bits", "bwd_ex", "bwd_da_bits")
MASK_OF = {"fwd": "none", "bwd": "none", "bwd_fused": "H", "bwd_fused_bits": "bits", "bwd_ex": None, "bwd_da_bits": "bits"}


def cdiv(a, b):
    return -(-a // b)


def ceil4(x):
    return cdiv(x, 4) * 4


def ceil16(x):
    return cdiv(x, 16) * 16


# ---------------------------------------------------------------------------------------------------------- float64
def _f64(x):
    return np.asarray(x, np.float32).astype(np.float64)


def fwd_ref(a, b):
    """-> (want, mag) float64 [m, p]: a . b and |a| . |b|"""
    a, b = _f64(a), _f64(b)
    return a @ b, np.abs(a) @ np.abs(b)


def pack_bits(mask, wpr=None):
    """bit (c & 31) of word [r, c >> 5] = mask[r, c] -> uint32 [m, wpr]"""
    mask = np.asarray(mask, bool)
    m, n = mask.shape
    wpr = wpr or cdiv(n, 32)
    bits = np.zeros((m, wpr), np.uint32)
    for c in range(n):
        bits[:, c // 32] |= mask[:, c].astype(np.uint32) << np.uint32(c % 32)
    return bits


def unpack_bits(bits, n):
    bits = np.asarray(bits, np.uint32)
    c = np.arange(n)
    return ((bits[:, c // 32] >> (c % 32).astype(np.uint32)) & np.uint32(1)).astype(bool)


def positive(a):
    """the mask the kernels take from activations: a > 0 in float32 (false for -0.0, true for a positive denormal)"""
    return np.asarray(a, np.float32) > np.float32(0)


def row_factor(m, scale=None, rowscale=None):
    """the factor of row r as the kernels form it: scale * rowscale[r] in float32 (1 without a mask epilogue) -> float64 [m, 1]"""
    if scale is None:
        return np.ones((m, 1))
    f = np.full(m, np.float32(scale), np.float32)
    if rowscale is not None:
        f = f * np.asarray(rowscale, np.float32)
    return f.astype(np.float64)[:, None]


def bwd_ref(a, b, dc, mask=None, scale=None, rowscale=None):
    """-> ((da, mag_da), (db, mag_db)) float64: da = mask . f_r . (dc . b^T), db = a^T . dc, and the same products on absolute
    values (mag_da carries the row factors, not the mask).  mask: bool [m, n] or None; a = None: no db"""
    b, dc = _f64(b), _f64(dc)
    f = row_factor(dc.shape[0], scale, rowscale)
    prod, mag = (dc @ b.T) * f, (np.abs(dc) @ np.abs(b.T)) * np.abs(f)
    da = prod if mask is None else np.where(np.asarray(mask, bool), prod, 0.0)
    if a is None:
        return (da, mag), (None, None)
    a = _f64(a)
    return (da, mag), (a.T @ dc, np.abs(a).T @ np.abs(dc))


# ------------------------------------------------------------------------------------------------------------- gate
def al_of(shift):
    """byte alignment of an address `shift` four-byte words into a 16-byte-aligned allocation"""
    return 16 if shift % 4 == 0 else 8 if shift % 2 == 0 else 4


def rowstream_plan(K, Nc, lda, ldc, a_al=16, c_al=16, mask="none", ldh=0, h_al=16):
    """launch_rowstream's choices -> dict(vec, vec_out, NT, gy, kch, staged, lds, per_cu, batched) (lds > LDS_LIMIT: refused)"""
    vec = lda % 4 == 0 and a_al % 16 == 0
    vec_out = ldc % 4 == 0 and c_al % 16 == 0 and (mask != "H" or (ldh % 4 == 0 and h_al % 16 == 0))
    if not vec:
        vec_out = vec_out and Nc >= 64
    nt_total = cdiv(Nc, 16)
    NT = 8 if nt_total > 4 else 4 if nt_total > 3 else nt_total
    Kp = ceil16(K)
    staged = vec_out and not vec
    lds = (Kp * (NT * 16 + 4) + (4 * 16 * (NT * 16 + 4) if staged else 0)) * 4
    kch = Kp // 16 if Kp <= 128 and Kp // 16 in (1, 2, 3, 4, 8) else 0
    if kch == 8 and not (vec and lda >= 128):
        kch = 0
    return dict(vec=vec, vec_out=vec_out, NT=NT, gy=cdiv(nt_total, NT), kch=kch, staged=staged, lds=lds,
                per_cu=1 if lds > 76 * 1024 else 2 if lds > 32 * 1024 else 4, attribute=lds > 64 * 1024,
                batched=bool(vec and kch and lda >= 16 * kch))           # the KCH loads issued together; else load4 per chunk


def rowstream_name(q, mask):
    epi = ("sw4" if q["vec_out"] else "sw1") if q["vec"] else ("staged" if q["vec_out"] else "plain")
    return f"rowstream<{q['NT']},{'vec' if q['vec'] else 'scalar'},{mask},{q['kch']}>/{epi}" + ("/y>1" if q["gy"] > 1 else "")


def rowstream_cap_rows(lds, n_cu=N_CU):
    """rows one pass of the capped grid covers: workgroups x 4 waves x 16 rows"""
    return n_cu * (1 if lds > 76 * 1024 else 2 if lds > 32 * 1024 else 4) * 64


def atb_vec(ld, al):
    return 4 if ld % 4 == 0 and al % 16 == 0 else 2 if ld % 2 == 0 and al % 8 == 0 else 1


def atb_plan(m, n, p, VA, VB, n_cu=N_CU):
    """launch_atb's split -> dict(gy, gz, rows_per_worker, n_workers, n_slabs)"""
    p_ld = ceil4(p)
    gy, gz = cdiv(n, 16 * VA), cdiv(p, 16 * VB)
    slab = n * p_ld * 4
    workers = cdiv(n_cu * (16 if slab <= (256 << 10) else 4), gy * gz)
    while workers > 4 and (workers // 4) * slab > (12 << 20):
        workers = workers * 3 // 4
    workers = max(1, min(workers, cdiv(m, 32)))
    workers = cdiv(workers, 4) * 4
    rpw = ceil4(cdiv(m, workers))
    n_workers = cdiv(m, rpw)
    return dict(gy=gy, gz=gz, rows_per_worker=rpw, n_workers=n_workers, n_slabs=cdiv(n_workers, 4))


def slab_reduce_opb(total, n_slabs):
    return 64 if total >= 64 * 512 or n_slabs <= 16 else 16 if total >= 16 * 512 or n_slabs <= 64 else 8


def atb_name(m, n, p, lda, a_al, lddc, dc_al, n_cu=N_CU):
    VA, VB = atb_vec(lda, a_al), atb_vec(lddc, dc_al)
    return f"atb<{VA},{VB}>+reduce<{slab_reduce_opb(n * p, atb_plan(m, n, p, VA, VB, n_cu)['n_slabs'])}>"


def cls_fwd_fits(m, n, p, lda, ldc, a_al=16, c_al=16):
    return (n == 128 and 1 <= p <= 64 and m >= 2048 and lda % 4 == 0 and lda >= 128 and ldc % 4 == 0 and a_al % 16 == 0 and c_al % 16 == 0
            and m * lda * 4 < (1 << 32))


def cls_bwd_fits(m, n, p, lda, lddc, ldda, wpr, has_bits=True, dc_al=16, da_al=16, bits_al=16):
    return (n == 128 and 1 <= p <= 64 and m >= 2048 and wpr == 4 and has_bits and bits_al % 16 == 0 and lda >= 128 and lddc % 4 == 0
            and lddc >= ceil16(p) and ldda % 4 == 0 and ldda >= 128 and dc_al % 16 == 0 and da_al % 16 == 0 and m * lda * 4 < (1 << 32)
            and m * lddc * 4 < (1 << 32))


def cls_fwd_cap_rows(n_cu=N_CU):
    return 3 * n_cu * 4 * 32                               # three workgroups per CU, four waves, a 32-row block each


def cls_bwd_cap_rows(n_cu=N_CU):
    return n_cu * 4 * 32                                   # one workgroup per CU, four wave pairs


def gate(entry, m, n, p, strides, alignments=None, option=2, has_db=True, mask_kind=None, has_rowscale=False, n_cu=N_CU, has_da=True,
         scale=1.0):
    """the names of what one call launches, " | "-joined in launch order.  strides: dict(a, b, c | dc, da, db, wpr);
    alignments: byte alignment per operand (a, c, dc, da, bits; 16 where not given); option: the context's gemm_bf16x3;
    mask_kind: "H" | "bits" for bwd_ex (and "none" for an entry point that is handed no mask words it needs)"""
    s, al = strides, dict(alignments or {})
    A = lambda k: al.get(k, 16)
    mask = MASK_OF[entry] or mask_kind or "bits"
    if mask_kind is not None and MASK_OF[entry] is not None and mask_kind != MASK_OF[entry]:
        return "refused"                                     # the entry point was not handed the mask words it needs
    if m < 0 or n <= 0 or p <= 0 or s["b"] < p:
        return "refused"
    if entry == "fwd":
        if s["a"] < n or s["c"] < p:
            return "refused"
        if m == 0:
            return ""
        if option >= 1 and cls_fwd_fits(m, n, p, s["a"], s["c"], A("a"), A("c")):
            return "class_fwd/p>32" if p > 32 else "class_fwd"
        q = rowstream_plan(n, p, s["a"], s["c"], A("a"), A("c"))
        return "refused" if q["lds"] > LDS_LIMIT else rowstream_name(q, "none")
    if s["dc"] < p:
        return "refused"
    if entry == "bwd_da_bits":
        has_db = False
    if entry in ("bwd_fused_bits", "bwd_ex", "bwd_da_bits") and not has_da:
        return "refused"
    if has_da and s["da"] < n:
        return "refused"
    if has_db and s["db"] < p:
        return "refused"
    needs_a = entry in ("bwd", "bwd_fused", "bwd_fused_bits") or has_db or mask == "H"
    if needs_a and s["a"] < n:
        return "refused"
    if mask == "bits" and s["wpr"] * 32 < n:
        return "refused"
    if entry == "bwd_ex" and not scale > 0:
        return "refused"
    if m == 0:
        return "zero_rows" if has_db else ""
    if (entry == "bwd_ex" and has_db and option >= 1
            and cls_bwd_fits(m, n, p, s["a"], s["dc"], s["da"], s["wpr"], mask == "bits", A("dc"), A("da"), A("bits"))):
        return f"class_bwd<{cdiv(p, 16)}>"
    names = []
    if has_da:
        q = rowstream_plan(p, n, s["dc"], s["da"], A("dc"), A("da"), mask, s["a"], A("a"))
        if q["lds"] > LDS_LIMIT:
            return "refused"
        names.append(rowstream_name(q, mask))
    if has_db:
        names.insert(0, atb_name(m, n, p, s["a"], A("a"), s["dc"], A("dc"), n_cu))
    return " | ".join(names)


def rowstream_names():
    out = set()
    for NT, vec, mask, kch in itertools.product((1, 2, 3, 4, 8), (True, False), ("none", "H", "bits"), (0, 1, 2, 3, 4, 8)):
        if kch == 8 and not vec:
            continue
        for epi in (("sw4", "sw1") if vec else ("plain", "staged") if NT >= 4 else ("plain",)):
            for y in (("", "/y>1") if NT == 8 else ("",)):
                out.add(f"rowstream<{NT},{'vec' if vec else 'scalar'},{mask},{kch}>/{epi}{y}")
    return out


def every_name():
    """every name a launch can have (refusals aside), written out from the template lists of dense_kernels.h and matmul.hip"""
    names = rowstream_names() | {"zero_rows", "class_fwd", "class_fwd/p>32"} | {f"class_bwd<{k}>" for k in (1, 2, 3, 4)}
    names |= {f"atb<{va},{vb}>+reduce<{o}>" for va in (1, 2, 4) for vb in (1, 2, 4) for o in (8, 16, 64)}
    return names


def kernels_of(name):
    """the single launches of a call's name"""
    return [k for k in name.split(" | ") if k]


# ------------------------------------------------------------------------------------------------------- the table
# id -> dict(entry, m, n, p, ld {a, b, c | dc, da, db, wpr}, shift {operand: words}, opt (gemm_bf16x3), db, da, mask ("none" | "H"
# | "bits"), rowscale, scale, name = what gate() must answer)
def _row(entry, m, n, p, name, ld=None, shift=None, opt=2, db=None, da=True, mask=None, rowscale=False, scale=2.0):
    ld = dict(ld or {})
    ld.setdefault("a", n), ld.setdefault("b", ceil4(p)), ld.setdefault("wpr", cdiv(n, 32))
    if entry == "fwd":
        ld.setdefault("c", ceil4(p))
    else:
        ld.setdefault("dc", ceil4(p)), ld.setdefault("da", n), ld.setdefault("db", ceil4(p))
    mask = mask if mask is not None else (MASK_OF[entry] or "bits")
    db = (entry not in ("fwd", "bwd_da_bits")) if db is None else db
    return dict(entry=entry, m=m, n=n, p=p, ld=ld, shift=dict(shift or {}), opt=opt, db=db, da=da, mask=mask,
                rowscale=bool(rowscale and entry == "bwd_ex"), scale=scale, name=name)


def gate_of(row, n_cu=N_CU, **over):
    """gate() on a table row"""
    al = {k: al_of(v) for k, v in row["shift"].items()}
    kw = dict(entry=row["entry"], m=row["m"], n=row["n"], p=row["p"], strides=row["ld"], alignments=al, option=row["opt"], has_db=row["db"],
              mask_kind=row["mask"], has_rowscale=row["rowscale"], n_cu=n_cu, has_da=row["da"],
              scale=row["scale"])
    kw.update(over)
    return gate(**kw)


CLS_P = (1, 16, 17, 32, 33, 48, 49, 64)                   # NKS 1-4 of the class backward, the second class block of both kernels
CLS_M = (2048, 2049, 2048 + 31)                            # whole 32-row blocks, one row more, a last block of 31
CLS_LD = (128, 132, 160)                                   # row strides of H1 and of dH1
NC_OF = {1: (1, 3, 16), 2: (17,), 3: (33, 47, 48), 4: (64,), 8: (65, 100)}
NC_Y = (129, 130)                                          # a second column block, with one and with two mask words more
K_OF = {1: (1, 12, 16), 2: (17,), 3: (33, 48), 4: (64,), 8: (128,), 0: (65, 100, 130, 288)}
K_SCALAR_0 = (65, 100, 128, 130, 288)                      # K = 128 behind scalar A: KCH = 8 is refused, the generic loop runs
MS = (1, 15, 16, 17, 65)
MASK_ENTRIES = {"none": ("fwd", "bwd"), "H": ("bwd_fused", "bwd_ex"), "bits": ("bwd_fused_bits", "bwd_ex", "bwd_da_bits")}
BIG_ROWSTREAM_M = 4 * 64 * N_CU + 17
BIG_CLS_BWD_M = 4 * 32 * N_CU + 37
BIG_CLS_FWD_M = 3 * 4 * 32 * N_CU + 37


def _not4(x):
    """the next stride >= x that is no multiple of 4"""
    return x if x % 4 else x + 1


def unvec_ways(mask):
    """the ways out of 16-byte stores: a stride of C that is no multiple of 4, a shifted C and, where H gives the mask, the same of H"""
    return ("ld", "shift") + (("ldh", "shifth") if mask == "H" else ())


def rowstream_row(entry, mask, m, K, Nc, vec, epi, i=0, rowscale=False, wide_a=False, way=None, scalar_by=None):
    """the row of one row-stream form: K and Nc as the kernel sees them (fwd: n, p; the backward entries: p, n).  i picks
    among the ways to the same form: a stride that is no multiple of 4, or an operand one float into its allocation"""
    fwd = entry == "fwd"
    A, Cn = ("a", "c") if fwd else ("dc", "da")
    n, p = (K, Nc) if fwd else (Nc, K)
    ld, shift = {}, {}
    if vec:
        ld[A] = ceil16(K) if wide_a else ceil4(K)
    elif K == 128 or (scalar_by or ("stride", "shift")[i % 2]) == "stride":
        ld[A] = _not4(K)
    else:
        ld[A], shift[A] = ceil4(K) + 4, 1 + 2 * (i // 2 % 2)
    ld[Cn] = ceil4(Nc) + (4 if i % 3 == 1 else 0)
    if not fwd:
        ld["a"] = ceil4(Nc)
    if epi == "sw1" or (epi == "plain" and Nc >= 64):
        ways = unvec_ways(mask)
        way = way or ways[i % len(ways)]
        if way == "ld":
            ld[Cn] = _not4(Nc)
        elif way == "shift":
            shift[Cn] = 1 + i % 3
        elif way == "ldh":
            ld["a"] = _not4(Nc)
        else:
            shift["a"] = 2
    if not fwd:
        ld["b"] = (K, K + 1, ceil4(K))[i % 3]
        if i % 4 == 3:
            shift["b"] = 1
        ld["db"] = ceil4(K) + (1 if i % 2 else 0)
        if mask == "bits":
            ld["wpr"] = cdiv(Nc, 32) + (1 if i % 5 == 2 else 0)
            if i % 7 == 3:
                shift["bits"] = 1
    else:
        ld["b"] = (Nc, Nc + 1, ceil4(Nc))[i % 3]
    row = _row(entry, m, n, p, "", ld=ld, shift=shift, mask=mask, rowscale=rowscale, opt=2)
    row["name"] = gate_of(row)
    return row


def _paths():
    P = {}
    cnt = itertools.count()
    turn = {}

    def pick(seq, key=None):                               # each list in turn (one turn per key), whatever else varies beside it
        turn[key, seq] = turn.get((key, seq), -1) + 1
        return seq[turn[key, seq] % len(seq)]
    # ---- every (NT, VEC, mask source, KCH) of gemm_rowstream_kernel once per entry point that reaches it, the epilogue forms
    # and the second column block spread over them
    for mask, NT, vec, kch in itertools.product(("none", "H", "bits"), (1, 2, 3, 4, 8), (True, False), (0, 1, 2, 3, 4, 8)):
        if kch == 8 and not vec:
            continue
        forms = [(e, y) for e in (("sw4", "sw1") if vec else ("plain", "staged") if NT >= 4 else ("plain",)) for y in ((0, 1) if NT == 8 else (0,))]
        entries = MASK_ENTRIES[mask]
        for j in range(max(len(forms), len(entries))):
            i = next(cnt)
            entry, (epi, y) = entries[j % len(entries)], forms[j % len(forms)]
            Ks = K_OF[kch] if vec or kch else K_SCALAR_0
            K = pick(Ks)
            if NT == 8 and epi == "staged" and K == 288:      # 149 KiB of W and 33 KiB of staging: refused (its own row below)
                K = 130
            Ncs = NC_Y if y else NC_OF[NT]
            Nc = pick(Ncs)
            # a row factor on every other gcnhip_matmul_bwd_ex row of each (mask source, A loads, epilogue)
            rs = entry == "bwd_ex" and pick((True, False), (mask, vec, epi))
            way = pick(unvec_ways(mask), (entry, vec)) if epi == "sw1" or (epi == "plain" and Nc >= 64) else None
            by = None if vec else pick(("stride", "shift"), (entry, mask))
            row = rowstream_row(entry, mask, pick(MS), K, Nc, vec, epi, i, rowscale=rs, way=way, scalar_by=by)
            want = f"rowstream<{NT},{'vec' if vec else 'scalar'},{mask},{kch}>/{epi}" + ("/y>1" if y else "")
            assert kernels_of(row["name"])[-1] == want, (row, want)
            P[f"rs-{entry}-{want[10:]}"] = row
    # ---- each epilogue form with each mask source, with and without a row factor (gcnhip_matmul_bwd_ex), two column blocks
    for mask, (vec, epi), rs in itertools.product(("H", "bits"), ((True, "sw4"), (True, "sw1"), (False, "staged"), (False, "plain")), (False, True)):
        i = next(cnt)
        P[f"epi-{mask}-{epi}-{'rowscale' if rs else 'plain'}"] = rowstream_row("bwd_ex", mask, 33, 41, 130, vec, epi, i, rowscale=rs)
    for way in range(4):                                   # sw1 by ldc % 4, by a misaligned C, by an odd-stride H, by a misaligned H
        P[f"sw1-way{way}"] = rowstream_row("bwd_fused", "H", 17, 16, 47, True, "sw1", way)
    # ---- A loads: the KCH loads of a row issued together need 16 KCH floats in the row's allocation
    for K, kch in ((12, 1), (17, 2), (33, 3)):
        P[f"a-load4-K{K}"] = rowstream_row("fwd", "none", 17, K, 16, True, "sw4")
        P[f"a-batched-K{K}"] = rowstream_row("fwd", "none", 17, K, 16, True, "sw4", wide_a=True)
    P["a-kch8-scalar"] = rowstream_row("fwd", "none", 17, 128, 41, False, "plain")
    P["a-kch8-vec"] = rowstream_row("fwd", "none", 17, 128, 41, True, "sw4")
    # ---- the LDS tiers: <= 32 KiB, > 32 KiB (two workgroups per CU), > 64 KiB (the attribute), > 76 KiB (one), the last K that fits
    for K, Nc in ((48, 100), (64, 100), (128, 100), (160, 100), (288, 100)):
        P[f"lds-K{K}"] = rowstream_row("fwd", "none", 65, K, Nc, True, "sw4")
    P["lds-K288-bwd"] = rowstream_row("bwd_fused", "H", 33, 288, 65, True, "sw4")
    P["rows-past-the-cap"] = rowstream_row("fwd", "none", BIG_ROWSTREAM_M, 16, 16, True, "sw4")
    # ---- gemm_atb_kernel: every (VA, VB) by stride parity and by address; worker shapes; the three slab sums
    n0, p0 = 48, 41
    V_LD = {4: 0, 2: 2, 1: 1}                              # added to a multiple of 4
    for VA, VB in itertools.product((4, 2, 1), (4, 2, 1)):
        for how in ("stride", "address"):
            for m, tag in ((33, ""), (2100, "-r16"), (8321, "-r8")):
                if how == "stride":
                    ld, sh = dict(a=ceil4(n0) + V_LD[VA], dc=ceil4(p0) + V_LD[VB]), {}
                else:
                    ld = dict(a=ceil4(n0) + (4 if VA != 1 else 0), dc=ceil4(p0))
                    sh = {k: {4: 0, 2: 2, 1: 1}[v] for k, v in (("a", VA), ("dc", VB)) if v != 4}
                    if not sh:
                        continue
                opb = {"": 64, "-r16": 16, "-r8": 8}[tag]
                P[f"atb-{VA}{VB}-{how}{tag}"] = _row("bwd", m, n0, p0, f"atb<{VA},{VB}>+reduce<{opb}>", ld=ld, shift=sh, da=False)
    for i, m in enumerate((1, 31, 32, 33, 127, 129)):      # one worker, ragged worker tails, fewer than four live waves at the end
        VA, VB = ((4, 4), (2, 1), (1, 2))[i % 3]
        ld = dict(a=ceil4(100) + V_LD[VA], dc=ceil4(70) + V_LD[VB])
        name = f"atb<{VA},{VB}>+reduce<64> | " + rowstream_name(rowstream_plan(70, 100, ld["dc"], 100, mask="H", ldh=ld["a"]), "H")
        P[f"atb-m{m}"] = _row("bwd_fused", m, 100, 70, name, ld=ld)            # n > 64, p > 64: gridDim.y, gridDim.z > 1
    # ---- the class layer: both bf16x3 kernels, and what takes over under option 0
    # (pi, oi: the indices of p and of the option.  Every choice below runs through all of its values over pi at EACH oi, so
    #  both bf16x3 options meet every m, lda, ldda, lddc and ldb form: test_matmul_dispatch_cpu.py counts them)
    for (pi, p), (oi, opt) in itertools.product(enumerate(CLS_P), enumerate((2, 1, 0))):
        m = CLS_M[(pi + oi) % 3]
        lda, ldda = CLS_LD[(pi + 2 * oi + 1) % 3], CLS_LD[(pi // 3 + oi) % 3]
        lddc = ceil16(p) + (0, 4, 16)[(pi // 2 + oi) % 3]
        ldb = (p, p + 1, ceil4(p))[(2 * pi + oi) % 3]
        sh = dict(b=1) if (pi + oi) % 2 else {}
        i = pi + pi // 2 + oi                              # the row factor and the stride of db: on and off at every NKS
        fq, bq = rowstream_plan(128, p, lda, lddc), rowstream_plan(p, 128, lddc, ldda, mask="bits")
        P[f"class-fwd-p{p}-opt{opt}"] = _row("fwd", m, 128, p, ("class_fwd/p>32" if p > 32 else "class_fwd") if opt else rowstream_name(fq, "none"),
                                             ld=dict(a=lda, b=ldb, c=lddc), shift=sh, opt=opt)
        name = f"class_bwd<{cdiv(p, 16)}>" if opt else atb_name(m, 128, p, lda, 16, lddc, 16) + " | " + rowstream_name(bq, "bits")
        P[f"class-bwd-p{p}-opt{opt}"] = _row("bwd_ex", m, 128, p, name, ld=dict(a=lda, b=ldb, dc=lddc, da=ldda, db=ceil4(p) + (i % 2), wpr=4), shift=sh,
                                             opt=opt, mask="bits", rowscale=i % 2 == 0)
    P["class-bwd-past-the-cap"] = _row("bwd_ex", BIG_CLS_BWD_M, 128, 41, "class_bwd<3>", ld=dict(dc=48, wpr=4), mask="bits", rowscale=True)
    P["class-fwd-past-the-cap"] = _row("fwd", BIG_CLS_FWD_M, 128, 41, "class_fwd/p>32", ld=dict(c=48))
    P["class-bwd-odd-lda"] = _row("bwd_ex", 2049, 128, 41, "class_bwd<3>", ld=dict(a=130, dc=48, wpr=4), shift=dict(a=1), mask="bits")   # H1 is read by dwords
    # ---- every reason a class gate says no, one at a time: the f32-MFMA kernels run
    f = lambda why, name, m=2049, n=128, p=41, ld=None, shift=None: P.__setitem__(
        f"class-fwd-no-{why}", _row("fwd", m, n, p, name, ld=dict(dict(c=48), **(ld or {})), shift=shift))
    f("m2047", "rowstream<3,vec,none,8>/sw4", m=2047)
    f("p65", "rowstream<8,vec,none,8>/sw4", p=65, ld=dict(c=80))
    f("n132", "rowstream<3,vec,none,0>/sw4", n=132)
    f("n64", "rowstream<3,vec,none,4>/sw4", n=64)
    f("lda130", "rowstream<3,scalar,none,0>/plain", ld=dict(a=130))
    f("ldc42", "rowstream<3,vec,none,8>/sw1", ld=dict(c=42))
    f("a-shift1", "rowstream<3,scalar,none,0>/plain", shift=dict(a=1))
    f("a-shift2", "rowstream<3,scalar,none,0>/plain", shift=dict(a=2))
    f("c-shift1", "rowstream<3,vec,none,8>/sw1", shift=dict(c=1))
    f("c-shift2", "rowstream<3,vec,none,8>/sw1", shift=dict(c=2))
    AT, RS = "atb<4,4>+reduce<16> | ", "rowstream<8,vec,bits,3>/sw4"

    def g(why, name, m=2049, n=128, p=41, ld=None, shift=None, **kw):
        P[f"class-bwd-no-{why}"] = _row("bwd_ex", m, n, p, name, ld=dict(dict(dc=48, wpr=cdiv(n, 32)), **(ld or {})), shift=shift,
                                        mask=kw.pop("mask", "bits"), rowscale=True, **kw)
    g("m2047", "atb<4,4>+reduce<64> | " + RS, m=2047)
    g("p65", "atb<4,4>+reduce<16> | rowstream<8,vec,bits,0>/sw4", p=65, ld=dict(dc=80))
    g("n132", "atb<4,4>+reduce<16> | rowstream<8,vec,bits,3>/sw4/y>1", n=132)
    g("wpr5", AT + RS, ld=dict(wpr=5))
    g("lddc44", AT + RS, ld=dict(dc=44))
    g("lddc50", "atb<4,2>+reduce<16> | rowstream<8,scalar,bits,3>/staged", ld=dict(dc=50))
    g("ldda130", AT + "rowstream<8,vec,bits,3>/sw1", ld=dict(da=130))
    g("dc-shift2", "atb<4,2>+reduce<16> | rowstream<8,scalar,bits,3>/staged", shift=dict(dc=2))
    g("da-shift1", AT + "rowstream<8,vec,bits,3>/sw1", shift=dict(da=1))
    g("bits-shift1", AT + RS, shift=dict(bits=1))
    g("bits-shift2", AT + RS, shift=dict(bits=2))
    g("no-db", RS, db=False)
    g("no-bits", AT + "rowstream<8,vec,H,3>/sw4", mask="H")
    # ---- m == 0: db is zeroed row by row, da is not touched
    for entry in ENTRIES:
        P[f"empty-{entry}"] = _row(entry, 0, 48, 41, "zero_rows" if entry not in ("fwd", "bwd_da_bits") else "", ld=dict(db=45))
    P["empty-bwd-no-db"] = _row("bwd", 0, 48, 41, "", db=False)
    P["empty-bwd_ex-H"] = _row("bwd_ex", 0, 48, 41, "zero_rows", mask="H")
    # ---- refusals: -1, nothing launched
    P["refused-fwd-K304"] = _row("fwd", 17, 304, 65, "refused")
    P["refused-fwd-K288-staged"] = _row("fwd", 17, 288, 65, "refused", ld=dict(a=289))
    for entry in ENTRIES[1:]:
        P[f"refused-{entry}-K304"] = _row(entry, 17, 65, 304, "refused", ld=dict(a=68))      # (the weight gradient alone would run)
        if entry != "bwd_da_bits":
            P[f"refused-{entry}-lda"] = _row(entry, 17, 48, 41, "refused", ld=dict(a=47), mask="H" if entry == "bwd_ex" else None)
        if MASK_OF[entry] in ("bits", None):
            P[f"refused-{entry}-wpr"] = _row(entry, 17, 48, 41, "refused", ld=dict(wpr=1))
    P["refused-fwd-lda"] = _row("fwd", 17, 48, 41, "refused", ld=dict(a=47))
    P["refused-bwd_ex-scale0"] = _row("bwd_ex", 17, 48, 41, "refused", scale=0.0)
    P["refused-bwd_ex-scale-nan"] = _row("bwd_ex", 17, 48, 41, "refused", scale=float("nan"))
    P["refused-bwd_ex-scale-neg"] = _row("bwd_ex", 17, 48, 41, "refused", scale=-1.0)
    P["refused-bwd_fused_bits-no-bits"] = _row("bwd_fused_bits", 17, 48, 41, "refused", mask="none")
    return P


PATHS = _paths()
