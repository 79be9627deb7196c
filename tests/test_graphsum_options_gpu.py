"""Every GraphSum option against every other, inside one launch, on every kernel path: the launch record (GsCall,
csrc/graphsum.hip) as a table of accepted and refused combinations, held to the float64 restatement in tests/graphsum_ref.py
(proved on the CPU by test_graphsum_options_cpu.py).

Graph: graphsum_ref.planted_graph — 400 nodes, twelve hubs of exact degree wired to leaves only.  It is built on three
devices: split_edges = 16 (rows of 2 .. 10 and 19 segments: every tail length of gs_segment_sum, with and without a full
batch of four); split_edges left at 0, where plan::split_length gives this small graph its floor of 128 edges, so the hubs of
degree 129, 145 and 300 are still cut (2, 2 and 3 segments); and split_edges = 4096, where nothing is split and the finalize
launch is off.

PATHS names the kernel each (dim, ld, gs_l) reaches; gate() restates the choice of graphsum_impl and the table is checked
against it.  Per path the inner loop runs rows {all, two registered subsets, two sets of output-row bits} x input-row bits x
accumulate x scaling 0-3 x epilogue {none, ReLU, keep mask, Philox at three offsets, Philox + mask words}, then the
epilogues again through two restricted operators that share `out`; refusals() lists what graphsum_impl turns away.
Output-row bits are carried by gcnhip_graphsum_masked alone, which takes input-row bits beside them and nothing else, so
that is the only pairing they appear in.

Checks per accepted case: touched rows within test_ops_gpu.close_mag, k = 8, of float64; every other float of `out`
(untouched rows, padding columns) keeps its bits; mask words == packbits(out > 0) on the stored values, untouched words keep
their fill.  Bit identities: all rows / subset / output-row bits; gcnhip_graphsum_part and the plain entry points against
gcnhip_graphsum_ex; schedule modes 0 / 1 / 2; a clone; gs_l = 4 with mask words against gs_l = 0; gs_u 1 / 2 / 4 (vector
kernel, predict, blend) — the order of additions is the same in all of them, and on an MI355X they do agree bit for bit.

Measured on an MI355X: every case is inside k = 8 as it stands (no row needed the reference's own sequential f32 sum);
the file: 128 cases in 12 s, the slowest 0.36 s.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests.graphsum_ref import HUB_DEGREES, SPLIT, dinv_f32, graphsum_ref, keep_decisions, pack_positive, planted_graph, planted_row_sets, segments
from tests.test_ops_gpu import bf16_round, close_mag

pytestmark = pytest.mark.gpu

SEED, EPOCH = 0xabcdef12345, 3
BITS_FILL = 0xDEADBEEF

# id -> (dim, ld, gs_l, (kernel, L, column slices or passes) as gate() must give it)
PATHS = {
    "scalar-L1": (1, 1, 0, ("scalar", 1, 1)), "scalar-L4": (3, 3, 0, ("scalar", 4, 1)), "scalar-L32": (29, 29, 0, ("scalar", 32, 1)),
    "scalar-L64-41": (41, 41, 0, ("scalar", 64, 1)), "scalar-L64-70": (70, 70, 0, ("scalar", 64, 1)),
    "scalar-L64-two-passes": (300, 301, 0, ("scalar", 64, 2)),
    "vec-L1": (3, 4, 0, ("vec", 1, 1)), "vec-L2": (7, 8, 0, ("vec", 2, 1)), "vec-L4": (16, 16, 0, ("vec", 4, 1)),
    "vec-L8": (31, 32, 0, ("vec", 8, 1)), "vec-L16-41": (41, 44, 0, ("vec", 16, 1)), "vec-L16-60": (60, 64, 0, ("vec", 16, 1)),
    "vec-L32": (100, 100, 0, ("vec", 32, 1)), "vec-L64-200": (200, 200, 0, ("vec", 64, 1)), "vec-L64-260": (260, 260, 0, ("vec", 64, 2)),
    "slices64-64": (64, 64, 0, ("vec", 16, 1)), "slices64-128": (128, 128, 0, ("vec", 16, 2)), "slices64-256": (256, 256, 0, ("vec", 16, 4)),
    "gl8-64": (64, 64, 8, ("vec", 8, 2)), "gl8-128": (128, 128, 8, ("vec", 8, 4)), "gl8-256": (256, 256, 8, ("vec", 8, 8)),
    "gl4-32": (32, 32, 4, ("vec", 4, 2)), "gl4-64": (64, 64, 4, ("vec", 4, 4)), "gl4-128": (128, 128, 4, ("vec", 4, 8)),
}
BF16_PATHS = {
    "bf16-L1": (7, 8, ("bf16", 1, 1)), "bf16-L2": (16, 16, ("bf16", 2, 1)), "bf16-L4": (31, 32, ("bf16", 4, 1)),
    "bf16-L8": (41, 48, ("bf16", 8, 1)), "bf16-L16": (128, 128, ("bf16", 16, 1)), "bf16-L8-sliced": (200, 208, ("bf16", 8, 4)),
}
VEC_PATHS = [k for k, v in PATHS.items() if v[3][0] == "vec"]


def gate(dim, ld, gs_l=0, pos_bits=False, bf16=False):
    """the kernel graphsum_impl launches, as a pure function: (kernel, lanes per row slice, column slices bound to XCD groups
    — or column passes of the scalar kernel)"""
    cdiv = lambda a, b: -(-a // b)
    sliced = lambda chunks: chunks if chunks > 1 and 8 % chunks == 0 else 1
    if bf16:
        d8 = cdiv(dim, 8)
        L = 1 if d8 <= 1 else 2 if d8 <= 2 else 4 if d8 <= 4 else 16 if d8 % 16 == 0 else 8
        return "bf16", L, sliced(cdiv(dim, L * 8))
    if ld % 4 == 0:
        if (gs_l == 8 or (gs_l == 4 and not pos_bits)) and dim % (gs_l * 4) == 0 and dim // (gs_l * 4) > 1 and 8 % (dim // (gs_l * 4)) == 0:
            return "vec", gs_l, dim // (gs_l * 4)
        if dim % 64 == 0 and 8 % (dim // 64) == 0:
            return "vec", 16, sliced(dim // 64)
        d4 = cdiv(dim, 4)
        L = next(l for l in (1, 2, 4, 8, 16, 32, 64) if d4 <= l or l == 64)
        return "vec", L, sliced(cdiv(dim, L * 4))
    L = next(l for l in (1, 2, 4, 8, 16, 32, 64) if dim <= l or l == 64)
    return "scalar", L, cdiv(dim, L * 4)


def test_the_table_names_the_path_the_gate_takes():
    for dim, ld, gl, want in PATHS.values():
        assert gate(dim, ld, gl) == want, (dim, ld, gl)
    for dim, ld, want in BF16_PATHS.values():
        assert gate(dim, ld, bf16=True) == want, (dim, ld)
    kinds = {v[3][:2] for v in PATHS.values()} | {v[2][:2] for v in BF16_PATHS.values()}
    assert {("scalar", l) for l in (1, 4, 32, 64)} <= kinds and {("vec", l) for l in (1, 2, 4, 8, 16, 32, 64)} <= kinds
    assert {("bf16", l) for l in (1, 2, 4, 8, 16)} <= kinds
    for dim in (32, 64, 128):                                # 16-float slices hold half a mask word: with pos_bits the launch is gs_l = 0's
        assert gate(dim, dim, 4, pos_bits=True) == gate(dim, dim, 0, pos_bits=True)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


class World:
    """one device with the planted graph on it, its row subsets and the masks that stay resident"""

    def __init__(self, split):
        from cuda_gcn_amd.ops import Device
        self.split = split
        self.dev = Device(0)
        if split:
            self.dev.set_option("split_edges", split)
        self.gp, self.gi, self.hubs = planted_graph()
        self.n = self.gp.size - 1
        self.g = self.dev.graph(self.gp, self.gi)
        ns = segments(self.gp, SPLIT)
        assert set(range(1, 10)) <= set(ns.tolist()) and tuple(np.diff(self.gp)[self.hubs]) == HUB_DEGREES
        assert sorted(segments(self.gp, 128)[self.hubs][-3:]) == [2, 2, 3] and segments(self.gp, 4096).max() == 1
        dr, dr2 = self.g.scales()[:2]
        assert np.array_equal(dr, dinv_f32(self.gp)[0]) and np.array_equal(dr2, dinv_f32(self.gp)[1])
        a, b, self.nz = planted_row_sets(self.gp, self.hubs)
        self.row_sets = {"A": a, "B": b}
        self.rs = {k: self.g.add_rowset(v) for k, v in self.row_sets.items()}
        self.ob = {k: self.dev._bits(v) for k, v in self.row_sets.items()}
        self.nz_bits = self.dev._bits(self.nz)
        self.cache = {}

    def close(self):
        self.g.free()
        self.dev.close()


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(split):
        if split not in made:
            made[split] = World(split)
        return made[split]
    yield get
    for w in made.values():
        w.close()


class Operands:
    """the inputs of one path, uploaded once: x (padding columns NaN), x with NaN in the rows the input bits switch off, prev,
    the keep mask and the Philox decisions of every epilogue"""

    def __init__(self, w, dim, ld, bf16=False):
        self.dim, self.ld = dim, ld
        n = w.n
        rng = np.random.default_rng(1000 + dim)
        x = rng.standard_normal((n, dim)).astype(np.float32)
        self.codes = None
        if bf16:
            self.codes, x = bf16_round(x)
        self.x = x
        self.xn = np.where(w.nz[:, None], x, np.nan).astype(np.float32)
        self.prev = rng.standard_normal((n, dim)).astype(np.float32)
        self.km = (rng.random((n, dim)) < 0.6).astype(np.uint8)
        pad = lambda a: np.concatenate([a, np.full((n, ld - dim), np.nan, np.float32)], axis=1)
        self.host = {0: np.full((n, ld), np.nan, np.float32), 1: pad(self.prev)}      # what `out` holds before a call, by accumulate
        if not bf16:
            self.d_x, self.d_xn = w.dev.buf(pad(x)), w.dev.buf(pad(self.xn))
            self.d_km = w.dev.buf(self.km)
            self.d_out = w.dev.buf((n, ld))
            self.wpr = (dim + 31) // 32
            self.d_bits = w.dev.buf((n, self.wpr), np.uint32)
            self.bits_fill = np.full((n, self.wpr), BITS_FILL, np.uint32)
        self.keep = {}

    def decisions(self, ep):
        """bool [n, dim] keep decisions of an epilogue (None: no dropout)"""
        if not ep.get("training"):
            return None
        key = (ep["p"], ep.get("elem_offset"), "keep_mask" in ep)
        if key not in self.keep:
            self.keep[key] = keep_decisions(self.x.shape[0], self.dim, 1, ep["p"], SEED, EPOCH, ep.get("elem_offset", 0),
                                            self.km if "keep_mask" in ep else None)
        return self.keep[key]


def epilogues(dim, vec, extra_p=False):
    e = {"none": {}, "relu": dict(relu_dropout=1), "mask": dict(relu_dropout=1, training=1, p=0.3, keep_mask=True),
         "philox@0": dict(relu_dropout=1, training=1, p=0.3, elem_offset=0),
         "philox@4004": dict(relu_dropout=1, training=1, p=0.3, elem_offset=4 * 1001),
         "philox@77": dict(relu_dropout=1, training=1, p=0.3, elem_offset=77)}
    if vec and dim % 32 == 0:
        e["philox+bits"] = dict(relu_dropout=1, training=1, p=0.3, elem_offset=4 * 1001, want_bits=True)
        e["relu+bits"] = dict(relu_dropout=1, want_bits=True)
    if extra_p:
        e["philox p=0.5"] = dict(relu_dropout=1, training=1, p=0.5, elem_offset=77)
    return e


def launch(w, P, g, rs, rows, inb, acc, scaling, ep, entry="ex", host=None):
    """one call on resident operands -> (the whole out buffer [n, ld], mask words or None); host: what `out` holds before it"""
    host = P.host[acc] if host is None else host
    P.d_out.upload(host)
    kw = dict(dim=P.dim, out=P.d_out, accumulate=acc, row_nonzero=w.nz_bits if inb else None)
    if rows in ("A", "B"):
        kw["rows"] = rs[rows]
    for k in ("relu_dropout", "training", "p", "elem_offset"):
        if k in ep:
            kw[k] = ep[k]
    if ep.get("training"):
        kw.update(seed=SEED, epoch=EPOCH)
    if "keep_mask" in ep:
        kw["keep_mask"] = P.d_km
    x = P.d_xn if inb else P.d_x
    if entry == "part":
        w.dev.graphsum_part(g, x, **kw)
        return P.d_out.download(), None
    if rows in ("obA", "obB"):
        kw["out_rows"] = w.ob[rows[2]]
    if ep.get("want_bits"):
        P.d_bits.upload(P.bits_fill)
        kw["bits"] = P.d_bits
    w.dev.graphsum_ex(g, x, scaling, **kw)
    return P.d_out.download(), (P.d_bits.download() if ep.get("want_bits") else None)


def reference(w, P, rows, inb, acc, scaling, ep, keep_cols=None, prev=None):
    sel = w.row_sets[rows[-1]] if rows != "all" else None
    return graphsum_ref(w.gp, w.gi, P.x, rows=sel if rows in ("A", "B") else None, out_row_bits=sel if rows in ("obA", "obB") else None,
                        in_row_bits=w.nz if inb else None, accumulate=acc, prev=P.prev if prev is None else prev, scaling=scaling,
                        keep_cols=keep_cols,
                        relu_dropout=ep.get("relu_dropout", 0), training=ep.get("training", 0), p=ep.get("p", 0.0), keep=P.decisions(ep),
                        cache=w.cache, x_key=(P.dim, P.codes is not None))


def check(w, P, out, bits, ref, acc, what, host=None):
    """assertions 1-3 of one accepted case"""
    want, mag, touched = ref
    host = P.host[acc] if host is None else host
    dim = P.dim
    try:
        close_mag(out[touched, :dim], want[touched], mag[touched])
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None
    keep = np.ones(out.shape, bool)
    keep[touched, :dim] = False
    assert np.array_equal(u32(out)[keep], u32(host)[keep]), f"{what}: a float outside the touched rows' columns changed"
    if bits is not None:
        assert np.array_equal(bits[touched], pack_positive(out[:, :dim])[touched]), f"{what}: mask words != (out > 0)"
        assert np.all(bits[~touched] == BITS_FILL), f"{what}: mask words of untouched rows written"


def cases(vec, dim, extra_p=False):
    """(rows, input-row bits, accumulate, scaling, epilogue name, epilogue) of every accepted combination, `all` rows first"""
    eps = epilogues(dim, vec, extra_p)
    for rows, inb, acc, scaling, (en, ep) in itertools.product(("all", "A", "B"), (0, 1), (0, 1), (0, 1, 2, 3) if vec else (0,), eps.items()):
        yield rows, inb, acc, scaling, en, ep
    for rows, inb in itertools.product(("obA", "obB"), (0, 1)):
        yield rows, inb, 0, 0, "none", eps["none"]


PROBES = [("all", 0, 0, 0, "none"), ("A", 1, 1, 1, "philox@77"), ("B", 0, 1, 2, "philox+bits"), ("all", 1, 0, 3, "relu"), ("A", 0, 0, 0, "mask")]


def probe(w, P, g, rs, vec):
    """a handful of combinations on adjacency object g, for the identities between objects and schedules"""
    eps = epilogues(P.dim, vec)
    res = []
    for rows, inb, acc, scaling, en in PROBES:
        ep = eps.get(en, eps["philox@77"])
        out, bits = launch(w, P, g, rs, rows, inb, acc, scaling if vec else 0, ep)
        res.append(u32(out))
        if bits is not None:
            res.append(bits)
    return res


@pytest.mark.parametrize("split", [16, 0, 4096])
@pytest.mark.parametrize("path", list(PATHS))
def test_every_option_combination(worlds, split, path):
    w = worlds(split)
    dev, g = w.dev, w.g
    dim, ld, gl, want_gate = PATHS[path]
    vec = want_gate[0] == "vec"
    assert gate(dim, ld, gl) == want_gate
    P = Operands(w, dim, ld)
    g.reserve(dim)
    eps = epilogues(dim, vec)
    dev.set_option("gs_l", gl)
    try:
        full = {}
        for rows, inb, acc, scaling, en, ep in cases(vec, dim, extra_p=path == "vec-L4"):
            what = f"{path} split={split} rows={rows} in_bits={inb} accumulate={acc} scaling={scaling} epilogue={en}"
            out, bits = launch(w, P, g, w.rs, rows, inb, acc, scaling, ep)
            ref = reference(w, P, rows, inb, acc, scaling, ep)
            check(w, P, out, bits, ref, acc, what)
            touched = ref[2]
            key = (inb, acc, scaling, en)
            if rows == "all":
                full[key] = (out, bits)
            else:                                            # subset / output-row bits: the bits of the all-rows call on the touched rows
                assert np.array_equal(u32(out)[touched], u32(full[key][0])[touched]), f"{what}: differs from the all-rows call"
                if bits is not None:
                    assert np.array_equal(bits[touched], full[key][1][touched]), f"{what}: mask words differ from the all-rows call"
            if rows in ("obA", "obB"):                       # ... and of the registered subset with the same rows
                sub, _ = launch(w, P, g, w.rs, rows[2], inb, 0, 0, ep)
                assert np.array_equal(u32(sub), u32(out)), f"{what}: output-row bits differ from the registered subset"
            elif scaling == 0 and bits is None:              # gcnhip_graphsum_part carries these fields too
                part, _ = launch(w, P, g, w.rs, rows, inb, acc, 0, ep, entry="part")
                assert np.array_equal(u32(part), u32(out)), f"{what}: gcnhip_graphsum_part differs from gcnhip_graphsum_ex"
            if gl == 4 and bits is not None:                 # fell back to the 64-float slices: gs_l = 0's bits
                dev.set_option("gs_l", 0)
                o0, b0 = launch(w, P, g, w.rs, rows, inb, acc, scaling, ep)
                dev.set_option("gs_l", gl)
                assert np.array_equal(u32(o0), u32(out)) and np.array_equal(b0, bits), f"{what}: not the launch of gs_l = 0"
        # the plain entry points carry a subset of the fields: same bits as gcnhip_graphsum_ex with those fields
        f = lambda a: u32(a[:, :dim])
        assert np.array_equal(u32(dev.graphsum(g, P.x, ld_in=ld, ld_out=ld)), f(full[(0, 0, 0, "none")][0]))
        assert np.array_equal(u32(dev.graphsum(g, P.xn, ld_in=ld, ld_out=ld, row_nonzero=w.nz)), f(full[(1, 0, 0, "none")][0]))
        assert np.array_equal(u32(dev.graphsum_masked(g, P.xn, ld_in=ld, ld_out=ld, row_nonzero=w.nz)), f(full[(1, 0, 0, "none")][0]))
        a = w.row_sets["A"]
        got = dev.graphsum_rowset(g, w.rs["A"], P.xn, ld_in=ld, ld_out=ld, row_nonzero=w.nz)
        assert np.array_equal(u32(got)[a], f(full[(1, 0, 0, "none")][0])[a]) and np.isnan(got[~a]).all()
        got = dev.graphsum_relu_dropout(g, P.x, training=True, p=0.3, seed=SEED, epoch=EPOCH, elem_offset=77, ld=ld)
        assert np.array_equal(u32(got), f(full[(0, 0, 0, "philox@77")][0]))
        got = dev.graphsum_relu_dropout(g, P.x, training=False, p=0.3, ld=ld)
        assert np.array_equal(u32(got), f(full[(0, 0, 0, "relu")][0]))
        if "philox+bits" in eps:
            got, gb = dev.graphsum_relu_dropout_bits(g, P.x, training=True, p=0.3, seed=SEED, epoch=EPOCH, elem_offset=4 * 1001, ld=ld)
            assert np.array_equal(u32(got), f(full[(0, 0, 0, "philox+bits")][0])) and np.array_equal(gb, full[(0, 0, 0, "philox+bits")][1])
        # schedule modes and a clone change the task list and the segment slots, never the order inside a row
        base = probe(w, P, g, w.rs, vec)
        for mode in (1, 2):
            g.set_schedule(mode, (np.arange(w.n) % 5).astype(np.int32) if mode == 1 else None, 0 if mode == 1 else 16)
            try:
                again = probe(w, P, g, w.rs, vec)
            finally:
                g.set_schedule(0)
            assert all(np.array_equal(p, q) for p, q in zip(base, again)), f"{path}: schedule mode {mode} changed bits"
        gc = g.clone()
        try:
            rs_c = {k: gc.add_rowset(v) for k, v in w.row_sets.items()}
            again = probe(w, P, gc, rs_c, vec)
        finally:
            gc.free()
        assert all(np.array_equal(p, q) for p, q in zip(base, again)), f"{path}: the clone's bits differ from its parent's"
        # two operators with complementary columns share the rows of `out`, the second adds to what the first left and
        # runs the epilogue: the hidden layer of a row-partitioned model (host/module.cpp)
        own = np.arange(w.n) % 2 == 0
        ga, gb = g.restricted(own), g.restricted(~own)
        try:
            first, _ = launch(w, P, ga, None, "all", 0, 0, 0, {}, entry="part")
            check(w, P, first, None, reference(w, P, "all", 0, 0, 0, {}, keep_cols=own), 0, f"{path} split={split}: own columns")
            for inb, (en, ep) in itertools.product((0, 1), eps.items()):
                if ep.get("want_bits"):
                    continue
                what = f"{path} split={split}: remote columns added, in_bits={inb} epilogue={en}"
                second, _ = launch(w, P, gb, None, "all", inb, 1, 0, ep, entry="part", host=first)
                check(w, P, second, None, reference(w, P, "all", inb, 1, 0, ep, keep_cols=~own, prev=first[:, :dim]), 1, what, host=first)
                again, _ = launch(w, P, gb, None, "all", inb, 1, 0, ep, host=first)
                assert np.array_equal(u32(again), u32(second)), f"{what}: gcnhip_graphsum_ex differs from gcnhip_graphsum_part"
        finally:
            ga.free(); gb.free()
    finally:
        dev.set_option("gs_l", 0)


@pytest.mark.parametrize("split", [16, 0, 4096])
@pytest.mark.parametrize("path", list(BF16_PATHS))
def test_every_option_combination_of_the_bf16_table(worlds, split, path):
    """what gcnhip_graphsum_bf16 exposes: a registered row subset, input-row bits, the ReLU/dropout epilogue"""
    w = worlds(split)
    dev, g = w.dev, w.g
    dim, ld, want_gate = BF16_PATHS[path]
    assert gate(dim, ld, bf16=True) == want_gate
    P = Operands(w, dim, dim, bf16=True)
    table = np.zeros((w.n, ld), np.uint16)
    table[:, :dim] = P.codes
    table_n = table.copy()
    table_n[~w.nz] = 0x7FC0                                  # NaN in the rows the input bits switch off
    full = {}
    for rows, inb, (en, ep) in itertools.product(("all", "A", "B"), (0, 1), epilogues(dim, False).items()):
        what = f"{path} split={split} rows={rows} in_bits={inb} epilogue={en}"
        rd = None
        if ep:
            rd = dict(training=ep.get("training", 0), p=ep.get("p", 0.0), seed=SEED, epoch=EPOCH, elem_offset=ep.get("elem_offset", 0),
                      keep_mask=P.km if "keep_mask" in ep else None)
        out = dev.graphsum_bf16(g, table_n if inb else table, dim, row_nonzero=w.nz if inb else None, relu_dropout=rd,
                                out_rows=w.rs[rows] if rows != "all" else None)
        ref = reference(w, P, rows, inb, 0, 0, ep)
        check(w, P, out, None, ref, 0, what)
        if rows == "all":
            full[(inb, en)] = out
        else:
            assert np.array_equal(u32(out)[ref[2]], u32(full[(inb, en)])[ref[2]]), f"{what}: differs from the all-rows call"


@pytest.mark.parametrize("split", [16, 0])
@pytest.mark.parametrize("path", VEC_PATHS)
def test_batch_depth_changes_no_bit(worlds, split, path):
    """gs_u = 1, 2, 4 row loads in flight (4 by default, 2 once the table passes the Infinity Cache): lane group g adds its
    edges g, g + G, ... in that order whatever the depth, so the three agree bit for bit — vector kernel, every form it is
    launched in; the prediction kernels (depth 2 or 4); the blend kernels (2 or 4).  Each is also held to float64."""
    w = worlds(split)
    dev, g = w.dev, w.g
    dim, ld, gl, _ = PATHS[path]
    P = Operands(w, dim, ld)
    g.reserve(dim)
    eps = epilogues(dim, True)
    combos = [(rows, inb, acc, scaling, en) for rows, inb, acc, scaling, en in
              itertools.product(("all", "A"), (0, 1), (0, 1), (0, 1), ("none", "philox+bits" if "philox+bits" in eps else "philox@77"))]
    got = {}
    dev.set_option("gs_l", gl)
    try:
        for u in (1, 2, 4):
            dev.set_option("gs_u", u)
            for rows, inb, acc, scaling, en in combos:
                out, bits = launch(w, P, g, w.rs, rows, inb, acc, scaling, eps[en])
                check(w, P, out, bits, reference(w, P, rows, inb, acc, scaling, eps[en]), acc, f"{path} gs_u={u} {rows} {inb} {acc} {scaling} {en}")
                got[(u, rows, inb, acc, scaling, en)] = (u32(out), bits)
            if dim <= 64 and gl == 0:
                for scaling, rs in itertools.product((0, 1), (None, w.rs["A"])):
                    r = dev.graphsum_predict(g, P.x, scaling=scaling, rows=rs, ld=ld)
                    got[(u, "predict", scaling, rs is None)] = (r["pred"], u32(r["prob"]), u32(r["logp"]), u32(r["logits"]))
                if u >= 2:
                    o, pred = dev.graphsum_blend(g, P.x, base=P.prev, alpha=0.8, beta=0.2, lo=-0.5, hi=0.75, ld=ld, argmax=True)
                    got[(u, "blend")] = (u32(o), pred)
    finally:
        dev.set_option("gs_u", 0)
        dev.set_option("gs_l", 0)
    for key, val in got.items():
        if key[0] == 4:
            continue
        ref = got[(4,) + key[1:]]
        assert all(a is b or np.array_equal(a, b) for a, b in zip(val, ref)), f"{path}: gs_u = {key[0]} and 4 differ at {key[1:]}"
    if dim <= 64 and gl == 0:                                # the predicted logits are the plain aggregation's
        assert np.array_equal(got[(4, "predict", 0, True)][3], got[(4, "all", 0, 0, 0, "none")][0][:, :dim])


# ---- what graphsum_impl and its entry points turn away: (name, call, words the detail text must hold or None) ------------
class RefusalBuffers:
    """operands wide enough that every call below would stay inside them if it were accepted: dim <= 100, ld <= 128"""

    def __init__(self, w):
        n = w.n
        self.x_host = np.random.default_rng(2).standard_normal((n, 128)).astype(np.float32)
        self.out_fill = np.full((n, 128), np.nan, np.float32)
        self.bits_fill = np.full((n, 4), BITS_FILL, np.uint32)
        self.x, self.out, self.bits = w.dev.buf(self.x_host), w.dev.buf(self.out_fill), w.dev.buf(self.bits_fill)
        self.i32, self.f32 = w.dev.buf(np.zeros(n, np.int32)), w.dev.buf(np.zeros((n, 128), np.float32))


def refusals(w, B, lib):
    from cuda_gcn_amd.ops import GsLoss, GsOpts
    dev, g = w.dev, w.g
    x, out, bits, i32, f32 = B.x.ptr, B.out.ptr, B.bits.ptr, B.i32.ptr, B.f32.ptr
    dim = ld = 64
    keepers = []

    def ex(ldi=ld, ldo=ld, d=dim, **f):
        o = GsOpts()
        for k, v in f.items():
            setattr(o, k, v)
        keepers.append(o)
        return lambda: lib.gcnhip_graphsum_ex(dev.ctx, g.h, C.byref(o), x, ldi, out, ldo, d)

    def loss(**f):
        lo = GsLoss()
        lo.truth, lo.grad, lo.ld_grad, lo.training, lo.count, lo.row_terms = i32, f32, 128, 1, 5, f32
        keepers.append(lo)
        return ex(loss=C.addressof(lo), **f)

    def predict(d=dim, ldi=ld, scaling=0, table=None):
        return lambda: lib.gcnhip_graphsum_predict(dev.ctx, g.h, None, None if table else x, table, ldi, out, max(ld, ldi), d, scaling, i32, f32, None, 0)

    def blend(d=dim, ldi=ld, o=out):
        return lambda: lib.gcnhip_graphsum_blend(dev.ctx, g.h, x, ldi, f32, ld, o, ld, d, 1.0, 0.0, -1.0, 1.0, None)
    other = g.clone()
    keepers.append(other)
    rs_other = other.add_rowset(w.row_sets["A"])
    rd = dict(relu_dropout=1, training=1)
    table = [
        ("scaling 4", ex(scaling=4), None), ("scaling -1", ex(scaling=-1), None),
        ("ld_in < dim", ex(ldi=dim - 4), None), ("ld_out < dim", ex(ldo=dim - 4), None), ("dim 0", ex(d=0), None),
        ("p = 1", ex(p=1.0, **rd), None), ("p < 0", ex(p=-0.1, **rd), None),
        ("mask words without the epilogue", ex(pos_bits=bits, words_per_row=2), None),
        ("mask words, dim % 32 != 0", ex(d=48, pos_bits=bits, words_per_row=2, relu_dropout=1), "dim % 32 == 0"),
        ("mask words, too few words per row", ex(pos_bits=bits, words_per_row=1, relu_dropout=1), "words_per_row"),
        ("mask words, rows not of 16 bytes", ex(ldi=ld + 1, d=32, pos_bits=bits, words_per_row=1, relu_dropout=1), "16-byte aligned"),
        ("scaling 1, rows not of 16 bytes", ex(ldi=ld + 1, scaling=1), "scaling != 0"),
        ("scaling 2, out rows not of 16 bytes", ex(ldo=ld + 2, d=32, scaling=2), "scaling != 0"),
        ("a subset of another object", ex(rows=rs_other.value), "another adjacency object"),
        ("loss + ReLU", loss(relu_dropout=1), "loss epilogue"), ("loss, dim > 64", loss(d=100, ldi=100, ldo=100), "loss epilogue"),
        ("loss, rows not of 16 bytes", loss(ldo=ld + 3, d=16), "loss epilogue"),
        ("predict, dim > 64", predict(d=100, ldi=100), "gcnhip_graphsum_predict"),
        ("predict, rows not of 16 bytes", predict(ldi=ld + 1), "gcnhip_graphsum_predict"),
        ("predict, bf16 table + scaling", predict(scaling=1, table=f32), "gcnhip_graphsum_predict"),
        ("blend, out == in", blend(o=x), "out must not be in"), ("blend, rows not of 16 bytes", blend(ldi=ld + 2, d=32), "16-byte aligned"),
        ("blend, dim 0", blend(d=0), "1 <= dim <= 64"), ("blend, dim > 64", blend(d=100, ldi=100), "1 <= dim <= 64"),
        ("bf16, ld % 8 != 0", lambda: lib.gcnhip_graphsum_bf16(dev.ctx, g.h, f32, 20, out, ld, 16, None, None, 0, 0, 0.0, 0, None, 0, None), None),
        ("bf16, p = 1", lambda: lib.gcnhip_graphsum_bf16(dev.ctx, g.h, f32, 64, out, ld, 64, None, None, 1, 1, 1.0, 0, None, 0, None), None),
        ("relu_dropout_bits without words",
         lambda: lib.gcnhip_graphsum_relu_dropout_bits(dev.ctx, g.h, x, ld, out, ld, dim, 0, 0.0, 0, None, 0, None, None, 2), None),
        ("part, p = 1", lambda: lib.gcnhip_graphsum_part(dev.ctx, g.h, None, x, ld, out, ld, dim, None, 0, 1, 1, 1.0, 0, None, 0, None), None),
        ("rowset without a subset", lambda: lib.gcnhip_graphsum_rowset(dev.ctx, g.h, None, x, ld, out, ld, dim, None), None),
    ]
    return table, keepers


def test_refused_combinations_touch_nothing(worlds):
    """each refused combination returns non-zero, names its reason where graphsum_impl gives one, and writes neither `out`
    nor the mask words (test_edge_cases_gpu.test_c_abi_rejects_bad_arguments holds the NULL operands and the scratch width)"""
    w = worlds(16)
    lib = w.dev.lib
    B = RefusalBuffers(w)
    table, keepers = refusals(w, B, lib)
    for name, call, words in table:
        lib.gcnhip_ctx_set_option(w.dev.ctx, b"no such option", 0)   # leaves its own detail text: a stale one cannot pass below
        rc = call()
        w.dev.sync()
        assert rc != 0, f"{name}: accepted"
        assert lib.gcnhip_error_string(rc), name
        if words:
            assert words in lib.gcnhip_last_error().decode(), f"{name}: detail text {lib.gcnhip_last_error().decode()!r}"
        assert np.isnan(B.out.download()).all(), f"{name}: out written"
        assert np.all(B.bits.download() == BITS_FILL), f"{name}: mask words written"
    assert np.array_equal(u32(B.x.download()), u32(B.x_host))
    P = Operands(w, 64, 64)
    out, _ = launch(w, P, w.g, w.rs, "all", 0, 0, 0, {})     # the context still works
    check(w, P, out, None, reference(w, P, "all", 0, 0, 0, {}), 0, "after the refusals")
    for k in keepers:
        if hasattr(k, "free"):
            k.free()
