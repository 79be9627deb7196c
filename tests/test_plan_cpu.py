"""The host planning of the adjacency and feature objects (csrc/plan.h) without a GPU: tests/plan_check.cpp, a program
of its own built with g++ under AddressSanitizer and UBSan, plans the irregular graph and feature matrices of
irregular_inputs.py, and every plan is compared for exact equality with the numpy statement of the same rule in plan_ref.py.
These rules fix the summation order of every aggregation and weight gradient."""
import os
import subprocess

import numpy as np
import pytest

from tests import irregular_inputs as ii
from tests import plan_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_GRAPH = 300
SPLITS = {"by_size": 0, "forced_16": 16, "forced_1024": 1024}       # the hub row (2 500 stored edges) is cut at each
MODES = {"by_size": (0, 0), "forced_16": (1, 0), "forced_1024": (2, 7)}      # (schedule mode, n_groups): every mode once


def write_arrays(path, arrays):
    with open(path, "wb") as fp:
        for a in arrays:
            a = np.ascontiguousarray(a)
            assert a.dtype.itemsize == 4
            np.array([a.size], np.int32).tofile(fp)
            a.tofile(fp)


def read_arrays(path):
    words = np.fromfile(path, np.int32)
    out, at = [], 0
    while at < words.size:
        n = int(words[at])
        out.append(words[at + 1:at + 1 + n])
        at += 1 + n
    assert at == words.size
    return out


def pack_bits(flags):
    bits = np.packbits(np.asarray(flags, bool), bitorder="little")
    return np.concatenate([bits, np.zeros((-bits.size) % 4 + 4, np.uint8)]).view(np.uint32)


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    """run(mode, arrays) -> the arrays the program wrote; built once, with the sanitizers, nothing loaded into Python"""
    d = tmp_path_factory.mktemp("plan_check")
    exe = str(d / "plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "plan_check.cpp"), "-o", exe, "-pthread"], check=True)
    count = [0]

    def run(mode, arrays):
        count[0] += 1
        fin, fout = str(d / f"in{count[0]}.bin"), str(d / f"out{count[0]}.bin")
        write_arrays(fin, arrays)
        r = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return read_arrays(fout)
    return run


@pytest.fixture(scope="module")
def graph_inputs():
    rng = np.random.default_rng(ii.SEED_GRAPH)
    gp, gi = ii.irregular_graph(rng, N_GRAPH)
    assert int(np.diff(gp).max()) == 2500
    return dict(gp=gp, gi=gi, group=rng.integers(0, 5, N_GRAPH).astype(np.int32), rows=rng.random(N_GRAPH) < 0.4,
                cols=rng.random(N_GRAPH) < 0.5, cf=rng.standard_normal(gi.size).astype(np.float32))


@pytest.fixture(scope="module", params=sorted(SPLITS))
def graph_plan(request, plan_check, graph_inputs):
    """the C++ plan of the 300-node irregular graph at one split length, with the reference's row order and task list"""
    g = graph_inputs
    forced = SPLITS[request.param]
    mode, n_groups = MODES[request.param]
    rows = g["rows"].copy()
    rows[0] = True                                                  # the hub: the subset has a split row
    out = plan_check("graph", [np.array([N_GRAPH, N_GRAPH, forced, mode, n_groups, 5], np.int32), g["gp"], g["gi"],
                               np.zeros(0, np.int32), g["group"] if mode == 1 else np.zeros(0, np.int32),
                               pack_bits(rows), pack_bits(g["cols"]), g["cf"].view(np.int32)])
    names = ("valid one many lengths order tasks split n_slots bounds sub_tasks sub_split sub_n_slots sub_bounds recovered "
             "r_indptr r_indices r_coef").split()
    assert len(out) == len(names)
    p = dict(zip(names, out))
    for k in ("tasks", "split", "sub_tasks", "sub_split"):
        p[k] = p[k].reshape(-1, 4)
    key = {0: None, 1: g["group"], 2: plan_ref.dealt_key(g["gp"], max(n_groups, 1))}[mode]
    p.update(seg=plan_ref.split_length(int(g["gp"][-1]), forced), forced=forced, rows=rows, ref_order=plan_ref.row_order(g["gp"], key))
    return p


def test_split_length_and_threads(graph_plan):
    p = graph_plan
    seg, seg_large, thr_small, thr_large = p["lengths"][:4].tolist()
    assert seg == p["seg"] == {0: 128, 16: 16, 1024: 1024}[p["forced"]]
    assert seg_large == (p["forced"] or 1024)
    assert thr_small == 1 and 1 <= thr_large <= 16                  # one thread below 2^20 edges, at most 16 above
    by_size = [plan_ref.split_length(n) for n in (0, 128 * 8192 - 1, 256 * 8192 - 1, 256 * 8192, 512 * 8192, 1024 * 8192)]
    assert p["lengths"][4:].tolist() == by_size == [128, 128, 128, 256, 512, 1024]


def test_neighbour_sort(graph_plan, graph_inputs):
    g, p = graph_inputs, graph_plan
    assert p["valid"][0] == 1
    assert np.array_equal(p["one"], plan_ref.neighbour_order(g["gp"], g["gi"]))
    assert np.array_equal(p["one"], p["many"])                      # 1 thread and 5


def test_row_order_and_recovery(graph_plan):
    p = graph_plan
    assert np.array_equal(p["order"], p["ref_order"])
    assert np.array_equal(p["recovered"], p["order"])               # the order a child object rebuilds its tasks from


def test_tasks_cover_every_edge_once(graph_plan, graph_inputs):
    p, gp = graph_plan, graph_inputs["gp"].astype(np.int64)
    tasks, split, n_slots = plan_ref.cut_segments(gp, p["ref_order"], p["seg"])
    assert np.array_equal(p["tasks"], tasks) and np.array_equal(p["split"], split) and p["n_slots"][0] == n_slots
    t = p["tasks"].astype(np.int64)
    assert split.shape[0] >= 1 and np.all(t[:, 2] - t[:, 1] <= p["seg"])
    # the tasks of a row, in task order, are its stored edges once each in stored order
    covered = np.concatenate([np.arange(a, b) for a, b in t[:, 1:3]])
    by_row = np.concatenate([np.arange(gp[r], gp[r + 1]) for r in p["order"]])
    assert np.array_equal(covered, by_row) and covered.size == gp[-1]
    # slots: consecutive inside a split row, numbered without gaps over the list
    slots = t[t[:, 3] >= 0, 3]
    assert np.array_equal(slots, np.arange(n_slots))
    for r, first, ns, _ in p["split"].tolist():
        mine = t[t[:, 0] == r]
        assert np.array_equal(mine[:, 3], first + np.arange(ns)) and mine[0, 1] == gp[r] and mine[-1, 2] == gp[r + 1]


def test_xcd_bounds(graph_plan):
    p = graph_plan
    for tasks, bounds in ((p["tasks"], p["bounds"]), (p["sub_tasks"], p["sub_bounds"])):
        n = tasks.shape[0]
        b = bounds.reshape(4, 9)
        assert np.array_equal(b, plan_ref.xcd_bounds(tasks))
        assert np.all(np.diff(b, axis=1) >= 0) and np.all((b % 4 == 0) | (b == n)) and np.all(b[:, 8] == n) and np.all(b[:, 0] == 0)
        for lg in range(4):
            assert np.all(b[lg, 1 << lg:] == n)


def test_rowset_is_the_full_list_filtered(graph_plan):
    p = graph_plan
    assert np.array_equal(p["sub_tasks"], p["tasks"][p["rows"][p["tasks"][:, 0]]])
    assert np.array_equal(p["sub_split"], p["split"][p["rows"][p["split"][:, 0]]])
    assert p["sub_split"].shape[0] >= 1 and 0 < p["sub_tasks"].shape[0] < p["tasks"].shape[0]


def test_restriction_keeps_edges_in_order(graph_plan, graph_inputs):
    g, p = graph_inputs, graph_plan
    keep = g["cols"][p["one"]]
    row_of = np.repeat(np.arange(N_GRAPH), np.diff(g["gp"]))
    ip = np.concatenate([[0], np.cumsum(np.bincount(row_of[keep], minlength=N_GRAPH))]).astype(np.int32)
    assert np.array_equal(p["r_indptr"], ip) and 0 < ip[-1] < g["gi"].size
    assert np.array_equal(p["r_indices"], p["one"][keep])
    assert np.array_equal(p["r_coef"], g["cf"].view(np.int32)[keep])


def test_invalid_arrays_are_refused(plan_check, graph_inputs):
    g = graph_inputs
    tail = [np.zeros(0, np.int32)] * 2 + [pack_bits(g["rows"]), pack_bits(g["cols"]), g["cf"].view(np.int32)]
    head = np.array([N_GRAPH, N_GRAPH, 0, 0, 0, 1], np.int32)
    for bad in (-1, N_GRAPH):
        gi = g["gi"].copy()
        gi[gi.size // 2] = bad
        assert plan_check("graph", [head, g["gp"], gi] + tail)[0][0] == 0
    gp = g["gp"].copy()
    gp[5] = gp[6] + 1                                               # a row pointer that goes back
    assert plan_check("graph", [head, gp, g["gi"]] + tail)[0][0] == 0


@pytest.mark.parametrize("forced", [0, 16])
@pytest.mark.parametrize("case", sorted(ii.FEATURE_CASES))
def test_feature_plan(plan_check, case, forced):
    fp, fi, fv, F = ii.gpu_features(case)
    n = fp.size - 1
    out = plan_check("feat", [np.array([n, F, forced], np.int32), fp, fi])
    assert out[0].tolist() == [0, 1] and len(out) == 8
    ptr, row, pos, (nw, seg), tasks, split, (n_slots,) = out[1:]
    # CSC: a permutation of the entries, columns ascending, rows ascending inside every column (a stable sort by column)
    ref_pos = np.argsort(fi, kind="stable").astype(np.int32)
    row_of = np.repeat(np.arange(n), np.diff(fp)).astype(np.int32)
    assert np.array_equal(ptr, np.concatenate([[0], np.cumsum(np.bincount(fi, minlength=F))]))
    assert np.array_equal(np.sort(pos), np.arange(fi.size)) and np.array_equal(pos, ref_pos) and np.array_equal(row, row_of[pos])
    for k in range(F):
        assert np.all(fi[pos[ptr[k]:ptr[k + 1]]] == k) and np.all(np.diff(row[ptr[k]:ptr[k + 1]]) >= 0)
    # the weight gradient's tasks: waves by mean column length, columns beyond the segment length cut by the rows' cutter
    mean = fi.size / F
    assert nw == (forced or (1 if mean <= 128 else 4 if mean <= 1024 else 16)) and seg == max(1024, nw * 256)
    ref_tasks, ref_split, ref_slots = plan_ref.cut_segments(ptr, np.arange(F), seg)
    assert np.array_equal(tasks.reshape(-1, 4), ref_tasks) and np.array_equal(split.reshape(-1, 4), ref_split) and n_slots == ref_slots
    longest = int(np.diff(ptr).max())
    assert (ref_split.shape[0] >= 1) == (longest > seg)
    if case == "long":
        assert longest > 4096 and seg == (4096 if forced else 1024) and ref_split.shape[0] == 1


def test_dense_layout(plan_check):
    rng = np.random.default_rng(ii.SEED_FEAT)
    n, F = 12, 9
    fp, fi, _, _ = ii.permuted_full_features(rng, n, F)
    head = np.array([n, F, 0], np.int32)
    assert plan_check("feat", [head, fp, fi])[0][0] == 0            # nnz == n.F, one row a permutation: NOT dense
    ident = np.tile(np.arange(F, dtype=np.int32), n)
    assert plan_check("feat", [head, fp, ident])[0][0] == 1
    assert plan_check("feat", [head, fp, np.zeros(0, np.int32)])[0][0] == 1         # no index array: the caller asserts the layout
    short = fp.copy()
    short[-1] -= 1
    assert plan_check("feat", [head, short, ident[:-1]])[0][0] == 0
    assert plan_check("feat", [head, fp, np.where(ident == F - 1, F, ident)])[0].tolist() == [0, 0]    # an id past the last column
