"""The reach report on reddit-syn and on an R-MAT graph, HIP events and wall clocks — the figures of DESIGN §4.22:
  * gcnhip_hop_distance of csrc/reach.hip from the training split, without and with `nearest`: the whole call (it synchronises, so
    a wall clock around it is honest), the levels and the rows per level, and every level launch on its own (max_hops = L minus
    max_hops = L - 1, HIP events around the calls with levels_per_sync = 64);
  * the same call against gcnhip_nbr_agreement over every row of the same object — one walk over the same index stream — and
    against the byte floor of ONE pass over the row pointers and the indices at the HBM copy rate (6.29 TB/s); a traversal of L
    levels is allowed L such passes at most, and its later levels should cost far less than one;
  * gcnhip_components: rounds, the call and the time per round; gcnhip_component_counts and gcnhip_distance_strata;
  * the same traversal and components on datagen.rmat_graph(--rmat SCALE, default 18), a long-tailed degree distribution, from a
    random 1 % of the rows;
  * reach_report() as a whole (wall time) against scipy's breadth_first_order / connected_components on the host (the multi-source
    search as one search from a virtual node listed by every source's row: the transposed direction scipy needs is built outside
    the timed part);
  * with --parent DIR (a built checkout of the parent commit): `python bench.py --gpus 1 --steps 50 --warmup 10` in DIR and here,
    alternating --rounds times (default 3): the epoch path is meant not to move.
Prints one JSON line, with the hashes of the sources it measured (cuda_gcn_amd/provenance.py); --out FILE also writes it there.
None of the values is a pass/fail threshold.  usage: bench_reach.py [dataset] [hidden] [epochs] [--out FILE] [--parent DIR] [--rounds N] [--rmat SCALE]"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_gcn_amd import datagen, provenance
from cuda_gcn_amd.model import HipGCNModel
from cuda_gcn_amd.ops import Device, _ck

HBM_BYTES_S = 6.29e12


def timeit(dev, fn, iters, warmup=2):
    lib = dev.lib
    e0, e1 = C.c_void_p(), C.c_void_p()
    lib.gcnhip_event_create(C.byref(e0)); lib.gcnhip_event_create(C.byref(e1))
    for _ in range(warmup):
        fn()
    dev.sync()
    lib.gcnhip_event_record(dev.ctx, e0)
    for _ in range(iters):
        fn()
    lib.gcnhip_event_record(dev.ctx, e1)
    dev.sync()
    ms = C.c_float()
    lib.gcnhip_event_elapsed_ms(e0, e1, C.byref(ms))
    lib.gcnhip_event_destroy(e0); lib.gcnhip_event_destroy(e1)
    return ms.value / iters


def wall(fn, reps=5):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def note(text):
    print(f"bench_reach: {text}", file=sys.stderr, flush=True)


def epoch_path(parent, rounds):
    """bench.py on the parent checkout and on this one, alternating: epochs/s of every run"""
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = dict(parent=[], this=[])
    for _ in range(rounds):
        for label, root in (("parent", parent), ("this", here)):
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "50", "--warmup", "10"], cwd=root, capture_output=True, text=True,
                               timeout=600, check=True)
            out[label].append(json.loads(r.stdout.strip().splitlines()[-1])["value"])
            note(f"bench.py on {label}: {out[label][-1]}")
    return out


def kernels(dev, gp, gi, seeds, label=None, with_agreement=None):
    """the figures of one graph: the traversal from `seeds` (both forms, per level), the components, the counts"""
    lib = dev.lib
    n = gp.size - 1
    g = dev.graph(gp, gi)
    sb = dev.buf(seeds)
    dist, near, comp, size, marked = (dev.buf((n,), np.int32) for _ in range(5))
    scratch, counts = dev.buf((64,), np.int64), dev.buf((6 + 34 * 4 + 1,), np.int64)
    levels, skipped, rounds = C.c_int(), C.c_int64(), C.c_int()
    lc = np.zeros(n + 1, np.int64)
    out = dict(rows=n, stored_entries=int(gp[-1]), seeds=int(seeds.size), mean_row=float(gp[-1]) / n, longest_row=int(np.diff(gp).max()))
    out["pass_floor_ms"] = 1e3 * (4.0 * gp[-1] + 4.0 * (n + 1)) / HBM_BYTES_S

    def hop(nearest, max_hops=0, sync=8):
        _ck(lib, lib.gcnhip_hop_distance_ex(dev.ctx, g.h, sb.ptr, int(seeds.size), max_hops, dist.ptr, near.ptr if nearest else None, scratch.ptr,
                                            C.byref(levels), lc.ctypes.data, lc.size, C.byref(skipped), 0, sync), "hop_distance")
    for nearest, key in ((False, "distance"), (True, "distance_nearest")):
        hop(nearest)
        L = levels.value
        res = dict(levels=L, rows_per_level=lc[:L + 1].tolist(), unreachable=int(n - lc[:L + 1].sum()))
        res["call_ms"] = wall(lambda: hop(nearest))
        res["call_sync1_ms"] = wall(lambda: hop(nearest, sync=1))
        res["call_sync64_ms"] = wall(lambda: hop(nearest, sync=64))
        upto = [timeit(dev, lambda: hop(nearest, max_hops=k, sync=64), 10) for k in range(1, min(L, 12) + 2)]   # k = L + 1: one empty level more
        res["upto_level_ms"] = upto
        res["level_ms"] = [upto[0]] + [upto[k] - upto[k - 1] for k in range(1, len(upto))]   # [0] holds the clear, the seeding and a read-back too
        res["passes_of_floor"] = res["call_ms"] / out["pass_floor_ms"]
        out[key] = res
        note(f"{key}: {res}")

    def components():
        _ck(lib, lib.gcnhip_components(dev.ctx, g.h, comp.ptr, scratch.ptr, C.byref(rounds)), "components")
    components()
    cres = dict(rounds=rounds.value, call_ms=wall(components))
    cres["per_round_ms"] = cres["call_ms"] / max(rounds.value, 1)
    mark = dev.buf(np.isin(np.arange(n), seeds).astype(np.int32))
    cres["counts_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_component_counts(dev.ctx, comp.ptr, mark.ptr, n, size.ptr, marked.ptr, counts.ptr), "counts"), 20)
    t = counts.download()[:6]
    cres.update(components=int(t[1]), largest=int(t[2]), unseeded_components=int(t[3]), unseeded_rows=int(t[4]))
    out["components"] = cres
    note(f"components: {cres}")
    if label is not None:
        lab = dev.buf(label)
        hop(True)
        out["strata_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_distance_strata(dev.ctx, dist.ptr, near.ptr, lab.ptr, lab.ptr, n, None, n, int(label.max()) + 1, 8,
                                                                                   counts.ptr + 48, counts.ptr + 48 + 8 * 136), "strata"), 20)
        if with_agreement:
            cls = int(label.max()) + 1
            per, ag = dev.buf((3 * n,), np.int32), dev.buf((cls * cls + cls + 9,), np.int64)
            a = ag.ptr
            out["nbr_agreement_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_nbr_agreement(dev.ctx, g.h, lab.ptr, cls, None, n, per.ptr, per.ptr + 4 * n, per.ptr + 8 * n,
                                                                                            a, a + 8 * cls * cls, a + 8 * (cls * cls + cls), a + 8 * (cls * cls + cls + 8)),
                                                              "nbr_agreement"), 20)
            for key in ("distance", "distance_nearest"):
                out[key]["ratio_to_nbr_agreement"] = out[key]["call_ms"] / out["nbr_agreement_ms"]
    return out


def host_reference(gp, gi, seeds):
    """scipy on the host: the multi-source search from a virtual node, and the weak components; wall ms of each (the matrices are
    built outside the timed part)"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import breadth_first_order, connected_components
    n = gp.size - 1
    a = sp.csr_matrix((np.ones(gi.size, np.int8), gi, gp), shape=(n, n))
    # row v gathers from the entries it lists: information flows u -> v, so the search runs over the transpose, from node n
    t = sp.vstack([sp.hstack([a.T.tocsr(), sp.csr_matrix((n, 1), dtype=np.int8)]),
                   sp.csr_matrix((np.ones(seeds.size, np.int8), (np.zeros(seeds.size, np.int64), seeds)), shape=(1, n + 1))]).tocsr()
    t0 = time.perf_counter()
    order, _ = breadth_first_order(t, n, directed=True, return_predecessors=True)
    t1 = time.perf_counter()
    k, _ = connected_components(a, directed=True, connection="weak")
    t2 = time.perf_counter()
    return dict(bfs_wall_ms=1e3 * (t1 - t0), reached=int(order.size) - 1, components_wall_ms=1e3 * (t2 - t1), components=int(k))


def main():
    args = sys.argv[1:]
    opts = {"--parent": None, "--rounds": "3", "--out": None, "--rmat": "18"}
    for flag in list(opts):
        if flag in args:
            i = args.index(flag)
            opts[flag] = args[i + 1]
            del args[i:i + 2]
    name = args[0] if len(args) > 0 else "reddit-syn"
    hidden = int(args[1]) if len(args) > 1 else 128
    epochs = int(args[2]) if len(args) > 2 else 5
    ds = datagen.make_dataset(name)
    gp, gi = np.asarray(ds["g_indptr"]), np.asarray(ds["g_indices"])
    label, split = np.asarray(ds["label"], np.int32), np.asarray(ds["split"])
    train = np.flatnonzero(split == 1).astype(np.int32)
    res = dict(dataset=name, hidden=hidden, epochs=epochs)

    dev = Device(0)
    res["graph"] = kernels(dev, gp, gi, train, label=label, with_agreement=True)
    scale = int(opts["--rmat"])
    if scale > 0:
        rp, ri = datagen.rmat_graph(scale)
        rn = rp.size - 1
        res["rmat"] = dict(kernels(dev, np.asarray(rp), np.asarray(ri), np.sort(np.random.default_rng(1).choice(rn, rn // 100, replace=False)).astype(np.int32)),
                           scale=scale)
    dev.close()

    # ---- the model call against the host
    m = HipGCNModel(ds, seed=1, hidden_dim=hidden, dropout=0.5)
    m.run_epochs(epochs, want_trace=False)
    rep = m.reach_report()
    res["report"] = dict(by_distance=[r for r in rep["by_distance"] if r["rows"]], inside_receptive_field=rep["inside_receptive_field"],
                         outside_receptive_field=rep["outside_receptive_field"], unreachable=rep["unreachable"],
                         nearest_label_accuracy=rep["nearest_label_accuracy"], levels=rep["levels"], n_components=rep["n_components"],
                         largest=rep["largest"], unmarked_components=rep["unmarked_components"], unmarked_nodes=rep["unmarked_nodes"], rounds=rep["rounds"])
    res["reach_report_wall_ms"] = wall(lambda: m.reach_report())
    res["reach_report_no_forward_wall_ms"] = wall(lambda: m.reach_report(predicted=False))
    res["label_distance_wall_ms"] = wall(lambda: m.label_distance(split=3))
    res["components_wall_ms"] = wall(lambda: m.components(split=3))
    res["evaluate_test_split_wall_ms"] = wall(lambda: m.evaluate(split=3))
    m.close()
    res["host"] = host_reference(gp, gi, train)
    res["host"]["agrees"] = bool(res["host"]["components"] == rep["n_components"] and
                                 res["host"]["reached"] == int(sum(res["graph"]["distance"]["rows_per_level"])))
    note(f"reach_report {res['reach_report_wall_ms']:.2f} ms, host {res['host']}")
    if opts["--parent"]:
        runs = epoch_path(opts["--parent"], int(opts["--rounds"]))
        res["epoch_path"] = dict(runs, parent_median=float(np.median(runs["parent"])), this_median=float(np.median(runs["this"])),
                                 parent_spread=[float(min(runs["parent"])), float(max(runs["parent"]))])
    res["_meta"] = dict(sources=provenance.source_sha(["reach.hip", "structure.hip", "common.h", "cuda_gcn_amd/host/reach_query.cpp", "cuda_gcn_amd/host/reach.cpp"]))
    line = json.dumps(res)
    print(line)
    if opts["--out"]:
        with open(opts["--out"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
