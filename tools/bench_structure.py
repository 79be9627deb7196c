"""The structure report on reddit-syn (41 classes), HIP events — the figures of DESIGN §4.20:
  * the gcnhip_nbr_agreement launch of csrc/structure.hip (per-position outputs and mixing counts on) over every row and over the
    test split, with each lane grouping, against its byte floor at the HBM copy rate (6.29 TB/s): 4 B per stored entry walked,
    the row pointers (4 B per row over every row, 8 B per listed row plus the 4 B of the list entry), and the three int32 outputs
    per position; the label gathers are not in the floor (the table stays in L2);
  * the same launch against the class-width aggregation on the same rows of the same adjacency object: gcnhip_graphsum_ex at
    dim = 41 in rows of 48 floats (192 B gathered per entry), with per-edge coefficients and factored, every row and the test
    split as a registered row subset; `ratio` is agreement / the FASTER of the two aggregations and is meant to stay at or
    below 1.035 (the spread README records between machines);
  * structure_report() as a whole (wall time) against evaluate() and against datagen.edge_homophily(ds) on the host;
  * with --parent DIR (a built checkout of the parent commit): `python bench.py --gpus 1 --steps 50 --warmup 10` in DIR and here,
    alternating --rounds times (default 2): the epoch path is meant not to move.
Prints one JSON line, with the hashes of the sources it measured (cuda_gcn_amd/provenance.py); --out FILE also writes it there.
None of the values is a pass/fail threshold.  usage: bench_structure.py [dataset] [hidden] [epochs] [--out FILE] [--parent DIR] [--rounds N]"""
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
from cuda_gcn_amd.ops import Device, GsOpts, _ck

HBM_BYTES_S = 6.29e12
SPREAD = 1.035


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


def wall(fn, reps=3):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def note(text):
    print(f"bench_structure: {text}", file=sys.stderr, flush=True)


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


def main():
    args = sys.argv[1:]
    opts = {"--parent": None, "--rounds": "2", "--out": None}
    for flag in list(opts):
        if flag in args:
            i = args.index(flag)
            opts[flag] = args[i + 1]
            del args[i:i + 2]
    name = args[0] if len(args) > 0 else "reddit-syn"
    hidden = int(args[1]) if len(args) > 1 else 128
    epochs = int(args[2]) if len(args) > 2 else 5
    ds = datagen.make_dataset(name)
    N, cls = ds["num_nodes"], ds["output_dim"]
    gp, gi = np.asarray(ds["g_indptr"]), np.asarray(ds["g_indices"])
    label, split = np.asarray(ds["label"], np.int32), np.asarray(ds["split"])
    res = dict(dataset=name, nodes=N, classes=cls, stored_entries=int(gp[-1]), hidden=hidden, epochs=epochs)

    # ---- the launches themselves, on the dataset's adjacency
    dev = Device(0)
    lib = dev.lib
    g = dev.graph(gp, gi)
    test = np.flatnonzero(split == 3).astype(np.int32)
    lab = dev.buf(label)
    per, tb = dev.buf((3 * N,), np.int32), dev.buf(test)
    counts = dev.buf((cls * cls + cls + 8 + 1,), np.int64)
    mix, crow, tot, skip = counts.ptr, counts.ptr + 8 * cls * cls, counts.ptr + 8 * (cls * cls + cls), counts.ptr + 8 * (cls * cls + cls + 8)
    ld = 48
    xin, xout, ep = dev.buf(np.random.default_rng(0).random((N, ld), np.float32)), dev.buf((N, ld), np.float32), dev.buf(np.zeros(1, np.uint32))
    g.reserve(cls)
    subset = g.add_rowset(split == 3)
    for what, rows, n, handle in (("all_rows", None, N, None), ("test_split", tb.ptr, int(test.size), subset)):
        walked = int(gp[-1]) if rows is None else int((gp[test + 1] - gp[test]).sum())
        out = dict(rows=n, entries_walked=walked)
        floor_bytes = 4.0 * walked + (4.0 * (n + 1) if rows is None else 12.0 * n) + 12.0 * n
        out["floor_ms"] = 1e3 * floor_bytes / HBM_BYTES_S

        def agree(group):
            _ck(lib, lib.gcnhip_nbr_agreement_ex(dev.ctx, g.h, lab.ptr, cls, rows, n, per.ptr, per.ptr + 4 * n, per.ptr + 8 * n, mix, crow, tot, skip, group, 0),
                "nbr_agreement")

        def aggregate(scaling):
            o = GsOpts()
            o.rows, o.scaling, o.d_epoch = handle, scaling, ep.ptr
            rc = lib.gcnhip_graphsum_ex(dev.ctx, g.h, C.byref(o), xin.ptr, ld, xout.ptr, ld, cls)
            if rc != 0:
                raise RuntimeError(f"gcnhip_graphsum_ex: {rc}: {lib.gcnhip_last_error().decode()}")
        for group in (0, 4, 16, 64):
            out["agreement_ms" if group == 0 else f"agreement_group{group}_ms"] = timeit(dev, lambda: agree(group), 20)
        out["aggregation_coef_ms"] = timeit(dev, lambda: aggregate(0), 20)
        try:
            out["aggregation_factored_ms"] = timeit(dev, lambda: aggregate(1), 20)
        except RuntimeError as e:                              # an object without factor arrays: the per-edge form alone
            note(str(e))
            out["aggregation_factored_ms"] = out["aggregation_coef_ms"]
        out["agreement_again_ms"] = timeit(dev, lambda: agree(0), 20)      # once more behind the aggregations: the same clocks
        best = min(out["agreement_ms"], out["agreement_again_ms"])
        out["aggregation_ms"] = min(out["aggregation_coef_ms"], out["aggregation_factored_ms"])
        out["ratio"] = best / out["aggregation_ms"]
        out["within_spread"] = bool(out["ratio"] <= SPREAD)
        out["fraction_of_floor"] = out["floor_ms"] / best
        out["entries_per_s"] = walked / (best * 1e-3)
        res[what] = out
        note(f"{what}: {out}")
    t = counts.download()
    res["edge_homophily_gpu"] = float(np.trace(t[:cls * cls].reshape(cls, cls)) / max(t[:cls * cls].sum(), 1))   # of the last launch: the test split
    for b in (lab, per, tb, counts, xin, xout, ep):
        b.free()
    del g
    dev.close()

    # ---- the model call
    m = HipGCNModel(ds, seed=1, hidden_dim=hidden, dropout=0.5)
    m.run_epochs(epochs, want_trace=False)
    rep = m.structure_report()
    res["report"] = dict(edge_homophily=rep["truth"]["edge_homophily"], node_homophily=rep["truth"]["node_homophily"],
                         adjusted_homophily=rep["truth"]["adjusted_homophily"],
                         class_insensitive_homophily=rep["truth"]["class_insensitive_homophily"], pred_edge_homophily=rep["pred"]["edge_homophily"],
                         by_degree=[r for r in rep["by_degree"] if r["rows"]], by_agreement=rep["by_agreement"])
    res["structure_report_wall_ms"] = wall(lambda: m.structure_report())
    res["structure_report_test_split_wall_ms"] = wall(lambda: m.structure_report(split=3))
    res["structure_report_truth_only_wall_ms"] = wall(lambda: m.structure_report(predicted=False))
    res["evaluate_wall_ms"] = wall(lambda: m.evaluate())
    res["evaluate_test_split_wall_ms"] = wall(lambda: m.evaluate(split=3))
    t0 = time.perf_counter()
    res["host_edge_homophily"] = datagen.edge_homophily(ds)
    res["host_edge_homophily_wall_ms"] = 1e3 * (time.perf_counter() - t0)
    res["edge_homophily_matches_host"] = bool(res["host_edge_homophily"] == rep["truth"]["edge_homophily"])
    m.close()
    note(f"structure_report {res['structure_report_wall_ms']:.2f} ms, evaluate {res['evaluate_wall_ms']:.2f} ms, host edge homophily "
         f"{res['host_edge_homophily_wall_ms']:.1f} ms")
    if opts["--parent"]:
        runs = epoch_path(opts["--parent"], int(opts["--rounds"]))
        res["epoch_path"] = dict(runs, parent_median=float(np.median(runs["parent"])), this_median=float(np.median(runs["this"])))
    res["_meta"] = dict(sources=provenance.source_sha(["structure.hip", "graphsum.hip", "common.h", "cuda_gcn_amd/host/structure_query.cpp",
                                                       "cuda_gcn_amd/host/structure.cpp"]))
    line = json.dumps(res)
    print(line)
    if opts["--out"]:
        with open(opts["--out"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
