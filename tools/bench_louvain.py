"""Louvain communities on reddit-syn, HIP events and wall time — the figures of DESIGN §4.32:
  * communities() as a whole (wall time of 7 calls behind one warm-up: the median and the range), with its levels, sweeps and
    modularity;
  * one level-0 call (gcnhip_louvain_level) and its coarsening (gcnhip_louvain_coarsen) apart, the C entry points on resident
    buffers, one warm-up, the mean of 5;
  * beside them the nearest existing measures of the adjacency on the same graph: the canonical pass (gcnhip_overlap_sets) and one
    gcnhip_overlap_rows walk over every row;
  * with --parent DIR (a built checkout of the parent commit): bench.py --gpus 1 --steps 50 --warmup 10 in DIR and here, alternating
    --rounds times (default 3).
Prints one JSON line with the hashes of the sources it measured; --out FILE also writes it there.  None of the values is a
pass/fail threshold.  usage: bench_louvain.py [--out FILE] [--parent DIR] [--rounds N] [--graph reddit-syn]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_gcn_amd import datagen, provenance
from cuda_gcn_amd.model import HipGCNModel
from cuda_gcn_amd.ops import Device
from tools.bench_kmeans import timeit
from tools.bench_overlap import epoch_path, ok


def launches(dev, ds):
    lib, ctx = dev.lib, dev.ctx
    ip, ix = np.asarray(ds["g_indptr"], np.int32), np.asarray(ds["g_indices"], np.int32)
    n = ip.size - 1
    g = dev.graph(ip, ix, n_cols=n, col_deg=np.ones(n, np.int32))
    sets = dev.overlap_sets(g)
    plan = C.c_int64()
    ok(lib.gcnhip_overlap_plan(g.h, C.byref(plan)))
    scratch = dev.buf(np.zeros(plan.value // 4 + 4, np.int32))
    out = dict(nodes=n, stored_entries=int(ip[-1]))
    out["sets_ms"] = timeit(dev, lambda: ok(lib.gcnhip_overlap_sets(ctx, g.h, sets[0].ptr, sets[1].ptr, scratch.ptr, plan.value)), 3)
    tb, kb, t2b, db = dev.buf(np.zeros(8, np.int64)), dev.buf(np.zeros(1, np.int64)), dev.buf(np.zeros(n, np.int64)), dev.buf(np.zeros(n, np.int32))
    out["rows_all_ms"] = timeit(dev, lambda: ok(lib.gcnhip_overlap_rows(ctx, g.h, sets[0].ptr, sets[1].ptr, None, n, t2b.ptr, db.ptr, tb.ptr, kb.ptr)), 3)
    lv = dev.louvain_level0(g, sets)
    first = dev.louvain_level(lv)                                # the wrappers once, for the buffers; then the entry points alone
    _, coarse = dev.louvain_coarsen(lv, first["comm"])
    work, need = dev._louvain_scratch(lv)
    args, info = (ctx,) + dev._louvain_args(lv), np.zeros(8, np.int64)
    out["level0_ms"] = timeit(dev, lambda: ok(lib.gcnhip_louvain_level(*args, 100, first["comm"].ptr, first["tot"].ptr, info.ctypes.data, work.ptr, need)), 5)
    label = dev.buf(np.zeros(n, np.int32))
    out["coarsen0_ms"] = timeit(dev, lambda: ok(lib.gcnhip_louvain_coarsen(*args, first["comm"].ptr, label.ptr, coarse["ptr"].ptr, coarse["len"].ptr,
                                                                           coarse["idx"].ptr, coarse["w"].ptr, coarse["self_w"].ptr, info.ctypes.data, work.ptr,
                                                                           need, 0)), 5)
    out.update(level0_sweeps=first["sweeps"], level0_wg_rows=first["wg_rows"], level0_long_rows=first["long_rows"], level1_vertices=coarse["n"],
               level1_extent=coarse["entries"])
    return out


def whole_call(ds):
    m = HipGCNModel(ds, seed=1, hidden_dim=16)
    m.communities(report=False)
    walls = []
    for _ in range(7):
        t0 = time.perf_counter()
        got = m.communities(report=False)
        walls.append((time.perf_counter() - t0) * 1e3)
    m.close()
    return dict(communities_ms=float(np.median(walls)), communities_ms_min=min(walls), communities_ms_max=max(walls), communities=got["communities"], modularity=got["modularity"], numerator=got["numerator"], m2=got["m2"],
                levels=len(got["level_records"]), sweeps=sum(r[1] for r in got["level_records"]), level_records=got["level_records"])


def main():
    args = sys.argv[1:]
    opts = {"--parent": None, "--rounds": "3", "--out": None, "--graph": "reddit-syn"}
    for flag in list(opts):
        if flag in args:
            i = args.index(flag)
            opts[flag] = args[i + 1]
            del args[i:i + 2]
    ds = datagen.make_dataset(opts["--graph"])
    dev = Device(0)
    res = {opts["--graph"]: launches(dev, ds)}
    dev.close()
    res["communities_call"] = whole_call(ds)
    if opts["--parent"]:
        runs = epoch_path(os.path.abspath(opts["--parent"]), int(opts["--rounds"]))
        res["epoch_path"] = dict(runs, parent_median=float(np.median(runs["parent"])), this_median=float(np.median(runs["this"])))
    res["_meta"] = dict(sources=provenance.source_sha(["louvain.hip", "overlap.hip", "common.h", "cuda_gcn_amd/host/louvain_query.cpp"]))
    line = json.dumps(res)
    print(line)
    if opts["--out"]:
        with open(opts["--out"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
