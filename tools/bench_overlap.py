"""Neighbourhood overlap on reddit-syn and R-MAT scale 18, HIP events — the figures of DESIGN §4.27, each launch apart:
  * the canonical pass (gcnhip_overlap_sets);
  * the rows launch over every row and over the test split, bitmap on and off, the lane group by the rule and forced to 4 / 16 /
    64; the pairs launch at 10^6 random pairs; one warm-up, the mean of 5;
  * each against its byte floor: 4 B per streamed set entry (rows: sum over the listed v and u in S(v) of d(u); pairs: d(a) + d(b);
    the pass: 8 B per stored entry) at the copy rate DESIGN uses, 4.0 TB/s;
  * the rows launch against the neighbour-agreement launch on the same rows, which reads the same index stream once;
  * clustering() as a whole over every node (wall time, reddit-syn only; the scipy form (A @ A).multiply(A) is not run here: the
    product's fill does not fit a host at this size — tests/test_overlap_cpu.py holds it on a small graph);
  * with --parent DIR (a built checkout of the parent commit): bench.py --gpus 1 --steps 50 --warmup 10 in DIR and here, alternating
    --rounds times (default 3).
Prints one JSON line with the hashes of the sources it measured; --out FILE also writes it there.  None of the values is a
pass/fail threshold.  usage: bench_overlap.py [--out FILE] [--parent DIR] [--rounds N] [--graphs reddit-syn,rmat-18]"""
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
from cuda_gcn_amd.ops import Device
from tools.bench_kmeans import timeit

COPY_BYTES_PER_S = 4.0e12
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def note(text):
    print(f"bench_overlap: {text}", file=sys.stderr, flush=True)


def ok(rc):
    """a timed call that was refused measured nothing"""
    if rc != 0:
        raise RuntimeError(f"a timed call returned {rc}")


def epoch_path(parent, rounds):
    """bench.py on the parent checkout and on this one, alternating: epochs/s of every run"""
    out = dict(parent=[], this=[])
    for _ in range(rounds):
        for label, root in (("parent", parent), ("this", HERE)):
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "50", "--warmup", "10"], cwd=root, capture_output=True, text=True,
                               timeout=600, check=True)
            out[label].append(json.loads(r.stdout.strip().splitlines()[-1])["value"])
            note(f"bench.py on {label}: {out[label][-1]}")
    return out


def launches(dev, ds):
    """the launches of one graph apart, with their byte floors"""
    lib, ctx = dev.lib, dev.ctx
    ip, ix = np.asarray(ds["g_indptr"], np.int64), np.asarray(ds["g_indices"], np.int32)
    n = ip.size - 1
    g = dev.graph(ip.astype(np.int32), ix, n_cols=n, col_deg=np.ones(n, np.int32))
    sets = dev.overlap_sets(g)
    length = sets[1].download()[:n].astype(np.int64)
    idx = sets[0].download()
    test = np.flatnonzero(np.asarray(ds["split"]) == 3).astype(np.int32)
    streamed = np.zeros(n, np.int64)                            # per row v: sum over u in S(v) of d(u)
    for v in range(n):
        streamed[v] = length[idx[ip[v]:ip[v] + length[v]]].sum()
    out = dict(nodes=n, stored_entries=int(ip[-1]), set_entries=int(length.sum()), max_set=int(length.max()), test_rows=int(test.size),
               lookups_all=int(streamed.sum()), lookups_test=int(streamed[test].sum()))
    plan = C.c_int64()
    ok(lib.gcnhip_overlap_plan(g.h, C.byref(plan)))
    need = plan.value
    scratch = dev.buf(np.zeros(need // 4 + 4, np.int32))
    out["sets_ms"] = timeit(dev, lambda: ok(lib.gcnhip_overlap_sets(ctx, g.h, sets[0].ptr, sets[1].ptr, scratch.ptr, need)), 5)
    out["sets_floor_ms"] = 8.0 * ip[-1] / COPY_BYTES_PER_S * 1e3
    tb, kb = dev.buf(np.zeros(8, np.int64)), dev.buf(np.zeros(1, np.int64))
    t2b, db = dev.buf(np.zeros(n, np.int64)), dev.buf(np.zeros(n, np.int32))
    rb = dev.buf(test)
    for tag, rows, cnt, work in (("all", None, n, streamed.sum()), ("test", rb.ptr, test.size, streamed[test].sum())):
        for name, group, bitmap in (("", 0, 1), ("_nobitmap", 0, 0), ("_g4", 4, 1), ("_g16", 16, 1), ("_g64", 64, 1)):
            fn = lambda: ok(lib.gcnhip_overlap_rows_ex(ctx, g.h, sets[0].ptr, sets[1].ptr, rows, int(cnt), t2b.ptr, db.ptr, tb.ptr, kb.ptr, group, 0, 0, bitmap))
            out[f"rows_{tag}{name}_ms"] = timeit(dev, fn, 5)
        out[f"rows_{tag}_floor_ms"] = 4.0 * float(work) / COPY_BYTES_PER_S * 1e3
        lab = dev.buf(np.asarray(ds["label"], np.int32))
        cb = dev.buf(np.zeros(64, np.int64))
        out[f"agreement_{tag}_ms"] = timeit(dev, lambda: ok(lib.gcnhip_nbr_agreement(ctx, g.h, lab.ptr, int(ds["output_dim"]), rows, int(cnt), db.ptr, None,
                                                                                      None, None, cb.ptr, tb.ptr, kb.ptr)), 5)
    rng = np.random.default_rng(1)
    src, dst = rng.integers(0, n, 10 ** 6).astype(np.int32), rng.integers(0, n, 10 ** 6).astype(np.int32)
    sb, eb, wb = dev.buf(src), dev.buf(dst), dev.buf(rng.integers(0, 1 << 32, n).astype(np.int64))
    cb, ub, xb = dev.buf(np.zeros(10 ** 6, np.int32)), dev.buf(np.zeros(10 ** 6, np.int32)), dev.buf(np.zeros(10 ** 6, np.int64))
    out["pairs_1e6_ms"] = timeit(dev, lambda: ok(lib.gcnhip_overlap_pairs(ctx, g.h, sets[0].ptr, sets[1].ptr, sb.ptr, eb.ptr, 10 ** 6, wb.ptr, cb.ptr, ub.ptr,
                                                                          xb.ptr, kb.ptr)), 5)
    out["pairs_1e6_floor_ms"] = 4.0 * float((length[src] + length[dst]).sum()) / COPY_BYTES_PER_S * 1e3
    return out


def whole_call(ds):
    m = HipGCNModel(ds, seed=1, hidden_dim=16)
    m.clustering(per_node=True)
    t0 = time.perf_counter()
    got = m.clustering(per_node=True)
    t_gpu = time.perf_counter() - t0
    m.close()
    return dict(clustering_ms=t_gpu * 1e3, triangles=got["triangles"], transitivity=got["transitivity"], avg_clustering=got["avg_clustering"],
                sum_t2=int(got["totals"][4]))


def main():
    args = sys.argv[1:]
    opts = {"--parent": None, "--rounds": "3", "--out": None, "--graphs": "reddit-syn,rmat-18"}
    for flag in list(opts):
        if flag in args:
            i = args.index(flag)
            opts[flag] = args[i + 1]
            del args[i:i + 2]
    res = {}
    dev = Device(0)
    for name in opts["--graphs"].split(","):
        ds = datagen.make_dataset(name)
        res[name] = launches(dev, ds)
        note(f"{name}: {res[name]}")
        if name == "reddit-syn":
            res["clustering_call"] = whole_call(ds)
            note(f"clustering(): {res['clustering_call']}")
    dev.close()
    if opts["--parent"]:
        runs = epoch_path(os.path.abspath(opts["--parent"]), int(opts["--rounds"]))
        res["epoch_path"] = dict(runs, parent_median=float(np.median(runs["parent"])), this_median=float(np.median(runs["this"])))
    res["_meta"] = dict(sources=provenance.source_sha(["overlap.hip", "structure.hip", "ranking.hip", "common.h", "cuda_gcn_amd/host/overlap_query.cpp",
                                                        "cuda_gcn_amd/host/overlap.h"]))
    line = json.dumps(res)
    print(line)
    if opts["--out"]:
        with open(opts["--out"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
