"""Link prediction ranks on the hidden layer of reddit-syn (hidden 128) with 5 % of its edges held out, HIP events — the figures of
DESIGN §4.29:
  * on the model's own hidden matrix, for the first 1 024, 16 384 and 65 536 held-out edges (--all: every held-out edge as well): the
    threshold launch (gcnhip_link_ranks, launches = 1) and the walk (launches = 2) without and with the filter (the neighbour sets of
    the remaining graph); one warm-up, 10 timed launches each, mean, min and max kept;
  * each walk against the exact-f32 MFMA floor 2 nq N h FLOP at 157.3 TF and against the product launch of gcnhip_topk_rows
    (launches = 1, k = 10) on the same query rows in the same process, the closest existing launch;
  * link_ranks() as a whole (wall time) for 1 024 queries against embed() plus numpy on the host;
  * MRR and Hits@10 of "dot" and "cosine" on the 16 384 edges after the short training run: a sanity line;
  * with --parent DIR (a built checkout of the parent commit): bench.py in DIR and here, alternating --rounds times.
Prints one JSON line with the hashes of the sources it measured; --out FILE also writes it there.  None of the values is a
pass/fail threshold.  usage: bench_linkrank.py [dataset] [hidden] [epochs] [--out FILE] [--parent DIR] [--rounds N] [--all]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_gcn_amd import datagen, provenance
from cuda_gcn_amd.model import HipGCNModel
from cuda_gcn_amd.ops import Device, _ck
from tools.bench_kmeans import epoch_path, timeit

MFMA_F32_FLOPS = 157.3e12


def note(text):
    print(f"bench_linkrank: {text}", file=sys.stderr, flush=True)


def timed(dev, fn, reps=10):
    fn()
    t = [timeit(dev, fn, 1, warmup=0) for _ in range(reps)]
    return dict(mean_ms=float(np.mean(t)), min_ms=float(min(t)), max_ms=float(max(t)))


def neighbour_sets(ds):
    """the distinct neighbours u != v of every node as a CSR with sorted rows"""
    N = ds["num_nodes"]
    row = np.repeat(np.arange(N, dtype=np.int64), np.diff(ds["g_indptr"]))
    key = np.unique((row * N + ds["g_indices"])[row != ds["g_indices"]])
    x_ptr = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(key // N, minlength=N), out=x_ptr[1:])
    return x_ptr.astype(np.int32), (key % N).astype(np.int32)


def main():
    args = sys.argv[1:]
    opts = {"--parent": None, "--rounds": "3", "--out": None}
    for flag in list(opts):
        if flag in args:
            i = args.index(flag)
            opts[flag] = args[i + 1]
            del args[i:i + 2]
    every = "--all" in args
    args = [a for a in args if a != "--all"]
    name = args[0] if len(args) > 0 else "reddit-syn"
    hidden = int(args[1]) if len(args) > 1 else 128
    epochs = int(args[2]) if len(args) > 2 else 5
    ds, (src, dst) = datagen.hold_out_edges(datagen.make_dataset(name), 0.05, 1)
    order = np.random.default_rng(0).permutation(src.size)
    src, dst = src[order], dst[order]
    N = ds["num_nodes"]
    res = dict(dataset=name, nodes=N, hidden=hidden, epochs=epochs, held_out_edges=int(src.size))
    m = HipGCNModel(ds, seed=1, hidden_dim=hidden, dropout=0.5)
    m.run_epochs(epochs, want_trace=False)
    # ---- the query as a whole, and what it says about the scorer
    m.link_ranks(src[:64], dst[:64])
    t0 = time.perf_counter()
    whole = m.link_ranks(src[:1024], dst[:1024], filtered=False)
    res["link_ranks_1024_wall_ms"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    emb = m.embed()
    s = emb[src[:1024]] @ emb.T
    t = s[np.arange(1024), dst[:1024]][:, None]
    keep = np.ones_like(s, bool)
    keep[np.arange(1024), src[:1024]] = keep[np.arange(1024), dst[:1024]] = False
    host_above = ((s > t) & keep).sum(axis=1)
    res["embed_plus_numpy_1024_wall_ms"] = 1e3 * (time.perf_counter() - t0)
    res["host_above_differs_on"] = int((host_above != whole["above"]).sum())       # numpy's f32 product is another sum order
    for metric in ("dot", "cosine"):
        r = m.link_ranks(src[:16384], dst[:16384], metric=metric, ks=(10,))
        res["quality_" + metric] = dict(queries=r["queries"], mrr=r["mrr"], mean_rank=r["mean_rank"], hits_at_10=r["hits"][10])
    note(f"whole calls: {res}")
    m.close()
    # ---- the launches themselves, on the same matrix
    dev = Device(0)
    lib = dev.lib
    x_ptr, x_ids = neighbour_sets(ds)
    tb, pb, ib = dev.buf(emb), dev.buf(x_ptr), dev.buf(x_ids)
    for nq in [1024, 16384, 65536] + ([int(src.size)] if every else []):
        nq = min(nq, int(src.size))
        sb, db = dev.buf(np.ascontiguousarray(src[:nq])), dev.buf(np.ascontiguousarray(dst[:nq]))
        plan = dev.link_rank_plan(N, nq)
        sc, ab, eb = dev.buf((max(plan["scratch_bytes"] // 4, 1),), np.float32), dev.buf((nq,), np.int32), dev.buf((nq,), np.int32)
        tp = dev.topk_plan(N, nq, 10)
        tsb = dev.buf((tp["scratch_bytes"] // 4,), np.uint32)
        oi, os_ = dev.buf((nq * 10,), np.int32), dev.buf((nq * 10,), np.float32)

        def ranks(launches, filtered):
            _ck(lib, lib.gcnhip_link_ranks(dev.ctx, tb.ptr, hidden, N, hidden, None, sb.ptr, db.ptr, nq, pb.ptr if filtered else None, None,
                                           ib.ptr if filtered else None, 1, 0, sc.ptr, plan["scratch_bytes"], launches, ab.ptr, eb.ptr), "link_ranks")

        def topk():
            _ck(lib, lib.gcnhip_topk_rows(dev.ctx, tb.ptr, hidden, N, hidden, None, None, sb.ptr, nq, 10, 1, 0, tsb.ptr, tp["scratch_bytes"], 1,
                                          oi.ptr, os_.ptr), "topk_rows")
        out = dict(queries=nq, plan=plan, thresholds=timed(dev, lambda: ranks(1, False)), topk_product_k10=timed(dev, topk),
                   walk=timed(dev, lambda: ranks(2, False)), walk_filtered=timed(dev, lambda: ranks(2, True)))
        out["mfma_floor_ms"] = 1e3 * 2.0 * nq * N * hidden / MFMA_F32_FLOPS
        out["floor_over_walk"] = out["mfma_floor_ms"] / out["walk"]["mean_ms"]
        out["walk_over_topk_product"] = out["walk"]["mean_ms"] / out["topk_product_k10"]["mean_ms"]
        out["filtered_over_unfiltered"] = out["walk_filtered"]["mean_ms"] / out["walk"]["mean_ms"]
        res[f"queries_{nq}"] = out
        note(f"{nq} queries: {out}")
    dev.close()
    if opts["--parent"]:
        runs = epoch_path(opts["--parent"], int(opts["--rounds"]))
        res["epoch_path"] = dict(runs, parent_median=float(np.median(runs["parent"])), this_median=float(np.median(runs["this"])))
    res["_meta"] = dict(sources=provenance.source_sha(["linkrank.hip", "embed.hip", "overlap.hip", "common.h", "cuda_gcn_amd/host/linkrank_query.cpp",
                                                       "cuda_gcn_amd/host/linkrank.h"]))
    line = json.dumps(res)
    print(line)
    if opts["--out"]:
        with open(opts["--out"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
