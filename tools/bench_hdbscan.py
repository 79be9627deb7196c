"""HDBSCAN on the hidden layer of reddit-syn (hidden 128), HIP events — the figures of DESIGN §4.28:
  * on the model's own hidden matrix with its inverse norms, over a 16 384-row sample and over the test split, min_samples 5: the
    NEAREST launch (gcnhip_hdbscan_nearest) of round 1 and of the last round, the pick + hook + jump launches (gcnhip_hdbscan_merge),
    and all rounds together; one warm-up, the mean of 10 for the launches (a launch reads comp and only lowers `best`, so a repeat
    does the same work), one timed run for the rounds together;
  * the round-1 NEAREST launch against the exact-f32 MFMA floor of HALF the square, n^2 . h FLOP at 157.3 TF, and against the DBSCAN
    count launch at one radius (gcnhip_dbscan_counts: the same products, a compare and a popcount behind them) on the same pack in
    the same process; the last round against the first shows what the tile skip buys;
  * hdbscan() as a whole (wall time) on the same lists, and on an 8 192-row node query against embed() plus scikit-learn's
    HDBSCAN(algorithm="brute") on the host, where it imports, with the adjusted Rand index between the two labellings;
  * with --parent DIR (a built checkout of the parent commit): bench.py in DIR and here, alternating --rounds times.
Prints one JSON line with the hashes of the sources it measured; --out FILE also writes it there.  None of the values is a
pass/fail threshold.  usage: bench_hdbscan.py [dataset] [hidden] [epochs] [--out FILE] [--parent DIR] [--rounds N]"""
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
MIN_SAMPLES = 5


def note(text):
    print(f"bench_hdbscan: {text}", file=sys.stderr, flush=True)


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
    N = ds["num_nodes"]
    res = dict(dataset=name, nodes=N, hidden=hidden, epochs=epochs, min_samples=MIN_SAMPLES)
    m = HipGCNModel(ds, seed=1, hidden_dim=hidden, dropout=0.5)
    m.run_epochs(epochs, want_trace=False)
    rng = np.random.default_rng(0)
    lists = dict(sample_16384=np.sort(rng.choice(N, min(16384, N), replace=False)).astype(np.int32),
                 test_split=np.flatnonzero(np.asarray(ds["split"]) == 3).astype(np.int32))
    q = np.sort(rng.choice(N, min(8192, N), replace=False)).astype(np.int32)
    # ---- the query as a whole
    m.hdbscan(nodes=q[:512], report=False)                         # code objects loaded, buffers warm
    for what, rows in list(lists.items()) + [("query_8192", q)]:
        t0 = time.perf_counter()
        whole = m.hdbscan(nodes=rows, report=False)
        res["hdbscan_" + what] = dict(rows=int(rows.size), wall_ms=1e3 * (time.perf_counter() - t0),
                                      **{k: whole[k] for k in ("n_clusters", "n_noise", "rounds")})
        note(f"hdbscan() on {what}: {res['hdbscan_' + what]}")
    try:
        from sklearn.cluster import HDBSCAN
        from sklearn.metrics import adjusted_rand_score
        t0 = time.perf_counter()
        host = HDBSCAN(min_cluster_size=5, algorithm="brute", copy=True).fit(m.embed(nodes=q, normalize=True)).labels_
        res["hdbscan_query_8192"].update(embed_plus_sklearn_wall_ms=1e3 * (time.perf_counter() - t0),
                                         sklearn_clusters=int(host.max() + 1), ari_with_sklearn=float(adjusted_rand_score(host, whole["labels"])))
    except ImportError as e:
        res["hdbscan_query_8192"]["sklearn"] = repr(e)
    note(f"against the host: {res['hdbscan_query_8192']}")
    emb = m.embed()
    m.close()
    # ---- the launches themselves, on the same matrix
    dev = Device(0)
    lib = dev.lib
    inv = dev.embed_inv_norms(emb)
    for what, rows in lists.items():
        n, k = int(rows.size), MIN_SAMPLES - 1
        pk = dev.tsne_pack(emb, rows=rows, inv_norm=inv, scratch_bytes=16)
        state_bytes = dev.hdbscan_plan(n, hidden)["state_bytes"]
        state, edges, counts = dev.buf((state_bytes // 4,), np.uint32), dev.buf((3 * n,), np.int32), dev.buf((2,), np.int32)
        cnt, d2 = dev.buf((n,), np.int32), dev._knn_rows(pk, k)[1]
        pp, eps = pk["pack"].ptr, np.array([0.3])

        def start():
            _ck(lib, lib.gcnhip_hdbscan_start(dev.ctx, pp, n, hidden, d2.ptr, k, state.ptr, state_bytes), "start")

        def nearest():
            _ck(lib, lib.gcnhip_hdbscan_nearest(dev.ctx, pp, n, hidden, state.ptr, state_bytes), "nearest")

        def merge():
            _ck(lib, lib.gcnhip_hdbscan_merge(dev.ctx, pp, n, hidden, state.ptr, state_bytes, edges.ptr, counts.ptr), "merge")

        def count():
            _ck(lib, lib.gcnhip_dbscan_counts(dev.ctx, pp, n, hidden, eps.ctypes.data, 1, cnt.ptr), "counts")

        def rounds_left():
            r = 0
            while True:
                nearest()
                merge()
                r += 1
                if int(counts.download()[0]) <= 1:
                    return r
        out = dict(rows=n)
        start()
        out["nearest_round1_ms"] = timeit(dev, nearest, 10)
        out["dbscan_count_e1_ms"] = timeit(dev, count, 10)
        per_round, comps = [], []
        while True:                                                # round by round: the nearest launch, then its merge
            per_round.append(timeit(dev, nearest, 3))
            merge_ms = timeit(dev, merge, 1, warmup=0)
            comps.append(int(counts.download()[0]))
            if comps[-1] <= 1:
                break
        out.update(rounds=len(per_round), nearest_per_round_ms=per_round, components_after_round=comps, nearest_last_round_ms=per_round[-1],
                   merge_last_round_ms=merge_ms)
        start()
        out["merge_round1_ms"] = (timeit(dev, lambda: (nearest(), merge()), 1, warmup=0) - out["nearest_round1_ms"])
        start()
        dev.sync()
        t0 = time.perf_counter()
        rounds_left()
        out["all_rounds_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        out["half_square_floor_ms"] = 1e3 * n * n * hidden / MFMA_F32_FLOPS
        out["floor_over_nearest_round1"] = out["half_square_floor_ms"] / out["nearest_round1_ms"]
        out["nearest_round1_over_dbscan_count"] = out["nearest_round1_ms"] / out["dbscan_count_e1_ms"]
        out["nearest_last_over_first"] = out["nearest_last_round_ms"] / out["nearest_round1_ms"]
        res[what] = out
        note(f"{what}: {out}")
    dev.close()
    if opts["--parent"]:
        runs = epoch_path(opts["--parent"], int(opts["--rounds"]))
        res["epoch_path"] = dict(runs, parent_median=float(np.median(runs["parent"])), this_median=float(np.median(runs["this"])))
    res["_meta"] = dict(sources=provenance.source_sha(["hdbscan.hip", "dbscan.hip", "mapq.hip", "tsne_pack.h", "bucket.h", "common.h",
                                                       "cuda_gcn_amd/host/hdbscan_query.cpp", "cuda_gcn_amd/host/hdbscan.cpp"]))
    line = json.dumps(res)
    print(line)
    if opts["--out"]:
        with open(opts["--out"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
