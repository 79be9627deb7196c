"""Map quality on the hidden layer of reddit-syn (hidden 128), HIP events — the figures of DESIGN §4.26:
  * on the model's own hidden matrix with its inverse norms, over a 16 384-row sample and over the test split, against a two-column
    lattice map: the selection walk (gcnhip_knn_rows) at k = 10 and 32, the threshold phase alone (gcnhip_nbr_d2) and the whole rank
    launch (gcnhip_nbr_ranks; the walk = the difference) at k = 10 and 32, the sums launch; one warm-up, the mean of 10;
  * each against the exact-f32 MFMA floor of the square, 2 n^2 h FLOP at 157.3 TF, against DBSCAN's COUNT at 8 radii and against the
    t-SNE gradient launch on the same pack in the same process;
  * map_quality() as a whole (wall time) on an 8 192-row node query against embed() plus scikit-learn's trustworthiness on the
    host, where it imports, with both values;
  * with --parent DIR (a built checkout of the parent commit): bench.py --gpus 1 --steps 200 --warmup 20 in DIR and here, alternating
    --rounds times (default 3).
Prints one JSON line with the hashes of the sources it measured; --out FILE also writes it there.  None of the values is a
pass/fail threshold.  usage: bench_mapq.py [dataset] [hidden] [epochs] [--out FILE] [--parent DIR] [--rounds N]"""
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
from tools.bench_kmeans import timeit

MFMA_F32_FLOPS = 157.3e12
SWEEP = np.array([0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.6, 0.8])
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def note(text):
    print(f"bench_mapq: {text}", file=sys.stderr, flush=True)


def epoch_path(parent, rounds):
    """bench.py on the parent checkout and on this one, alternating: epochs/s of every run"""
    out = dict(parent=[], this=[])
    for _ in range(rounds):
        for label, root in (("parent", parent), ("this", HERE)):
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20"], cwd=root, capture_output=True, text=True,
                               timeout=600, check=True)
            out[label].append(json.loads(r.stdout.strip().splitlines()[-1])["value"])
            note(f"bench.py on {label}: {out[label][-1]}")
    return out


def main():
    args = sys.argv[1:]
    opts = {"--parent": None, "--rounds": "3", "--out": None}
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
    res = dict(dataset=name, nodes=N, hidden=hidden, epochs=epochs)
    m = HipGCNModel(ds, seed=1, hidden_dim=hidden, dropout=0.5)
    m.run_epochs(epochs, want_trace=False)
    rng = np.random.default_rng(0)
    lists = dict(sample_16384=np.sort(rng.choice(N, min(16384, N), replace=False)).astype(np.int32),
                 test_split=np.flatnonzero(np.asarray(ds["split"]) == 3).astype(np.int32))
    # ---- the query as a whole, against the host
    q = np.sort(rng.choice(N, min(8192, N), replace=False)).astype(np.int32)
    xq = m.embed(nodes=q, normalize=True)
    yq = np.ascontiguousarray(xq[:, :2])                         # a crude map: the first two unit coordinates
    m.map_quality(yq, k=10, nodes=q, per_node=False)             # the code object's load
    t0 = time.perf_counter()
    whole = m.map_quality(yq, k=10, nodes=q, per_node=False)
    res["map_quality_query_8192"] = dict(rows=int(q.size), wall_ms=1e3 * (time.perf_counter() - t0), **whole)
    try:
        from sklearn.manifold import trustworthiness
        t0 = time.perf_counter()
        host = trustworthiness(m.embed(nodes=q, normalize=True).astype(np.float64), yq.astype(np.float64), n_neighbors=10)
        res["map_quality_query_8192"].update(embed_plus_sklearn_wall_ms=1e3 * (time.perf_counter() - t0), sklearn_trustworthiness=float(host))
    except ImportError as e:
        res["map_quality_query_8192"]["sklearn"] = repr(e)
    note(f"map_quality() against the host: {res['map_quality_query_8192']}")
    emb = m.embed()
    m.close()
    # ---- the launches themselves, on the same matrix
    dev = Device(0)
    lib = dev.lib
    inv = dev.embed_inv_norms(emb)
    for what, rows in lists.items():
        n = int(rows.size)
        tplan = dev.tsne_plan(n, hidden)
        sbytes = max(min(tplan["bytes"], 256 << 20), tplan["bytes_min"])
        pk = dev.tsne_pack(emb, rows=rows, inv_norm=inv, scratch_bytes=sbytes)
        py = dev.tsne_pack(np.ascontiguousarray((emb * inv[:, None])[:, :2]), rows=rows, scratch_bytes=16)
        dev.tsne_bandwidths(pk, 30.0)
        y, sums = dev.buf((1e-2 * rng.standard_normal((n, 2))).astype(np.float32)), dev.buf((n * 9,), np.float64)
        cnt = dev.buf((8 * n,), np.int32)
        pos = {k: dev.buf((n * k,), np.int32) for k in (10, 32)}
        posy, rx, ry = dev.buf((n * 10,), np.int32), dev.buf((n * 32,), np.int32), dev.buf((n * 10,), np.int32)
        d2, per, tot = dev.buf((n * 32,), np.float32), dev.buf((n * 3,), np.int32), dev.buf((4,), np.int64)
        pp, eight = pk["pack"].ptr, np.ascontiguousarray(SWEEP)

        def knn(k, pack=pp, dim=hidden, out=None):
            _ck(lib, lib.gcnhip_knn_rows(dev.ctx, pack, n, dim, k, (out or pos[k]).ptr, d2.ptr), "knn_rows")

        def thresholds(k):
            _ck(lib, lib.gcnhip_nbr_d2(dev.ctx, pp, n, hidden, k, pos[k].ptr, d2.ptr), "nbr_d2")

        def ranks(k):
            _ck(lib, lib.gcnhip_nbr_ranks(dev.ctx, pp, n, hidden, k, pos[k].ptr, rx.ptr), "nbr_ranks")

        def sums_launch():
            _ck(lib, lib.gcnhip_mapq_sums(dev.ctx, pp, hidden, py["pack"].ptr, 2, n, 10, pos[10].ptr, posy.ptr, rx.ptr, ry.ptr, per.ptr, tot.ptr), "sums")

        def count():
            _ck(lib, lib.gcnhip_dbscan_counts(dev.ctx, pp, n, hidden, eight.ctypes.data, 8, cnt.ptr), "counts")

        def gradient():
            _ck(lib, lib.gcnhip_tsne_gradient(dev.ctx, pp, n, hidden, y.ptr, 2, 0, sums.ptr, pk["scratch"].ptr, sbytes), "gradient")
        out = dict(rows=n, mfma_floor_ms=1e3 * 2.0 * n * n * hidden / MFMA_F32_FLOPS)
        for k in (10, 32):
            out[f"knn_k{k}_ms"] = timeit(dev, lambda: knn(k), 10)
            out[f"thresholds_k{k}_ms"] = timeit(dev, lambda: thresholds(k), 10)
            out[f"ranks_k{k}_ms"] = timeit(dev, lambda: ranks(k), 10)
            out[f"rank_walk_k{k}_ms"] = out[f"ranks_k{k}_ms"] - out[f"thresholds_k{k}_ms"]
        knn(10, py["pack"].ptr, 2, posy)                         # the map's lists, and two rank tables the sums launch can read
        _ck(lib, lib.gcnhip_nbr_ranks(dev.ctx, pp, n, hidden, 10, posy.ptr, rx.ptr), "nbr_ranks")
        _ck(lib, lib.gcnhip_nbr_ranks(dev.ctx, py["pack"].ptr, n, 2, 10, pos[10].ptr, ry.ptr), "nbr_ranks")
        out["knn_map_k10_ms"] = timeit(dev, lambda: knn(10, py["pack"].ptr, 2, posy), 10)
        out["sums_ms"] = timeit(dev, sums_launch, 10)
        out["dbscan_count_e8_ms"] = timeit(dev, count, 10)
        out["tsne_gradient_ms"] = timeit(dev, gradient, 10)
        for key in ("knn_k10_ms", "knn_k32_ms", "ranks_k10_ms", "ranks_k32_ms"):
            out[key[:-3] + "_over_floor"] = out[key] / out["mfma_floor_ms"]
            out[key[:-3] + "_over_dbscan_count_e8"] = out[key] / out["dbscan_count_e8_ms"]
            out[key[:-3] + "_over_tsne_gradient"] = out[key] / out["tsne_gradient_ms"]
        res[what] = out
        note(f"{what}: {out}")
    dev.close()
    if opts["--parent"]:
        runs = epoch_path(os.path.abspath(opts["--parent"]), int(opts["--rounds"]))
        res["epoch_path"] = dict(runs, parent_median=float(np.median(runs["parent"])), this_median=float(np.median(runs["this"])))
    res["_meta"] = dict(sources=provenance.source_sha(["mapq.hip", "dbscan.hip", "tsne.hip", "tsne_pack.h", "common.h", "cuda_gcn_amd/host/mapq_query.cpp"]))
    line = json.dumps(res)
    print(line)
    if opts["--out"]:
        with open(opts["--out"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
