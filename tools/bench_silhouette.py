"""Silhouette widths on the hidden layer of reddit-syn (hidden 128, k = 41), HIP events — the figures of DESIGN §4.23:
  * the labels are a cluster() run over every node; the sums launches (gcnhip_silhouette_sums: bucketing, the distance kernel and
    the fold) and the rows launches (gcnhip_silhouette_rows) of csrc/silhouette.hip are timed apart on the model's own hidden
    matrix with its inverse norms, over the test split, a 16 384-row sample and every row, with the scratch cap silhouette() uses;
  * the sums against 2 . n^2 . h FLOP at 157.3 TF (the exact-f32 MFMA) and against gcnhip_kmeans_assign on the same rows; the rows
    launch against its byte floor at the HBM rate (6.3 TB/s): n . k . 8 B of sums read, 32 B per row written, 4 B of labels read
    once per label;
  * silhouette() as a whole (wall time) on an 8 192-row node query against embed() plus scikit-learn's silhouette_samples on the
    host, where it imports;
  * with --parent DIR (a built checkout of the parent commit): `python bench.py --gpus 1 --steps 50 --warmup 10` in DIR and here,
    alternating --rounds times (default 2): the epoch path is meant not to move.
Prints one JSON line, with the hashes of the sources it measured (cuda_gcn_amd/provenance.py); --out FILE also writes it there.
None of the values is a pass/fail threshold.  usage: bench_silhouette.py [dataset] [hidden] [epochs] [--out FILE] [--parent DIR]
[--rounds N] [--k K]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_gcn_amd import datagen, provenance
from cuda_gcn_amd.model import HipGCNModel
from cuda_gcn_amd.ops import Device, _ck
from tools.bench_kmeans import epoch_path, timeit, wall

MFMA_F32_FLOPS, HBM_BYTES_S = 157.3e12, 6.3e12
SCRATCH_CAP = 256 << 20                                           # ModelQueries::SILHOUETTE_SCRATCH_DEFAULT


def note(text):
    print(f"bench_silhouette: {text}", file=sys.stderr, flush=True)


def main():
    args = sys.argv[1:]
    opts = {"--parent": None, "--rounds": "2", "--out": None, "--k": "41"}
    for flag in list(opts):
        if flag in args:
            i = args.index(flag)
            opts[flag] = args[i + 1]
            del args[i:i + 2]
    name = args[0] if len(args) > 0 else "reddit-syn"
    hidden = int(args[1]) if len(args) > 1 else 128
    epochs = int(args[2]) if len(args) > 2 else 5
    k = int(opts["--k"])
    ds = datagen.make_dataset(name)
    N = ds["num_nodes"]
    res = dict(dataset=name, nodes=N, hidden=hidden, epochs=epochs, k=k)
    m = HipGCNModel(ds, seed=1, hidden_dim=hidden, dropout=0.5)
    m.run_epochs(epochs, want_trace=False)
    assign = m.cluster(k=k, iters=20, report=False)["assign"]
    rng = np.random.default_rng(0)
    lists = dict(test_split=np.flatnonzero(np.asarray(ds["split"]) == 3).astype(np.int32),
                 sample_16384=np.sort(rng.choice(N, min(16384, N), replace=False)).astype(np.int32), every_row=None)
    # ---- the query as a whole, against the host
    q = np.sort(rng.choice(N, min(8192, N), replace=False)).astype(np.int32)
    whole = m.silhouette(assign[q], k=k, nodes=q)
    out = dict(rows=int(q.size), score=whole["score"], silhouette_wall_ms=wall(lambda: m.silhouette(assign[q], k=k, nodes=q)))
    try:
        from sklearn.metrics import silhouette_samples
    except ImportError:
        silhouette_samples = None
    if silhouette_samples is not None and np.unique(assign[q]).size >= 2:
        t0 = time.perf_counter()
        host = silhouette_samples(m.embed(nodes=q, normalize=True).astype(np.float64), assign[q], metric="euclidean")
        out["embed_plus_sklearn_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        out["max_abs_difference_to_sklearn"] = float(np.abs(host - whole["s"]).max())
    res["query_8192"] = out
    note(f"silhouette() on {q.size} rows: {out}")
    emb = m.embed()
    m.close()
    # ---- the launches themselves, on the same matrix
    dev = Device(0)
    lib = dev.lib
    table, inv = dev.buf(emb), dev.buf((N,), np.float32)
    _ck(lib, lib.gcnhip_embed_inv_norms(dev.ctx, table.ptr, hidden, N, hidden, inv.ptr), "inv_norms")
    centers, cn = dev.buf(np.zeros((k, hidden), np.float32)), dev.buf(np.ones((k,), np.float32))
    for what, rows in lists.items():
        n = N if rows is None else int(rows.size)
        lab = assign if rows is None else assign[rows]
        plan = dev.silhouette_plan(n, k, hidden)
        sbytes = max(min(plan["bytes"], SCRATCH_CAP), plan["bytes_min"])
        rb = None if rows is None else dev.buf(rows)
        lb, sb = dev.buf(np.ascontiguousarray(lab, np.int32)), dev.buf((sbytes // 4 + 4,), np.uint32)
        ub, zb = dev.buf((n * k,), np.float64), dev.buf((k,), np.int32)
        ob, nb = dev.buf((3 * n + k + 1,), np.float64), dev.buf((n + 3,), np.int32)
        ab, db, fb = dev.buf((n,), np.int32), dev.buf((n,), np.float32), dev.buf((1,), np.int32)
        rp = rb.ptr if rb else None

        def sums():
            _ck(lib, lib.gcnhip_silhouette_sums(dev.ctx, table.ptr, hidden, N, hidden, inv.ptr, rp, n, lb.ptr, k, ub.ptr, zb.ptr, sb.ptr, sbytes), "sums")

        def widths():
            _ck(lib, lib.gcnhip_silhouette_rows(dev.ctx, ub.ptr, lb.ptr, zb.ptr, rp, N, n, k, ob.ptr, ob.ptr + 8 * n, ob.ptr + 16 * n, nb.ptr,
                                                ob.ptr + 24 * n, ob.ptr + 24 * n + 8 * k, nb.ptr + 4 * n), "rows")

        def assign_launch():
            _ck(lib, lib.gcnhip_kmeans_assign(dev.ctx, table.ptr, hidden, N, hidden, inv.ptr, rp, n, centers.ptr, hidden, cn.ptr, k, None, ab.ptr, db.ptr,
                                              fb.ptr), "assign")
        iters = 2 if n > 100000 else 10
        out = dict(rows=n, scratch_mb=sbytes / 2 ** 20, full_scratch_mb=plan["bytes"] / 2 ** 20, segments_max=n // 512 + k)
        out["sums_ms"] = timeit(dev, sums, iters)
        out["rows_ms"] = timeit(dev, widths, 10)
        out["kmeans_assign_ms"] = timeit(dev, assign_launch, 10)
        out["sums_floor_flop_ms"] = 1e3 * 2.0 * n * n * hidden / MFMA_F32_FLOPS
        out["sums_fraction_of_mfma_floor"] = out["sums_floor_flop_ms"] / out["sums_ms"]
        out["sums_tflops"] = 2.0 * n * n * hidden / (out["sums_ms"] * 1e-3) / 1e12
        out["rows_floor_hbm_ms"] = 1e3 * (8.0 * n * k + 32.0 * n + 4.0 * n * (k + 1)) / HBM_BYTES_S
        res[what] = out
        note(f"{what}: {out}")
        for b in (rb, lb, sb, ub, zb, ob, nb, ab, db, fb):
            if b is not None:
                b.free()
    for b in (table, inv, centers, cn):
        b.free()
    dev.close()
    if opts["--parent"]:
        runs = epoch_path(opts["--parent"], int(opts["--rounds"]))
        res["epoch_path"] = dict(runs, parent_median=float(np.median(runs["parent"])), this_median=float(np.median(runs["this"])))
    res["_meta"] = dict(sources=provenance.source_sha(["silhouette.hip", "bucket.h", "kmeans.hip", "common.h", "cuda_gcn_amd/host/silhouette_query.cpp"]))
    line = json.dumps(res)
    print(line)
    if opts["--out"]:
        with open(opts["--out"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
