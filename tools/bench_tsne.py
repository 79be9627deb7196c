"""Exact t-SNE on the hidden layer of reddit-syn (hidden 128), HIP events — the figures of DESIGN §4.24:
  * on the model's own hidden matrix with its inverse norms, over a 16 384-row sample and over the test split: one gradient
    launch (gcnhip_tsne_gradient, without and with the KL terms), the small launch of an iteration (gcnhip_tsne_update), the
    bandwidth call and the pack, with the scratch cap tsne() uses;
  * the gradient launch against 2 . n^2 . h FLOP at 157.3 TF (the exact-f32 MFMA) and against gcnhip_silhouette_sums (k = 41, the
    labels of a cluster() run) on the same rows: silhouette.hip is the parent commit's, unchanged;
  * tsne() as a whole (wall time) on an 8 192-row node query against embed() plus scikit-learn's exact t-SNE on the host, where it
    imports and with --sklearn (it takes minutes), and the 10-neighbour label share of both maps;
  * with --parent DIR (a built checkout of the parent commit): bench.py in DIR and here, alternating --rounds times.
Prints one JSON line with the hashes of the sources it measured; --out FILE also writes it there.  None of the values is a
pass/fail threshold.  usage: bench_tsne.py [dataset] [hidden] [epochs] [--out FILE] [--parent DIR] [--rounds N] [--iters N] [--sklearn]"""
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

MFMA_F32_FLOPS = 157.3e12
SCRATCH_CAP = 256 << 20                                           # ModelQueries::TSNE_SCRATCH_DEFAULT


def note(text):
    print(f"bench_tsne: {text}", file=sys.stderr, flush=True)


def label_share(y, labels, k=10, block=1024):
    hits = 0
    for i in range(0, y.shape[0], block):
        d = ((y[i:i + block, None, :] - y[None, :, :]) ** 2).sum(axis=2)
        d[np.arange(d.shape[0]), np.arange(i, i + d.shape[0])] = np.inf
        hits += (labels[np.argpartition(d, k, axis=1)[:, :k]] == labels[i:i + block, None]).sum()
    return float(hits) / (y.shape[0] * k)


def main():
    args = sys.argv[1:]
    use_sklearn = "--sklearn" in args
    args = [a for a in args if a != "--sklearn"]
    opts = {"--parent": None, "--rounds": "2", "--out": None, "--iters": "1000"}
    for flag in list(opts):
        if flag in args:
            i = args.index(flag)
            opts[flag] = args[i + 1]
            del args[i:i + 2]
    name = args[0] if len(args) > 0 else "reddit-syn"
    hidden = int(args[1]) if len(args) > 1 else 128
    epochs = int(args[2]) if len(args) > 2 else 5
    ds = datagen.make_dataset(name)
    N, truth = ds["num_nodes"], np.asarray(ds["label"])
    res = dict(dataset=name, nodes=N, hidden=hidden, epochs=epochs, iters=int(opts["--iters"]))
    m = HipGCNModel(ds, seed=1, hidden_dim=hidden, dropout=0.5)
    m.run_epochs(epochs, want_trace=False)
    assign = m.cluster(k=41, iters=20, report=False)["assign"]
    rng = np.random.default_rng(0)
    lists = dict(sample_16384=np.sort(rng.choice(N, min(16384, N), replace=False)).astype(np.int32),
                 test_split=np.flatnonzero(np.asarray(ds["split"]) == 3).astype(np.int32))
    # ---- the query as a whole, against the host
    q = np.sort(rng.choice(N, min(8192, N), replace=False)).astype(np.int32)
    t0 = time.perf_counter()
    whole = m.tsne(nodes=q, iters=res["iters"])
    out = dict(rows=int(q.size), tsne_wall_ms=1e3 * (time.perf_counter() - t0), kl=whole["kl"], unconverged=whole["unconverged"],
               label_share_10=label_share(whole["coords"].astype(np.float64), truth[q]),
               pca_label_share_10=label_share(m.pca(k=2, nodes=q)["coords"].astype(np.float64), truth[q]))
    if use_sklearn:
        try:
            from sklearn.manifold import TSNE
            t0 = time.perf_counter()
            host = TSNE(method="exact", init="pca", max_iter=res["iters"]).fit_transform(m.embed(nodes=q, normalize=True))
            out.update(embed_plus_sklearn_wall_ms=1e3 * (time.perf_counter() - t0), sklearn_label_share_10=label_share(host.astype(np.float64), truth[q]))
        except (ImportError, TypeError) as e:
            out["sklearn"] = repr(e)
    res["query_8192"] = out
    note(f"tsne() on {q.size} rows: {out}")
    emb = m.embed()
    m.close()
    # ---- the launches themselves, on the same matrix
    dev = Device(0)
    lib = dev.lib
    inv = dev.embed_inv_norms(emb)
    table, invb = dev.buf(emb), dev.buf(inv)
    for what, rows in lists.items():
        n = int(rows.size)
        plan = dev.tsne_plan(n, hidden)
        sbytes = max(min(plan["bytes"], SCRATCH_CAP), plan["bytes_min"])
        pk = dev.tsne_pack(emb, rows=rows, inv_norm=inv, scratch_bytes=sbytes)
        dev.tsne_bandwidths(pk, 30.0)
        y = dev.buf((1e-2 * rng.standard_normal((n, 2))).astype(np.float32))
        sums, state = dev.buf((n * 9,), np.float64), dev.buf(np.ones(6 * n, np.float64))
        beta, invz, mm, cnt = dev.buf((n,), np.float64), dev.buf((n,), np.float64), dev.buf((n,), np.float32), dev.buf((2,), np.int32)
        rb, lb = dev.buf(rows), dev.buf(np.ascontiguousarray(assign[rows], np.int32))
        splan = dev.silhouette_plan(n, 41, hidden)
        sil_bytes = max(min(splan["bytes"], SCRATCH_CAP), splan["bytes_min"])
        ssb, ub, zb = dev.buf((sil_bytes // 4 + 4,), np.uint32), dev.buf((n * 41,), np.float64), dev.buf((41,), np.int32)
        pp, sp = pk["pack"].ptr, pk["scratch"].ptr

        def grad(kl=0):
            _ck(lib, lib.gcnhip_tsne_gradient(dev.ctx, pp, n, hidden, y.ptr, 2, kl, sums.ptr, sp, sbytes), "gradient")

        def update():
            _ck(lib, lib.gcnhip_tsne_update(dev.ctx, pp, n, hidden, 2, sums.ptr, 1.0, 0.8, 0.0, 1, state.ptr, y.ptr, None, None), "update")

        def bandwidths():
            _ck(lib, lib.gcnhip_tsne_bandwidths(dev.ctx, pp, n, hidden, pk["points"], 30.0, beta.ptr, mm.ptr, invz.ptr, cnt.ptr, sp, sbytes), "bandwidths")

        def pack():
            _ck(lib, lib.gcnhip_tsne_pack(dev.ctx, table.ptr, hidden, N, hidden, invb.ptr, rb.ptr, n, pp, plan["pack_bytes"], cnt.ptr + 4), "pack")

        def silhouette():
            _ck(lib, lib.gcnhip_silhouette_sums(dev.ctx, table.ptr, hidden, N, hidden, invb.ptr, rb.ptr, n, lb.ptr, 41, ub.ptr, zb.ptr, ssb.ptr, sil_bytes),
                "silhouette")
        out = dict(rows=n, scratch_mb=sbytes / 2 ** 20, full_scratch_mb=plan["bytes"] / 2 ** 20)
        out["gradient_ms"] = timeit(dev, grad, 10)
        out["gradient_with_kl_ms"] = timeit(dev, lambda: grad(1), 5)
        out["update_ms"] = timeit(dev, update, 10)                # lr = 0: y stays where it is
        out["bandwidths_ms"] = timeit(dev, bandwidths, 3)
        out["pack_ms"] = timeit(dev, pack, 10)
        out["silhouette_sums_ms"] = timeit(dev, silhouette, 10)
        out["gradient_floor_flop_ms"] = 1e3 * 2.0 * n * n * hidden / MFMA_F32_FLOPS
        out["gradient_fraction_of_mfma_floor"] = out["gradient_floor_flop_ms"] / out["gradient_ms"]
        out["gradient_over_silhouette"] = out["gradient_ms"] / out["silhouette_sums_ms"]
        res[what] = out
        note(f"{what}: {out}")
    dev.close()
    if opts["--parent"]:
        runs = epoch_path(opts["--parent"], int(opts["--rounds"]))
        res["epoch_path"] = dict(runs, parent_median=float(np.median(runs["parent"])), this_median=float(np.median(runs["this"])))
    res["_meta"] = dict(sources=provenance.source_sha(["tsne.hip", "silhouette.hip", "bucket.h", "common.h", "cuda_gcn_amd/host/tsne_query.cpp"]))
    line = json.dumps(res)
    print(line)
    if opts["--out"]:
        with open(opts["--out"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
