"""DBSCAN on the hidden layer of reddit-syn (hidden 128), HIP events — the figures of DESIGN §4.25:
  * on the model's own hidden matrix with its inverse norms, over a 16 384-row sample and over the test split: the COUNT launch
    (gcnhip_dbscan_counts) at 1 and at 8 radii, one LINK round (gcnhip_dbscan_link), the labels launch; one warm-up, the mean of 10;
  * the COUNT launch against the exact-f32 MFMA floor of HALF the square, n^2 . h FLOP at 157.3 TF, and against the t-SNE gradient
    launch (gcnhip_tsne_gradient: the whole square and a heavy epilogue) on the same pack in the same process;
  * dbscan() as a whole with its rounds (wall time) on the same lists, and on an 8 192-row node query against embed() plus
    scikit-learn's DBSCAN(algorithm="brute") on the host, where it imports, with whether the labels are equal;
  * with --parent DIR (a built checkout of the parent commit): bench.py in DIR and here, alternating --rounds times.
eps is the radius at which a sampled row has --neighbours neighbours in the median (default 20), from neighbor_counts over a sweep.
Prints one JSON line with the hashes of the sources it measured; --out FILE also writes it there.  None of the values is a
pass/fail threshold.  usage: bench_dbscan.py [dataset] [hidden] [epochs] [--out FILE] [--parent DIR] [--rounds N] [--neighbours K]"""
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
SWEEP = np.array([0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.6, 0.8])


def note(text):
    print(f"bench_dbscan: {text}", file=sys.stderr, flush=True)


def main():
    args = sys.argv[1:]
    opts = {"--parent": None, "--rounds": "2", "--out": None, "--neighbours": "20"}
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
    # ---- the radius: one walk prices the sweep
    q = np.sort(rng.choice(N, min(8192, N), replace=False)).astype(np.int32)
    med = np.median(m.neighbor_counts(SWEEP, nodes=lists["sample_16384"]), axis=1)
    eps = float(SWEEP[min(int(np.searchsorted(med, float(opts["--neighbours"]))), SWEEP.size - 1)])
    res.update(eps=eps, sweep=SWEEP.tolist(), sweep_median_neighbours=med.tolist())
    note(f"median neighbours over the sweep {med.tolist()}: eps = {eps}")
    # ---- the query as a whole
    for what, rows in list(lists.items()) + [("query_8192", q)]:
        t0 = time.perf_counter()
        whole = m.dbscan(eps, nodes=rows, report=False)
        res["dbscan_" + what] = dict(rows=int(rows.size), wall_ms=1e3 * (time.perf_counter() - t0),
                                     **{k: whole[k] for k in ("n_clusters", "n_core", "n_border", "n_noise", "rounds")})
        note(f"dbscan() on {what}: {res['dbscan_' + what]}")
    try:
        from sklearn.cluster import DBSCAN
        t0 = time.perf_counter()
        host = DBSCAN(eps=eps, min_samples=5, algorithm="brute").fit(m.embed(nodes=q, normalize=True)).labels_
        res["dbscan_query_8192"].update(embed_plus_sklearn_wall_ms=1e3 * (time.perf_counter() - t0),
                                        labels_differ=int((host != whole["labels"]).sum()))
    except ImportError as e:
        res["dbscan_query_8192"]["sklearn"] = repr(e)
    note(f"against the host: {res['dbscan_query_8192']}")
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
        dev.tsne_bandwidths(pk, 30.0)
        y, sums = dev.buf((1e-2 * rng.standard_normal((n, 2))).astype(np.float32)), dev.buf((n * 9,), np.float64)
        state_bytes = dev.dbscan_plan(n, hidden)["state_bytes"]
        cnt, state, flag = dev.buf((8 * n,), np.int32), dev.buf((state_bytes // 4,), np.uint32), dev.buf((1,), np.int32)
        lab, core, sizes, tot = dev.buf((n,), np.int32), dev.buf((n,), np.uint8), dev.buf((n,), np.int32), dev.buf((5,), np.int32)
        pp = pk["pack"].ptr
        one, eight = np.array([eps]), np.ascontiguousarray(SWEEP)

        def count(e):
            _ck(lib, lib.gcnhip_dbscan_counts(dev.ctx, pp, n, hidden, e.ctypes.data, int(e.size), cnt.ptr), "counts")

        def link():
            _ck(lib, lib.gcnhip_dbscan_link(dev.ctx, pp, n, hidden, eps, state.ptr, state_bytes, flag.ptr), "link")

        def labels():
            _ck(lib, lib.gcnhip_dbscan_labels(dev.ctx, pp, n, hidden, state.ptr, state_bytes, lab.ptr, core.ptr, sizes.ptr, tot.ptr), "labels")

        def gradient():
            _ck(lib, lib.gcnhip_tsne_gradient(dev.ctx, pp, n, hidden, y.ptr, 2, 0, sums.ptr, pk["scratch"].ptr, sbytes), "gradient")
        out = dict(rows=n)
        out["count_e8_ms"] = timeit(dev, lambda: count(eight), 10)
        out["count_e1_ms"] = timeit(dev, lambda: count(one), 10)
        _ck(lib, lib.gcnhip_dbscan_cores(dev.ctx, pp, n, hidden, cnt.ptr, 5, state.ptr, state_bytes), "cores")
        out["link_round_ms"] = timeit(dev, link, 10)                # the warm-up and the first rounds hook; the later ones find nothing to do
        out["labels_ms"] = timeit(dev, labels, 10)
        out["tsne_gradient_ms"] = timeit(dev, gradient, 10)
        out["count_floor_flop_ms"] = 1e3 * n * n * hidden / MFMA_F32_FLOPS
        out["count_fraction_of_mfma_floor"] = out["count_floor_flop_ms"] / out["count_e1_ms"]
        out["count_over_tsne_gradient"] = out["count_e1_ms"] / out["tsne_gradient_ms"]
        out["count_e8_over_e1"] = out["count_e8_ms"] / out["count_e1_ms"]
        res[what] = out
        note(f"{what}: {out}")
    dev.close()
    if opts["--parent"]:
        runs = epoch_path(opts["--parent"], int(opts["--rounds"]))
        res["epoch_path"] = dict(runs, parent_median=float(np.median(runs["parent"])), this_median=float(np.median(runs["this"])))
    res["_meta"] = dict(sources=provenance.source_sha(["dbscan.hip", "tsne.hip", "tsne_pack.h", "bucket.h", "common.h", "cuda_gcn_amd/host/dbscan_query.cpp"]))
    line = json.dumps(res)
    print(line)
    if opts["--out"]:
        with open(opts["--out"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
