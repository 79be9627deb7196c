"""The Gaussian mixture on the hidden layer of reddit-syn (hidden 128) at k = 41 and k = 256, HIP events — the figures of DESIGN §4.30:
  * over a 16 384-row sample, the test split and every row: the E-step launch (with the log joint written) of csrc/gmm.hip against
    gcnhip_kmeans_assign on the same rows at the same k and against the f32-MFMA floor 2 n k (2 h) / 157.3 TF; the M-step launches
    (the partials and their fold) against their byte floor (the log joint, the table and lse once at 6.3 TB/s) and the float64-MFMA
    floor 2 n k (1 + 2 h) / 78.6 TF (the product's published matrix rate);
  * gmm() as a whole (wall time, 8 192 nodes, k-means start, 20 iterations at most) against embed() plus scikit-learn's
    GaussianMixture(covariance_type="diag") on the host with the same cap, where scikit-learn imports;
  * with --parent DIR (a built checkout of the parent commit): `python bench.py --gpus 1 --steps 50 --warmup 10` in DIR and here,
    alternating --rounds times (default 3): the epoch path is meant not to move.
Prints one JSON line, with the hashes of the sources it measured (cuda_gcn_amd/provenance.py); --out FILE also writes it there.
None of the values is a pass/fail threshold.  usage: bench_gmm.py [dataset] [hidden] [epochs] [--out FILE] [--parent DIR] [--rounds N]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_kmeans import epoch_path, timeit, wall
from cuda_gcn_amd import datagen, provenance
from cuda_gcn_amd.model import HipGCNModel
from cuda_gcn_amd.ops import Device, _ck

MFMA_F32_FLOPS, MFMA_F64_FLOPS, HBM_BYTES_S = 157.3e12, 78.6e12, 6.3e12


def note(text):
    print(f"bench_gmm: {text}", file=sys.stderr, flush=True)


def launches(dev, emb, rows, k, out):
    """the E-step, the M-step and gcnhip_kmeans_assign on the listed rows of emb [N, h] with its inverse norms"""
    lib = dev.lib
    N, h = emb.shape
    n = int(rows.size)
    table, inv, rb = dev.buf(emb), dev.buf((N,), np.float32), dev.buf(np.ascontiguousarray(rows, np.int32))
    _ck(lib, lib.gcnhip_embed_inv_norms(dev.ctx, table.ptr, h, N, h, inv.ptr), "inv_norms")
    unit = emb[rows] / np.maximum(np.linalg.norm(emb[rows], axis=1, keepdims=True), 1e-30)
    shift = unit.mean(0, dtype=np.float64).astype(np.float32)
    mu = (unit[np.linspace(0, n - 1, k).astype(np.int64)] - shift).astype(np.float32)
    plan = dev.gmm_plan(n, k, h)
    hb, mb, vb, wb = dev.buf(shift), dev.buf(mu), dev.buf(np.full((k, h), 0.01, np.float32)), dev.buf(np.full(k, 1.0 / k, np.float32))
    pb, qb, cb = dev.buf((k, h), np.float32), dev.buf((k, h), np.float32), dev.buf((k,), np.float32)
    _ck(lib, lib.gcnhip_gmm_finalize(dev.ctx, None, n, k, h, 0, 1e-6, mb.ptr, vb.ptr, wb.ptr, pb.ptr, qb.ptr, h, cb.ptr), "finalize")
    lse, mr, ab, jb = dev.buf((n,), np.float32), dev.buf((n,), np.float32), dev.buf((n,), np.int32), dev.buf((n * k,), np.float32)
    ub, eb = dev.buf((1,), np.float64), dev.buf((plan["estep_bytes"] // 4 + 4,), np.uint32)
    sums, sb = dev.buf((k * (1 + 2 * h),), np.float64), dev.buf((plan["mstep_bytes"] // 4 + 4,), np.uint32)
    cn, zb, db, fb = dev.buf((k,), np.float32), dev.buf((k,), np.int32), dev.buf((n,), np.float32), dev.buf((2,), np.int32)
    kplan = dev.kmeans_plan(n, k, h)
    kb = dev.buf((kplan["update_bytes"] // 4 + 4,), np.uint32)
    centres = dev.buf(np.ascontiguousarray(mu + shift))

    def estep():
        _ck(lib, lib.gcnhip_gmm_estep(dev.ctx, table.ptr, h, N, h, inv.ptr, rb.ptr, n, hb.ptr, pb.ptr, qb.ptr, h, cb.ptr, k, lse.ptr, ab.ptr, mr.ptr, jb.ptr,
                                      ub.ptr, eb.ptr, plan["estep_bytes"]), "estep")

    def mstep():
        _ck(lib, lib.gcnhip_gmm_mstep(dev.ctx, table.ptr, h, N, h, inv.ptr, rb.ptr, n, hb.ptr, jb.ptr, lse.ptr, None, k, 0, n, sums.ptr, sb.ptr,
                                      plan["mstep_bytes"]), "mstep")

    def assign():
        _ck(lib, lib.gcnhip_kmeans_assign(dev.ctx, table.ptr, h, N, h, inv.ptr, rb.ptr, n, centres.ptr, h, cn.ptr, k, None, ab.ptr, db.ptr, fb.ptr), "assign")
    _ck(lib, lib.gcnhip_kmeans_update(dev.ctx, table.ptr, h, N, h, inv.ptr, rb.ptr, 0, None, None, k, centres.ptr, h, zb.ptr, cn.ptr, None, kb.ptr,
                                      kplan["update_bytes"]), "update")
    estep()
    out["estep_ms"], out["mstep_ms"], out["kmeans_assign_ms"] = timeit(dev, estep, 10), timeit(dev, mstep, 10), timeit(dev, assign, 10)
    out["estep_floor_mfma_ms"] = 1e3 * 2.0 * n * k * 2 * h / MFMA_F32_FLOPS
    out["estep_tflops"] = 2.0 * n * k * 2 * h / (out["estep_ms"] * 1e-3) / 1e12
    out["mstep_floor_hbm_ms"] = 1e3 * 4.0 * (n * k + n * h + n) / HBM_BYTES_S
    out["mstep_floor_mfma_f64_ms"] = 1e3 * 2.0 * n * k * (1 + 2 * h) / MFMA_F64_FLOPS
    out["mstep_scratch_mb"] = plan["mstep_bytes"] / 2 ** 20
    for b in (table, inv, rb, hb, mb, vb, wb, pb, qb, cb, lse, mr, ab, jb, ub, eb, sums, sb, cn, zb, db, fb, kb, centres):
        b.free()


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
    res = dict(dataset=name, nodes=N, hidden=hidden, epochs=epochs, iters_cap=20, whole_rows=8192)
    m = HipGCNModel(ds, seed=1, hidden_dim=hidden, dropout=0.5)
    m.run_epochs(epochs, want_trace=False)
    nodes = np.arange(min(8192, N), dtype=np.int32)
    try:
        from sklearn.mixture import GaussianMixture
    except ImportError:
        GaussianMixture = None
    for k in (41, 256):
        out = {}
        fit = m.gmm(k, nodes=nodes, iters=20, report=False)
        out["gmm_wall_ms"] = wall(lambda: m.gmm(k, nodes=nodes, iters=20, report=False), reps=2)
        out["iters_run"], out["converged"], out["lower_bound"] = fit["iters_run"], fit["converged"], fit["lower_bound"]
        if GaussianMixture is not None:
            t0 = time.perf_counter()
            host = GaussianMixture(k, covariance_type="diag", max_iter=20, random_state=0).fit(m.embed(normalize=True)[nodes])
            out["embed_plus_sklearn_wall_ms"] = 1e3 * (time.perf_counter() - t0)
            out["sklearn_lower_bound"], out["sklearn_iters"] = float(host.lower_bound_), int(host.n_iter_)
        res[f"k{k}"] = out
        note(f"gmm() at k = {k}: {out}")
    emb = m.embed()
    test = np.flatnonzero(np.asarray(ds["split"]) == 3).astype(np.int32)
    m.close()
    dev = Device(0)
    lists = dict(sample=np.sort(np.random.default_rng(0).choice(N, min(16384, N), replace=False)).astype(np.int32), test=test,
                 all=np.arange(N, dtype=np.int32))
    for k in (41, 256):
        for label, rows in lists.items():
            out = dict(rows=int(rows.size))
            launches(dev, emb, rows, k, out)
            res[f"k{k}"][label] = out
            note(f"launches at k = {k}, {label}: {out}")
    dev.close()
    if opts["--parent"]:
        runs = epoch_path(opts["--parent"], int(opts["--rounds"]))
        res["epoch_path"] = dict(runs, parent_median=float(np.median(runs["parent"])), this_median=float(np.median(runs["this"])))
    res["_meta"] = dict(sources=provenance.source_sha(["gmm.hip", "kmeans.hip", "embed.hip", "common.h", "cuda_gcn_amd/host/gmm_query.cpp"]))
    line = json.dumps(res)
    print(line)
    if opts["--out"]:
        with open(opts["--out"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
