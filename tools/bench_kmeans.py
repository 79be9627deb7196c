"""k-means on the hidden layer of reddit-syn (hidden 128) at k = 41 and k = 256, HIP events — the figures of DESIGN §4.19:
  * the assign launch, the update launches and one seeding step (the difference of a 9-centre and a 1-centre seeding, over 8)
    of csrc/kmeans.hip timed apart on the model's own hidden matrix with its inverse norms;
  * each against its byte floor at the HBM rate (6.3 TB/s): assign reads n . h . 4 B, update the same plus n . 4, a seeding
    step n . h . 4 + 8 n; assign also against 2 . n . k . h FLOP at 155 TF (the exact-f32 MFMA; k rounded up to the tile of 64
    the kernel multiplies);
  * cluster() as a whole (wall time, 20 iterations at most) against one evaluation forward (eval(2), wall time with its
    synchronisation) and, where scikit-learn imports, against embed() plus sklearn.cluster.KMeans on the host (same k,
    k-means++, one initialisation, the same iteration cap);
  * with --parent DIR (a built checkout of the parent commit): `python bench.py --gpus 1 --steps 50 --warmup 10` in DIR and here,
    alternating --rounds times (default 2): the epoch path is meant not to move.
Prints one JSON line, with the hashes of the sources it measured (cuda_gcn_amd/provenance.py); --out FILE also writes it there.
None of the values is a pass/fail threshold.  usage: bench_kmeans.py [dataset] [hidden] [epochs] [--out FILE] [--parent DIR] [--rounds N]"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_gcn_amd import datagen, provenance
from cuda_gcn_amd.model import HipGCNModel, KEY_KMEANS
from cuda_gcn_amd.ops import Device, _ck

MFMA_F32_FLOPS, HBM_BYTES_S = 155e12, 6.3e12


def timeit(dev, fn, iters, warmup=1):
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
    print(f"bench_kmeans: {text}", file=sys.stderr, flush=True)


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
    N = ds["num_nodes"]
    res = dict(dataset=name, nodes=N, hidden=hidden, epochs=epochs, iters_cap=20)
    m = HipGCNModel(ds, seed=1, hidden_dim=hidden, dropout=0.5)
    m.run_epochs(epochs, want_trace=False)
    res["eval_forward_wall_ms"] = wall(lambda: m.eval(2))
    note(f"model trained; evaluation forward {res['eval_forward_wall_ms']:.3f} ms")
    try:
        from sklearn.cluster import KMeans
    except ImportError:
        KMeans = None
    for k in (41, 256):
        out = {}
        run = m.cluster(k=k, iters=20, report=False)
        out["cluster_wall_ms"] = wall(lambda: m.cluster(k=k, iters=20, report=False), reps=2)
        out["iters_run"], out["converged"], out["inertia"] = run["iters_run"], run["converged"], run["inertia"]
        if KMeans is not None:
            def host():
                return KMeans(n_clusters=k, init="k-means++", n_init=1, max_iter=20, random_state=0).fit(m.embed(normalize=True))
            t0 = time.perf_counter()
            fit = host()
            out["embed_plus_sklearn_wall_ms"] = 1e3 * (time.perf_counter() - t0)
            out["sklearn_inertia"], out["sklearn_iters"] = float(fit.inertia_), int(fit.n_iter_)
        res[f"k{k}"] = out
        note(f"cluster() at k = {k}: {out}")
    emb = m.embed()
    m.close()
    # ---- the launches themselves, on the same matrix
    dev = Device(0)
    lib = dev.lib
    table, inv = dev.buf(emb), dev.buf((N,), np.float32)
    _ck(lib, lib.gcnhip_embed_inv_norms(dev.ctx, table.ptr, hidden, N, hidden, inv.ptr), "inv_norms")
    bytes_table = N * hidden * 4.0
    for k in (41, 256):
        plan = dev.kmeans_plan(N, k, hidden)
        sbytes = max(plan["update_bytes"], plan["seed_bytes"])
        sb = dev.buf((sbytes // 4 + 4,), np.uint32)
        mb, cb, zb, pb = dev.buf((k, hidden), np.float32), dev.buf((k,), np.float32), dev.buf((k,), np.int32), dev.buf((k,), np.int32)
        ab, db, fb, ib = dev.buf((N,), np.int32), dev.buf((N,), np.float32), dev.buf((1,), np.int32), dev.buf((1,), np.float64)

        def seed(kk):
            _ck(lib, lib.gcnhip_kmeans_seed(dev.ctx, table.ptr, hidden, N, hidden, inv.ptr, None, N, kk, 1 ^ KEY_KMEANS, mb.ptr, hidden, pb.ptr, sb.ptr,
                                            plan["seed_bytes"]), "seed")

        def assign():
            _ck(lib, lib.gcnhip_kmeans_assign(dev.ctx, table.ptr, hidden, N, hidden, inv.ptr, None, N, mb.ptr, hidden, cb.ptr, k, None, ab.ptr, db.ptr,
                                              fb.ptr), "assign")

        def update(n=N):
            _ck(lib, lib.gcnhip_kmeans_update(dev.ctx, table.ptr, hidden, N, hidden, inv.ptr, None, n, ab.ptr, db.ptr, k, mb.ptr, hidden, zb.ptr, cb.ptr,
                                              ib.ptr, sb.ptr, plan["update_bytes"]), "update")
        seed(k)
        update(0)                                                 # the norms of the seeded centres
        assign()
        out = res[f"k{k}"]
        out["seed_step_ms"] = (timeit(dev, lambda: seed(9), 5) - timeit(dev, lambda: seed(1), 5)) / 8
        out["seed_all_ms"] = timeit(dev, lambda: seed(k), 2)
        seed(k); update(0); assign()
        out["assign_ms"] = timeit(dev, assign, 20)
        out["update_ms"] = timeit(dev, update, 20)
        kpad = -(-k // 64) * 64
        out["assign_floor_hbm_ms"] = 1e3 * bytes_table / HBM_BYTES_S
        out["assign_floor_flop_ms"] = 1e3 * 2.0 * N * kpad * hidden / MFMA_F32_FLOPS
        out["update_floor_hbm_ms"] = 1e3 * (bytes_table + 4.0 * N) / HBM_BYTES_S
        out["seed_step_floor_hbm_ms"] = 1e3 * (bytes_table + 8.0 * N) / HBM_BYTES_S
        out["assign_tflops"] = 2.0 * N * kpad * hidden / (out["assign_ms"] * 1e-3) / 1e12
        out["update_scratch_mb"] = plan["update_bytes"] / 2 ** 20
        note(f"launches at k = {k}: assign {out['assign_ms']:.4f} ms, update {out['update_ms']:.4f} ms, seeding step {out['seed_step_ms']:.4f} ms")
        for b in (sb, mb, cb, zb, pb, ab, db, fb, ib):
            b.free()
    table.free(); inv.free()
    dev.close()
    if opts["--parent"]:
        runs = epoch_path(opts["--parent"], int(opts["--rounds"]))
        res["epoch_path"] = dict(runs, parent_median=float(np.median(runs["parent"])), this_median=float(np.median(runs["this"])))
    res["_meta"] = dict(sources=provenance.source_sha(["kmeans.hip", "embed.hip", "common.h", "cuda_gcn_amd/host/kmeans.cpp"]))
    line = json.dumps(res)
    print(line)
    if opts["--out"]:
        with open(opts["--out"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
