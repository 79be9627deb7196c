"""Explanation queries on reddit-syn (hidden 128), HIP events — the figures of DESIGN §4.12:
  * explain() for 1 024 nodes and for the test split (wall time, forward and copies included), beside one evaluation forward;
  * the entry points themselves on the model's own hidden matrix and weights: gcnhip_explain_hops and gcnhip_explain_features_agg
    timed apart (`*_call_ms`), and the device-to-host copy of the feature shares.  A call is not the kernel alone: each entry point
    first copies its query lists to the host and waits for the stream (two blocking copies, three for hops) before it launches.
    `query_check_ms` times those copies by themselves, and `*_kernel_ms` = call - check is what to hold against the floors;
  * the floors of the features launch from the chip's measured rates: 2 . sum(d) . F . h FLOP at 155 TF (the f32 vector / exact-f32
    MFMA rate) and sum(d) . F . 4 gathered bytes at the Infinity-Cache rate (8.6 TB/s) and at the HBM rate (6.3 TB/s).
  * with --parent DIR (a built checkout of the parent commit): `python bench.py --gpus 1 --steps 50 --warmup 10` in DIR and here,
    alternating, --rounds times each (default 2), to show the epoch path untouched.
The S table of the timed launch is A^.X of the unscaled X (the launch's time does not depend on the values).  Prints one JSON line.
None of the values is a pass/fail threshold.  usage: bench_explain.py [dataset] [hidden] [epochs] [--parent DIR] [--rounds N]"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_gcn_amd import datagen
from cuda_gcn_amd.model import HipGCNModel
from cuda_gcn_amd.ops import Device, Feat, _ck

F32_FLOPS, CACHE_BYTES_S, HBM_BYTES_S = 155e12, 8.6e12, 6.3e12
SCRATCH_CAP = 64 << 20                                            # ModelQueries::EMBED_SCRATCH_CAP


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


def wall(fn, reps=5):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def epoch_path(parent, rounds):
    """bench.py on the parent checkout and on this one, alternating: epochs/s of every run"""
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = dict(parent=[], this=[])
    for _ in range(rounds):
        for label, root in (("parent", parent), ("this", here)):
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "50", "--warmup", "10"], cwd=root, capture_output=True, text=True,
                               timeout=600, check=True)
            out[label].append(json.loads(r.stdout.strip().splitlines()[-1])["value"])
    return out


def main():
    args = sys.argv[1:]
    parent, rounds = None, 2
    for flag in ("--parent", "--rounds"):
        if flag in args:
            i = args.index(flag)
            value = args[i + 1]
            del args[i:i + 2]
            parent, rounds = (value, rounds) if flag == "--parent" else (parent, int(value))
    name = args[0] if len(args) > 0 else "reddit-syn"
    hidden = int(args[1]) if len(args) > 1 else 128
    epochs = int(args[2]) if len(args) > 2 else 5
    ds = datagen.make_dataset(name)
    N, nf, nc = ds["num_nodes"], ds["input_dim"], ds["output_dim"]
    res = dict(dataset=name, nodes=N, features=nf, hidden=hidden, classes=nc, epochs=epochs)
    m = HipGCNModel(ds, seed=1, hidden_dim=hidden, dropout=0.5)
    m.run_epochs(epochs, want_trace=False)
    factored = bool(m.row_scale()[1])
    res["eval_forward_wall_ms"] = wall(lambda: m.eval(2))
    q1024 = np.random.default_rng(0).integers(0, N, 1024).astype(np.int32)
    test = np.flatnonzero(ds["split"] == 3).astype(np.int32)
    res["explain_1024_wall_ms"] = wall(lambda: m.explain(q1024))
    res["explain_1024_no_features_wall_ms"] = wall(lambda: m.explain(q1024, features=False))
    res["explain_test_wall_ms"] = wall(lambda: m.explain(test), reps=2)
    res["feature_importance_test_wall_ms"] = wall(lambda: m.feature_importance(split=3), reps=2)
    classes = m.explain(test, features=False)["classes"]
    emb, w1, w2 = m.embed(), m.var(2), m.var(5)
    m.close()
    # ---- the launches themselves, on the same hidden matrix and weights
    dev = Device(0)
    lib = dev.lib
    g = dev.graph(ds["g_indptr"], ds["g_indices"])
    lens = np.diff(g.csr()[0]).astype(np.int64)
    xf = dev.feat(ds["f_indptr"], ds["f_indices"], ds["f_val"], nf)
    agg = Feat.aggregated(dev, g, xf)
    h1b, w1b, w2b = dev.buf(emb), dev.buf(w1), dev.buf(w2)
    for label, q, cls in (("1024", q1024, classes[np.arange(1024) % classes.size]), ("test", test, classes)):
        nq = int(q.size)
        ptr = np.concatenate([[0], np.cumsum(lens[q])])
        total = int(ptr[-1])
        qb, cb, pb = dev.buf(q), dev.buf(np.ascontiguousarray(cls, np.int32)), dev.buf(ptr[:nq].astype(np.int32))
        lb, hb = dev.buf((nq,), np.float32), dev.buf((nq, hidden), np.float32)
        rb, vb = dev.buf((max(total, 1),), np.int32), dev.buf((max(total, 1),), np.float32)
        batch = max(1, min(nq, SCRATCH_CAP // (nf * 4)))
        fb = dev.buf((batch, nf), np.float32)
        host = np.empty((batch, nf), np.float32)

        def hops():
            _ck(lib, lib.gcnhip_explain_hops(dev.ctx, g.h, qb.ptr, cb.ptr, nq, h1b.ptr, hidden, hidden, w2b.ptr, nc, nc, int(factored), lb.ptr, hb.ptr, hidden,
                                             pb.ptr, rb.ptr, vb.ptr, total), "hops")

        def features():
            for q0 in range(0, nq, batch):
                nb = min(batch, nq - q0)
                _ck(lib, lib.gcnhip_explain_features_agg(dev.ctx, g.h, qb.ptr + 4 * q0, cb.ptr + 4 * q0, nb, h1b.ptr, hidden, hidden, w2b.ptr, nc, nc, w1b.ptr,
                                                         hidden, nf, agg.values_ptr, nf, int(factored), fb.ptr, nf), "features_agg")

        def copy():
            _ck(lib, lib.gcnhip_d2h(dev.ctx, host.ctypes.data, fb.ptr, host.nbytes), "d2h")
        lists = np.empty(nq, np.int32)

        def check(copies):                                        # what an entry point does before it launches
            def run():
                for q0 in range(0, nq, batch if copies == 2 else nq):
                    nb = min(batch, nq - q0) if copies == 2 else nq
                    for _ in range(copies):
                        _ck(lib, lib.gcnhip_d2h(dev.ctx, lists.ctypes.data, qb.ptr + 4 * q0, 4 * nb), "d2h")
            return run
        iters = 10 if nq <= 4096 else 2
        sum_d = float(lens[q].sum())
        r = dict(queries=nq, sum_d=sum_d, batches=-(-nq // batch), hops_call_ms=timeit(dev, hops, iters), hops_query_check_ms=timeit(dev, check(3), iters),
                 features_agg_call_ms=timeit(dev, features, iters), features_agg_query_check_ms=timeit(dev, check(2), iters),
                 copy_of_one_batch_wall_ms=wall(copy, reps=3), floor_flop_ms=1e3 * 2.0 * sum_d * nf * hidden / F32_FLOPS,
                 floor_cache_ms=1e3 * sum_d * nf * 4.0 / CACHE_BYTES_S, floor_hbm_ms=1e3 * sum_d * nf * 4.0 / HBM_BYTES_S)
        r["hops_kernel_ms"] = r["hops_call_ms"] - r["hops_query_check_ms"]
        r["features_agg_kernel_ms"] = r["features_agg_call_ms"] - r["features_agg_query_check_ms"]
        r["features_tflops"] = 2.0 * sum_d * nf * hidden / (r["features_agg_kernel_ms"] * 1e-3) / 1e12
        res[label] = r
        for b in (qb, cb, pb, lb, hb, rb, vb, fb):
            b.free()
    dev.close()
    if parent:
        res["epochs_per_s"] = epoch_path(parent, rounds)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
