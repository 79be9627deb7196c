"""Node-embedding queries on reddit-syn (hidden 128), HIP events — the figures of DESIGN §4.11:
  * similar() at k = 10 (cosine) for 1 024 queries and for every node: the product launches and the merge launches of
    gcnhip_topk_rows timed apart (its `launches` argument) and together, on the model's own hidden matrix;
  * each against one evaluation forward (eval(2), wall time with its synchronisation);
  * each against two floors from the chip's measured rates: 2 . nq . N . h FLOP at 155 TF (the exact-f32 MFMA), and the table's
    bytes once per query tile of 64 at the Infinity-Cache rate (8.6 TB/s) and at the HBM rate (6.3 TB/s);
  * embed() of 1 024 nodes against var(3), wall time.
Prints one JSON line.  None of the values is a pass/fail threshold.  usage: bench_embed.py [dataset] [hidden] [epochs]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_gcn_amd import datagen
from cuda_gcn_amd.model import HipGCNModel
from cuda_gcn_amd.ops import Device, _ck

MFMA_F32_FLOPS, CACHE_BYTES_S, HBM_BYTES_S = 155e12, 8.6e12, 6.3e12
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


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "reddit-syn"
    hidden = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    epochs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    ds = datagen.make_dataset(name)
    N = ds["num_nodes"]
    res = dict(dataset=name, nodes=N, hidden=hidden, epochs=epochs, k=10)
    m = HipGCNModel(ds, seed=1, hidden_dim=hidden, dropout=0.5)
    m.run_epochs(epochs, want_trace=False)
    res["eval_forward_wall_ms"] = wall(lambda: m.eval(2))
    q1024 = np.random.default_rng(0).integers(0, N, 1024).astype(np.int32)
    res["embed_1024_wall_ms"] = wall(lambda: m.embed(nodes=q1024))
    res["var3_wall_ms"] = wall(lambda: m.var(3), reps=3)
    res["similar_1024_wall_ms"] = wall(lambda: m.similar(q1024, k=10))
    res["similar_all_wall_ms"] = wall(lambda: m.similar(None, k=10), reps=2)
    emb = m.embed()
    m.close()
    # ---- the launches themselves, on the same matrix
    dev = Device(0)
    lib = dev.lib
    table = dev.buf(emb)
    inv = dev.buf((N,), np.float32)
    res["inv_norms_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_embed_inv_norms(dev.ctx, table.ptr, hidden, N, hidden, inv.ptr), "inv_norms"), 20)
    for label, q in (("1024", q1024), ("all", np.arange(N, dtype=np.int32))):
        nq = int(q.size)
        plan = dev.topk_plan(N, nq, 10)
        sbytes = max(min(plan["scratch_bytes"], SCRATCH_CAP), plan["scratch_bytes_min"])
        qb, sb = dev.buf(q), dev.buf((sbytes // 4,), np.uint32)
        ib, ob = dev.buf((nq * 10,), np.int32), dev.buf((nq * 10,), np.float32)

        def run(launches):
            _ck(lib, lib.gcnhip_topk_rows(dev.ctx, table.ptr, hidden, N, hidden, inv.ptr, None, qb.ptr, nq, 10, 1, 0, sb.ptr, sbytes, launches,
                                          ib.ptr, ob.ptr), "topk")
        iters = 20 if nq <= 4096 else 2
        tiles = -(-nq // 64)
        res[label] = dict(queries=nq, chunk_rows=plan["chunk_rows"], n_chunks=plan["n_chunks"], scratch_mb=sbytes / 2 ** 20,
                          batches=-(-plan["scratch_bytes"] // sbytes),
                          product_ms=timeit(dev, lambda: run(1), iters), merge_ms=timeit(dev, lambda: run(2), iters),
                          both_ms=timeit(dev, lambda: run(3), iters),
                          floor_flop_ms=1e3 * 2.0 * nq * N * hidden / MFMA_F32_FLOPS,
                          floor_cache_ms=1e3 * tiles * N * hidden * 4.0 / CACHE_BYTES_S,
                          floor_hbm_ms=1e3 * tiles * N * hidden * 4.0 / HBM_BYTES_S)
        res[label]["tflops"] = 2.0 * nq * N * hidden / (res[label]["product_ms"] * 1e-3) / 1e12
        for b in (qb, sb, ib, ob):
            b.free()
    table.free(); inv.free()
    dev.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
