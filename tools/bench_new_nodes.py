"""Prediction for unseen nodes on reddit-syn (hidden 128) — the figures of DESIGN §4.17:
  * predict_new_nodes() for m = 1, 1 024 and 65 536 new nodes whose lists have the dataset's mean length (wall time: host plan,
    copies, the forward, every launch), and for one new node that lists 10 000 ids; beside predict(nodes=q) for 1 024 nodes, one
    evaluation forward, and what the only alternative costs today (the model built again on the augmented dataset);
  * the parts of a call through the C-ABI on tables of the model's shapes, HIP events: the feature object of X_new (wall), the two
    first-layer products (X_new . W1; X . W1 of the dataset nodes, which an aggregate-first model runs for this query alone), the
    two gcnhip_attach_gather launches (hidden width with ReLU, class width with the predict epilogue), the small product
    h . W2, and the copies (row lists in, results out; wall);
  * for the gathers, the bytes they read — per edge one table row, its index and its coefficient — at the rate the model's own
    hidden-width aggregation (gcnhip_graphsum over the dataset's adjacency) achieves in the same process;
  * with --parent DIR (a built checkout of the parent commit): `python bench.py --gpus 1 --steps 50 --warmup 10` in DIR and here,
    alternating, --rounds times each (default 2), to show the epoch path untouched.
Prints one JSON line.  None of the values is a pass/fail threshold.
usage: bench_new_nodes.py [dataset] [hidden] [epochs] [--parent DIR] [--rounds N] [--no-rebuild]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_gcn_amd import datagen
from cuda_gcn_amd.model import HipGCNModel, new_node_rows
from cuda_gcn_amd.ops import Device, _ck
from tools.bench_explain import timeit, wall, epoch_path

HUB = 10000


def row_ld(dim):                                                  # HipVariable's rule
    return (dim + 3) // 4 * 4 if dim <= 32 else (dim + 15) // 16 * 16


def new_batch(ds, m, mean_len, hub, seed):
    """m new nodes: dense feature rows = scaled copies of dataset rows, lists of about mean_len ids in [0, N + m); hub: row 0 lists HUB ids"""
    rng = np.random.default_rng(seed)
    N, F = ds["num_nodes"], ds["input_dim"]
    x = ds["f_val"].reshape(N, F)[rng.integers(0, N, m)] * rng.uniform(0.5, 1.5, (m, 1)).astype(np.float32)
    length = rng.poisson(mean_len, m)
    if hub:
        length[0] = HUB
    ptr = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    ids = rng.integers(0, N + m, int(ptr[-1])).astype(np.int32)
    return np.ascontiguousarray(x, np.float32), ptr, ids


def main():
    args = sys.argv[1:]
    parent, rounds, rebuild = None, 2, True
    if "--no-rebuild" in args:
        args.remove("--no-rebuild")
        rebuild = False
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
    N, F, nc = ds["num_nodes"], ds["input_dim"], ds["output_dim"]
    gp = ds["g_indptr"]
    mean_len = float(gp[-1]) / N - 1.0
    res = dict(dataset=name, nodes=N, features=F, hidden=hidden, classes=nc, epochs=epochs, mean_listed=mean_len)
    t0 = time.perf_counter()
    m = HipGCNModel(ds, seed=1, hidden_dim=hidden, dropout=0.5)
    res["model_build_wall_ms"] = 1e3 * (time.perf_counter() - t0)
    m.run_epochs(epochs, want_trace=False)
    factored = bool(m.row_scale()[1])
    res["factored"] = factored
    res["eval_forward_wall_ms"] = wall(lambda: m.eval(2))
    q1024 = np.random.default_rng(0).integers(0, N, 1024).astype(np.int32)
    res["predict_1024_wall_ms"] = wall(lambda: m.predict(nodes=q1024))
    batches = {}
    for label, mm, hub in (("1", 1, False), ("1_hub", 1, True), ("1024", 1024, True), ("65536", 65536, True)):
        batches[label] = new_batch(ds, mm, mean_len, hub, seed=mm + hub)
        x, ptr, ids = batches[label]
        res[f"predict_new_{label}_wall_ms"] = wall(lambda: m.predict_new_nodes(x, ptr, ids), reps=3)
        res[f"host_plan_{label}_wall_ms"] = wall(lambda: new_node_rows(gp, ptr, ids, factored=factored), reps=3)
    w1, w2 = m.var(2), m.var(5)
    m.close()
    if rebuild:                                                   # today's only way to score a new node: the dataset and the model again
        x, ptr, ids = batches["1024"]
        t0 = time.perf_counter()
        aug = dict(ds)
        rows = [np.concatenate([[N + i], ids[ptr[i]:ptr[i + 1]]]) for i in range(1024)]
        aug.update(num_nodes=N + 1024, g_indptr=np.concatenate([gp, gp[-1] + np.cumsum([len(r) for r in rows])]).astype(np.int32),
                   g_indices=np.concatenate([ds["g_indices"]] + rows).astype(np.int32),
                   f_indptr=(np.arange(N + 1025, dtype=np.int64) * F).astype(np.int32), f_indices=np.tile(np.arange(F, dtype=np.int32), N + 1024),
                   f_val=np.concatenate([ds["f_val"], x.ravel()]), split=np.concatenate([ds["split"], np.zeros(1024, np.int32)]),
                   label=np.concatenate([ds["label"], np.zeros(1024, np.int32)]))
        res["rebuild_arrays_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        m2 = HipGCNModel(aug, seed=1, hidden_dim=hidden, dropout=0.5)
        m2.set_weights(w1, w2)
        m2.predict(nodes=np.arange(N, N + 1024, dtype=np.int32))
        res["rebuild_model_and_predict_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        m2.close()
    # ---- the parts, on tables of the model's shapes (their values do not change a launch's time)
    dev = Device(0)
    lib = dev.lib
    rng = np.random.default_rng(5)
    ld_h, ld_c = row_ld(hidden), row_ld(nc)
    ta_h, ta_c = dev.buf(rng.standard_normal((N, ld_h)).astype(np.float32)), dev.buf(rng.standard_normal((N, ld_c)).astype(np.float32))
    w1b, w2b = dev.padded(w1, ld_h), dev.padded(w2, ld_c)
    x_all = dev.feat(ds["f_indptr"], ds["f_indices"], ds["f_val"], F)
    g = dev.graph(gp, ds["g_indices"])
    out_all = dev.buf((N, ld_h), np.float32)
    res["dataset_first_layer_product_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_spmm_fwd(dev.ctx, x_all.h, x_all.values_ptr, w1b.ptr, ld_h, out_all.ptr, ld_h, hidden,
                                                                                             0.0, 0, None, 0, None), "spmm_fwd"), 5)
    agg_ms = timeit(dev, lambda: _ck(lib, lib.gcnhip_graphsum(dev.ctx, g.h, ta_h.ptr, ld_h, out_all.ptr, ld_h, hidden), "graphsum"), 5)
    agg_bytes = float(gp[-1]) * (hidden * 4 + 8)
    res["hidden_aggregation_ms"], res["hidden_aggregation_TBps"] = agg_ms, agg_bytes / (agg_ms * 1e-3) / 1e12
    for label in ("1", "1_hub", "1024", "65536"):
        x, ptr, ids = batches[label]
        mm = x.shape[0]
        t0 = time.perf_counter()
        rows = new_node_rows(gp, ptr, ids, factored=factored)
        plan_ms = 1e3 * (time.perf_counter() - t0)
        nnz = int(rows["ptr"][-1])
        host_in = [rows["ptr"], rows["col"], rows["coef"]]
        pb, cb, fb = dev.buf(rows["ptr"]), dev.buf(rows["col"]), dev.buf(rows["coef"])
        tb_h, hb, pbuf = dev.buf((mm, ld_h), np.float32), dev.buf((mm, ld_h), np.float32), dev.buf((mm, ld_c), np.float32)
        pred, prob = dev.buf((mm,), np.int32), dev.buf((mm,), np.float32)
        xf = [None]

        def feat_object():
            if xf[0] is not None:
                xf[0].free()
            xf[0] = dev.feat(np.arange(mm + 1, dtype=np.int64) * F, None, x.ravel(), F)
        r = dict(new_nodes=mm, stored_entries=nnz, host_plan_wall_ms=plan_ms, feature_object_wall_ms=wall(feat_object, reps=3))
        r["new_first_layer_product_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_spmm_fwd(dev.ctx, xf[0].h, xf[0].values_ptr, w1b.ptr, ld_h, tb_h.ptr, ld_h, hidden, 0.0, 0,
                                                                                           None, 0, None), "spmm_fwd"), 10)
        r["hidden_gather_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_attach_gather(dev.ctx, pb.ptr, cb.ptr, fb.ptr, mm, ta_h.ptr, ld_h, N, tb_h.ptr, ld_h, hidden, 1,
                                                                                      hb.ptr, ld_h, None, None, None, 0, 1.0), "attach_gather"), 10)
        r["small_product_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_matmul_fwd(dev.ctx, hb.ptr, ld_h, w2b.ptr, ld_c, pbuf.ptr, ld_c, mm, hidden, nc), "matmul_fwd"), 10)
        r["class_gather_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_attach_gather(dev.ctx, pb.ptr, cb.ptr, fb.ptr, mm, ta_c.ptr, ld_c, N, pbuf.ptr, ld_c, nc, 2, None, 0,
                                                                                     pred.ptr, prob.ptr, None, 0, 1.0), "attach_gather"), 10)

        def copies():
            for b, a in zip((pb, cb, fb), host_in):
                b.upload(a)
            pred.download()
            prob.download()
        r["copies_wall_ms"] = wall(copies, reps=3)
        for key, dim in (("hidden", hidden), ("class", nc)):
            nbytes = float(nnz) * (dim * 4 + 8)
            r[f"{key}_gather_bytes"] = nbytes
            r[f"{key}_gather_TBps"] = nbytes / (r[f"{key}_gather_ms"] * 1e-3) / 1e12
            r[f"{key}_gather_ms_at_aggregation_rate"] = 1e3 * nbytes / (res["hidden_aggregation_TBps"] * 1e12)
        res["parts_" + label] = r
        xf[0].free()
        for b in (pb, cb, fb, tb_h, hb, pbuf, pred, prob):
            b.free()
    dev.close()
    if parent:
        res["epochs_per_s"] = epoch_path(parent, rounds)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
