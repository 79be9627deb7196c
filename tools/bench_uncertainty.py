"""Monte Carlo dropout on reddit-syn (hidden 128, 41 classes) — the figures of DESIGN §4.18:
  * HipGCNModel.mc_dropout(samples=20) over every row and over the test split, wall time with a synchronisation, against one
    predict() and against 20 training forwards' worth of the model's own device timers (the first-layer product, the two
    aggregations and the class-layer product of a training pass: what a stochastic forward launches);
  * one gcnhip_mc_accumulate_rows and one gcnhip_mc_finalize_rows launch over every row (HIP events) against their byte floors;
  * the accuracy of the mean-softmax class against predict()'s on the test split, and the mean mutual information of the
    wrongly and of the rightly classified test rows.
Prints one JSON line and, with --out, writes it.  None of the values is a pass/fail threshold.
usage: bench_uncertainty.py [--dataset reddit-syn] [--epochs 30] [--samples 20] [--out profiles/<file>.json]"""
import argparse
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


def timeit(dev, fn, iters=50, warmup=5):
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="reddit-syn")
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    ds = datagen.make_dataset(a.dataset)
    N, c, S = ds["num_nodes"], ds["output_dim"], a.samples
    test = np.flatnonzero(ds["split"] == 3)
    res = dict(dataset=a.dataset, nodes=N, classes=c, hidden=128, samples=S, test_rows=int(test.size), epochs=a.epochs)
    # ---- one launch each over every row of an [N x C] table
    dev = Device(0)
    lib = dev.lib
    z = np.random.default_rng(0).standard_normal((N, c)).astype(np.float32) * 2
    z -= z.max(axis=1, keepdims=True)
    logp = dev.buf(z - np.log(np.exp(z).sum(axis=1, keepdims=True)))
    acc, votes = dev.buf((N, c + 1), np.float64), dev.buf((N, c), np.int32)
    outs = [dev.buf((N,), np.float32) for _ in range(5)]
    pred, mp = dev.buf((N,), np.int32), dev.buf((N, c), np.float32)
    _ck(lib, lib.gcnhip_mc_accumulate_rows(dev.ctx, logp.ptr, c, N, None, N, c, 1, acc.ptr, votes.ptr), "accumulate")
    res["accumulate_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_mc_accumulate_rows(dev.ctx, logp.ptr, c, N, None, N, c, 0, acc.ptr, votes.ptr), "accumulate"))
    res["accumulate_first_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_mc_accumulate_rows(dev.ctx, logp.ptr, c, N, None, N, c, 1, acc.ptr, votes.ptr), "accumulate"))
    res["finalize_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_mc_finalize_rows(dev.ctx, acc.ptr, votes.ptr, N, c, S, mp.ptr, c, pred.ptr, *[o.ptr for o in outs]),
                                                 "finalize"))
    res["finalize_no_mean_prob_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_mc_finalize_rows(dev.ctx, acc.ptr, votes.ptr, N, c, S, None, c, pred.ptr,
                                                                                               *[o.ptr for o in outs]), "finalize"))
    # byte floors: the row read, both accumulators read and written; the accumulators read, 6 scalars (and the mean row) written
    res["accumulate_bytes"] = N * (4 * c + 2 * 8 * (c + 1) + 2 * 4 * c)
    res["accumulate_first_bytes"] = N * (4 * c + 8 * (c + 1) + 4 * c)
    res["finalize_bytes"] = N * (8 * (c + 1) + 4 * c + 6 * 4 + 4 * c)
    res["finalize_no_mean_prob_bytes"] = N * (8 * (c + 1) + 4 * c + 6 * 4)
    for k in ("accumulate", "accumulate_first", "finalize", "finalize_no_mean_prob"):
        res[k + "_gb_s"] = res[k + "_bytes"] / (res[k + "_ms"] * 1e-3) / 1e9
    for b in [logp, acc, votes, pred, mp] + outs:
        b.free()
    dev.close()
    # ---- the model
    m = HipGCNModel(ds, seed=1, hidden_dim=128, dropout=0.5)
    m.run_epochs(a.epochs, want_trace=False)
    m.set_timers(True)
    m.timers_reset()
    for _ in range(S):
        m.train_epoch()
    fw = {k: m.timer(k)[0] * 1e3 for k in ("spmatmul_fw", "graphsum_fw", "matmul_fw", "loss_fw")}
    m.set_timers(False)
    res["train_forward_timers_ms"] = fw                         # S training passes: the forward launches by module
    res["train_forwards_ms"] = fw["spmatmul_fw"] + fw["graphsum_fw"] + fw["matmul_fw"]
    res["predict_wall_ms"] = wall(lambda: m.predict())
    res["mc_all_rows_wall_ms"] = wall(lambda: m.mc_dropout(samples=S), reps=3)
    res["mc_test_split_wall_ms"] = wall(lambda: m.mc_dropout(samples=S, split=3), reps=3)
    pred, _ = m.predict()
    out = m.mc_dropout(samples=S, nodes=test.astype(np.int32))
    label = ds["label"][test]
    right = out["pred"] == label
    mi = out["mutual_information"].astype(np.float64)
    res.update(test_acc_predict=float(np.mean(pred[test] == label)), test_acc_mc=float(np.mean(right)),
               mc_pred_equals_predict=float(np.mean(out["pred"] == pred[test])),
               mean_mi_wrong=float(mi[~right].mean()) if (~right).any() else None, mean_mi_right=float(mi[right].mean()) if right.any() else None,
               mean_entropy=float(out["entropy"].astype(np.float64).mean()), mean_variation_ratio=float(out["variation_ratio"].astype(np.float64).mean()),
               seed=out["seed"], p=out["p"])
    m.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
