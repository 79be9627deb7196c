"""Time HipGCNModel.evaluate() on reddit-syn (hidden 128, 41 classes) against the two routes that exist without it — one
evaluation forward (eval(2)), and predict() on every node followed by the numpy confusion matrix on the host — and the two
count kernels alone against the bytes they read.  Model figures: the mean over --iters synchronised calls after --warmup
calls, timed with HIP events (torch.cuda.Event, recorded before and after the calls; every call synchronises its own
stream) and with the host clock, the protocol of tools/bench_predict.py.  Kernel figures: HIP events of the library's own
context around --kernel-iters back-to-back launches (each launch zeroes its output first: two memsets are inside the figure).
The script ends itself after --limit seconds.

    python tools/bench_report.py [--dataset reddit-syn] [--iters 20] [--warmup 3] [--limit 600]
"""
import argparse
import ctypes as C
import json
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernel_times(n, classes, ml_classes, iters):
    """microseconds per launch of the two count kernels on n rows, and the bytes each reads"""
    from cuda_gcn_amd.ops import Device, pack_multihot
    dev = Device(0)
    lib = dev.lib
    rng = np.random.default_rng(0)
    e0, e1 = C.c_void_p(), C.c_void_p()
    lib.gcnhip_event_create(C.byref(e0))
    lib.gcnhip_event_create(C.byref(e1))

    def timed(launch):
        for _ in range(3):
            assert launch() == 0
        dev.sync()
        lib.gcnhip_event_record(dev.ctx, e0)
        for _ in range(iters):
            launch()
        lib.gcnhip_event_record(dev.ctx, e1)
        dev.sync()
        ms = C.c_float()
        lib.gcnhip_event_elapsed_ms(e0, e1, C.byref(ms))
        return 1e3 * ms.value / iters
    out = {}
    truth = rng.integers(0, classes, n).astype(np.int32)
    uniform = rng.integers(0, classes, n).astype(np.int32)
    trained = np.where(rng.random(n) < 0.95, truth, uniform).astype(np.int32)          # 95 % on the diagonal, as a trained model
    hot_t, hot_p = truth.copy(), uniform.copy()
    hot = rng.random(n) < 0.9
    hot_t[hot], hot_p[hot] = 2, 2                                                      # 90 % of the rows in ONE cell
    rows = np.sort(rng.permutation(n)[: n // 10]).astype(np.int32)                     # a validation split's list
    cb, ob = dev.buf(np.zeros(classes * classes, np.int32)), dev.buf(np.zeros(1, np.int32))
    rb = dev.buf(rows)
    for tag, t, p in (("uniform", truth, uniform), ("trained", truth, trained), ("one_cell_90", hot_t, hot_p)):
        tb, pb = dev.buf(t), dev.buf(p)
        out[f"confusion_{tag}_us"] = round(timed(lambda: lib.gcnhip_confusion_rows(dev.ctx, pb.ptr, tb.ptr, n, None, n, classes, cb.ptr, ob.ptr)), 2)
        if tag == "trained":
            out["confusion_trained_rowlist_10pct_us"] = round(timed(lambda: lib.gcnhip_confusion_rows(dev.ctx, pb.ptr, tb.ptr, n, rb.ptr, rows.size, classes, cb.ptr, ob.ptr)), 2)
    out["confusion_bytes_read"] = 8 * n
    ld = (ml_classes + 3) // 4 * 4
    z = rng.standard_normal((n, ld)).astype(np.float32)
    words = pack_multihot(rng.random((n, ml_classes)) < 0.05)
    zb, wb, kb = dev.buf(z), dev.buf(words), dev.buf(np.zeros(3 * ml_classes, np.int32))
    out["class_counts_us"] = round(timed(lambda: lib.gcnhip_bce_class_counts_rows(dev.ctx, zb.ptr, ld, wb.ptr, words.shape[1], None, n, ml_classes, kb.ptr)), 2)
    out["class_counts_classes"] = ml_classes
    out["class_counts_bytes_read"] = int(n * (4 * ml_classes + 4 * words.shape[1]))
    for k, b in (("confusion_uniform", 8 * n), ("confusion_trained", 8 * n), ("class_counts", out["class_counts_bytes_read"])):
        out[k + "_GBps"] = round(b / out[k + "_us"] / 1e3, 1)
    lib.gcnhip_event_destroy(e0)
    lib.gcnhip_event_destroy(e1)
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="reddit-syn")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--limit", type=int, default=600)
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: sys.exit("bench_report: time limit reached"))
    signal.alarm(a.limit)
    import torch
    from cuda_gcn_amd import datagen
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.make_dataset(a.dataset)
    m = HipGCNModel(ds, seed=1, hidden_dim=128, dropout=0.5)
    for _ in range(3):
        m.train_epoch()
    label, cls = ds["label"].astype(np.int64), ds["output_dim"]

    def predict_numpy():
        pred, _ = m.predict()
        ok = (label >= 0) & (ds["split"] == 2)
        return np.bincount(label[ok] * cls + pred[ok], minlength=cls * cls).reshape(cls, cls)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return round(e0.elapsed_time(e1) / a.iters, 4), round(1e3 * (time.perf_counter() - t0) / a.iters, 4)
    assert np.array_equal(predict_numpy(), m.evaluate(2)["confusion"])
    res = {}
    for tag, fn in (("eval2", lambda: m.eval(2)), ("predict_all_plus_numpy", predict_numpy), ("evaluate_2", lambda: m.evaluate(2)),
                    ("evaluate_1", lambda: m.evaluate(1)), ("evaluate_all", lambda: m.evaluate())):
        res[tag + "_ms"], res[tag + "_host_ms"] = timed(fn)
    m.close()
    out = dict(dataset=a.dataset, nodes=int(ds["num_nodes"]), iters=a.iters, **res,
               evaluate_2_share_of_eval=round(res["evaluate_2_ms"] / res["eval2_ms"], 3),
               evaluate_2_share_of_predict_numpy=round(res["evaluate_2_ms"] / res["predict_all_plus_numpy_ms"], 3),
               kernels=kernel_times(int(ds["num_nodes"]), cls, 121, a.kernel_iters))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
