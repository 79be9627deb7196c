#!/usr/bin/env python3
"""Class-weighted training at the Reddit shape.  Kernels, HIP events, in one process: gcnhip_wxent_fwd_rows against
gcnhip_xent_fwd_rows_scaled on reddit-syn's training rows (153 756 x 41) and gcnhip_wbce_fwd_rows against gcnhip_bce_fwd_rows
at C = 121, each pair on the same inputs, alternating, several repeats (the spread of the unweighted kernel's repeats is the
yardstick for the ratio).  Model: epochs/s (run_epochs) of reddit-syn-zipf with "balanced" weights, unweighted with
HIPGCN_NO_LOSS_EPILOGUE=1 (the same shape: a loss kernel on the stored logits), and unweighted by default (loss epilogue).
Prints one JSON line.

    python tools/bench_class_weights.py [--epochs 50] [--warmup 10] [--no-model]
"""
import argparse
import ctypes as ct
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_gcn_amd import datagen  # noqa: E402
from cuda_gcn_amd.model import HipGCNModel  # noqa: E402


def epochs_per_s(m, epochs, warmup):
    m.run_epochs(warmup, want_trace=False)
    t0 = time.perf_counter()
    tr = m.run_epochs(epochs)
    return epochs / (time.perf_counter() - t0), tr[-1].tolist()


def kernel_pairs(n_rows, reps=50, repeats=5):
    from cuda_gcn_amd.ops import Device, pack_multihot
    dev = Device(0)
    lib = dev.lib
    rng = np.random.default_rng(0)
    N = int(n_rows * 1.52)                               # the logit table holds every node; the split's rows are listed
    rows = np.sort(rng.choice(N, n_rows, replace=False)).astype(np.int32)
    rb = dev.buf(rows)
    res, resi = dev.buf(np.zeros(4, np.float32)), dev.buf(np.zeros(4, np.int32))
    e0, e1 = ct.c_void_p(), ct.c_void_p()
    lib.gcnhip_event_create(ct.byref(e0))
    lib.gcnhip_event_create(ct.byref(e1))

    def timed(launch):
        for _ in range(5):
            launch()
        dev.sync()
        lib.gcnhip_event_record(dev.ctx, e0)
        for _ in range(reps):
            launch()
        lib.gcnhip_event_record(dev.ctx, e1)
        lib.gcnhip_event_sync(e1)
        ms = ct.c_float()
        lib.gcnhip_event_elapsed_ms(e0, e1, ct.byref(ms))
        return 1e3 * ms.value / reps

    out = {}
    # single-label, C = 41
    C, ld = 41, 44
    z, g = dev.buf(rng.standard_normal((N, ld)).astype(np.float32)), dev.buf((N, ld), np.float32)
    tb = dev.buf(rng.integers(0, C, N).astype(np.int32))
    w = rng.uniform(0.1, 10, C).astype(np.float32)
    wb = dev.buf(w)

    def xent():
        assert lib.gcnhip_xent_fwd_rows_scaled(dev.ctx, z.ptr, ld, g.ptr, ld, tb.ptr, rb.ptr, n_rows, C, 1, n_rows, 0, res.ptr, resi.ptr, None) == 0

    def wxent():
        assert lib.gcnhip_wxent_fwd_rows(dev.ctx, z.ptr, ld, g.ptr, ld, tb.ptr, rb.ptr, n_rows, C, 1, n_rows, 0, res.ptr, resi.ptr, None, wb.ptr,
                                         float(n_rows)) == 0
    a, b = [], []
    for _ in range(repeats):
        a.append(timed(xent))
        b.append(timed(wxent))
    out["xent_c41_us"], out["wxent_c41_us"] = a, b
    out["wxent_over_xent"] = float(np.median(b) / np.median(a))
    # multi-label, C = 121
    C, ld = 121, 124
    z, g = dev.buf(rng.standard_normal((N, ld)).astype(np.float32)), dev.buf((N, ld), np.float32)
    words = pack_multihot(rng.random((N, C)) < 0.05)
    tw = dev.buf(words)
    pb = dev.buf(rng.uniform(0.1, 10, C).astype(np.float32))

    def bce():
        assert lib.gcnhip_bce_fwd_rows(dev.ctx, z.ptr, ld, g.ptr, ld, tw.ptr, words.shape[1], rb.ptr, n_rows, C, 1, n_rows, None, res.ptr, resi.ptr) == 0

    def wbce():
        assert lib.gcnhip_wbce_fwd_rows(dev.ctx, z.ptr, ld, g.ptr, ld, tw.ptr, words.shape[1], rb.ptr, n_rows, C, 1, n_rows, None, res.ptr, resi.ptr,
                                        pb.ptr) == 0
    a, b = [], []
    for _ in range(repeats):
        a.append(timed(bce))
        b.append(timed(wbce))
    out["bce_c121_us"], out["wbce_c121_us"] = a, b
    out["wbce_over_bce"] = float(np.median(b) / np.median(a))
    lib.gcnhip_event_destroy(e0)
    lib.gcnhip_event_destroy(e1)
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    out = dict(train_rows=153756)
    out.update(kernel_pairs(out["train_rows"]))
    if not a.no_model:
        ds = datagen.make_dataset("reddit-syn-zipf")
        out["nodes"] = ds["num_nodes"]
        kw = dict(seed=1, hidden_dim=128, dropout=0.5)
        for name, env, cw in (("default_unweighted", None, None), ("unweighted_no_loss_epilogue", "1", None), ("balanced", None, "balanced"),
                              ("default_unweighted_again", None, None)):
            if env:
                os.environ["HIPGCN_NO_LOSS_EPILOGUE"] = env
            else:
                os.environ.pop("HIPGCN_NO_LOSS_EPILOGUE", None)
            m = HipGCNModel(ds, class_weights=cw, **kw)
            out[name + "_epochs_per_s"], out[name + "_last"] = epochs_per_s(m, a.epochs, a.warmup)
            m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
