#!/usr/bin/env python3
"""Multi-label training at the Reddit shape (reddit-syn: 232 965 nodes, 602 features, hidden 128): epochs/s (train_epoch +
eval(2), run_epochs) with C = 121 multi-label classes (datagen.multilabel_from_communities of the dataset's communities)
against the C = 41 single-label model on the same graph, and gcnhip_bce_fwd_rows alone on the training split's logits
(read Z rows, write dZ rows, truth words) against its bytes.  Prints one JSON line.

    python tools/bench_multilabel.py [--epochs 50] [--warmup 10]
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


def kernel_time(n_rows, C, reps=50):
    from cuda_gcn_amd.ops import Device, pack_multihot
    dev = Device(0)
    lib = dev.lib
    rng = np.random.default_rng(0)
    N = int(n_rows * 1.52)                               # the logit table holds every node; the split's rows are listed
    ld = (C + 3) // 4 * 4
    z = dev.buf(rng.standard_normal((N, ld)).astype(np.float32))
    g = dev.buf((N, ld), np.float32)
    words = pack_multihot(rng.random((N, C)) < 0.05)
    tb = dev.buf(words)
    rows = np.sort(rng.choice(N, n_rows, replace=False)).astype(np.int32)
    rb = dev.buf(rows)
    res, resi = dev.buf(np.zeros(4, np.float32)), dev.buf(np.zeros(4, np.int32))

    def launch():
        rc = lib.gcnhip_bce_fwd_rows(dev.ctx, z.ptr, ld, g.ptr, ld, tb.ptr, words.shape[1], rb.ptr, n_rows, C, 1, n_rows, None, res.ptr, resi.ptr)
        assert rc == 0, rc
    for _ in range(5):
        launch()
    dev.sync()
    e0, e1 = ct.c_void_p(), ct.c_void_p()
    lib.gcnhip_event_create(ct.byref(e0))
    lib.gcnhip_event_create(ct.byref(e1))
    lib.gcnhip_event_record(dev.ctx, e0)
    for _ in range(reps):
        launch()
    lib.gcnhip_event_record(dev.ctx, e1)
    lib.gcnhip_event_sync(e1)
    ms = ct.c_float()
    lib.gcnhip_event_elapsed_ms(e0, e1, ct.byref(ms))
    t = ms.value / reps
    nbytes = n_rows * (2 * C * 4 + words.shape[1] * 4 + 4)   # logits read, dZ written, truth words, row ids
    lib.gcnhip_event_destroy(e0)
    lib.gcnhip_event_destroy(e1)
    dev.close()
    return dict(ms=t, bytes=nbytes, gb_s=nbytes / t / 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    ds = datagen.make_dataset("reddit-syn")
    y = datagen.multilabel_from_communities(ds["label"], classes=121)
    out = dict(nodes=ds["num_nodes"], train_rows=int(np.sum(ds["split"] == 1)))
    m = HipGCNModel(ds, seed=1, hidden_dim=128, dropout=0.5)
    out["single_label_c41_epochs_per_s"], out["single_label_last"] = epochs_per_s(m, a.epochs, a.warmup)
    m.close()
    m = HipGCNModel(ds, seed=1, hidden_dim=128, dropout=0.5, multilabel=y)
    out["multilabel_c121_epochs_per_s"], out["multilabel_last"] = epochs_per_s(m, a.epochs, a.warmup)
    m.close()
    out["bce_kernel_c121"] = kernel_time(out["train_rows"], 121)
    out["bce_kernel_c41"] = kernel_time(out["train_rows"], 41)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
