"""Temperature scaling / calibration error on reddit-syn (hidden 128, 41 classes), HIP events — the figures of DESIGN §4.9:
  * one gcnhip_calib_nll_rows and one gcnhip_calib_bins_rows launch (with their finalize launch) over the validation split's
    rows, beside the bytes they read;
  * HipGCNModel.calibrate() as a whole against one predict(), wall time with a synchronisation;
  * ECE and NLL of the test split before and after.
Prints one JSON line.  None of the values is a pass/fail threshold.  usage: bench_calibration.py [dataset] [epochs]"""
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
    name = sys.argv[1] if len(sys.argv) > 1 else "reddit-syn"
    epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    ds = datagen.make_dataset(name)
    N, c = ds["num_nodes"], ds["output_dim"]
    val = np.flatnonzero(ds["split"] == 2).astype(np.int32)
    res = dict(dataset=name, nodes=N, classes=c, val_rows=int(val.size))
    # ---- one launch each over the validation rows of an [N x C] table
    dev = Device(0)
    lib = dev.lib
    rng = np.random.default_rng(0)
    z = rng.standard_normal((N, c)).astype(np.float32) * 2
    z -= z.max(axis=1, keepdims=True)
    logp = dev.buf(z - np.log(np.exp(z).sum(axis=1, keepdims=True)))
    truth, rows = dev.buf(ds["label"].astype(np.int32)), dev.buf(val)
    sums, conf = dev.buf((4,), np.float64), dev.buf((15,), np.float64)
    cnt, cor = dev.buf((15,), np.int32), dev.buf((15,), np.int32)
    res["nll_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_calib_nll_rows(dev.ctx, logp.ptr, c, truth.ptr, N, rows.ptr, val.size, c, 1.0, sums.ptr), "nll"))
    res["bins_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_calib_bins_rows(dev.ctx, logp.ptr, c, truth.ptr, N, rows.ptr, val.size, c, 1.0, 15,
                                                                            cnt.ptr, cor.ptr, conf.ptr), "bins"))
    res["bytes_read"] = int(val.size) * (4 * c + 8)              # the row, its id and its truth
    for k in ("nll", "bins"):
        res[k + "_gb_s"] = res["bytes_read"] / (res[k + "_ms"] * 1e-3) / 1e9
    for b in (logp, truth, rows, sums, conf, cnt, cor):
        b.free()
    dev.close()
    # ---- the model
    m = HipGCNModel(ds, seed=1, hidden_dim=128, dropout=0.5)
    m.run_epochs(epochs, want_trace=False)
    before = m.calibration(split=3)
    res["predict_wall_ms"] = wall(lambda: m.predict())
    res["calibrate_wall_ms"] = wall(lambda: m.calibrate(apply=False))
    fit = m.calibrate()
    after = m.calibration(split=3)
    res.update(epochs=epochs, temperature=fit["temperature"], steps=fit["steps"], val_nll_before=fit["nll_before"], val_nll_after=fit["nll_after"],
               test_rows=before["rows"], test_nll_before=before["nll"], test_nll_after=after["nll"], test_ece_before=before["ece"],
               test_ece_after=after["ece"])
    res["predict_calibrated_wall_ms"] = wall(lambda: m.predict())
    m.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
