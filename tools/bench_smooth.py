"""Label propagation / Correct & Smooth on reddit-syn (hidden 128, 41 classes), HIP events — the figures of DESIGN §4.8:
  * one blend launch (gcnhip_graphsum_blend) and one prediction launch (gcnhip_graphsum_predict, no logits stored) against
    one all-row class-width gcnhip_graphsum_ex launch (per-edge coefficients) on the same table: the blend reads one more
    row per output row;
  * HipGCNModel.correct_and_smooth at the default iteration counts against predict(), wall time with a synchronisation;
  * test-split accuracy before and after.
Prints one JSON line.  None of the values is a pass/fail threshold.  usage: bench_smooth.py [dataset] [epochs]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_gcn_amd import datagen
from cuda_gcn_amd.model import HipGCNModel
from cuda_gcn_amd.ops import Device, GsOpts, _ck


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
    ld = (c + 3) // 4 * 4 if c <= 32 else (c + 15) // 16 * 16
    res = dict(dataset=name, nodes=N, edges=int(ds["g_indices"].size), classes=c, ld=ld)
    # ---- one launch
    dev = Device(0)
    lib = dev.lib
    g = dev.graph(ds["g_indptr"], ds["g_indices"], row_group=ds["label"])             # as HipGCN builds it
    rng = np.random.default_rng(0)
    x, base, out = dev.buf(rng.random((N, ld), dtype=np.float32)), dev.buf(rng.random((N, ld), dtype=np.float32)), dev.buf((N, ld))
    pred, prob = dev.buf((N,), np.int32), dev.buf((N,), np.float32)
    o = GsOpts()
    res["graphsum_ex_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_graphsum_ex(dev.ctx, g.h, C.byref(o), x.ptr, ld, out.ptr, ld, c), "graphsum_ex"))
    res["blend_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_graphsum_blend(dev.ctx, g.h, x.ptr, ld, base.ptr, ld, out.ptr, ld, c, 0.8, 0.2, 0.0, 1.0, None), "blend"))
    res["blend_own_base_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_graphsum_blend(dev.ctx, g.h, x.ptr, ld, x.ptr, ld, out.ptr, ld, c, 0.8, 0.2, 0.0, 1.0, None), "blend"))
    res["blend_pred_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_graphsum_blend(dev.ctx, g.h, x.ptr, ld, base.ptr, ld, out.ptr, ld, c, 0.8, 0.2, 0.0, 1.0, pred.ptr), "blend"))
    res["predict_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_graphsum_predict(dev.ctx, g.h, None, x.ptr, None, ld, None, ld, c, 0, pred.ptr, prob.ptr, None, 0), "predict"))
    res["graphsum_ex_ms_again"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_graphsum_ex(dev.ctx, g.h, C.byref(o), x.ptr, ld, out.ptr, ld, c), "graphsum_ex"))
    for b in (x, base, out, pred, prob):
        b.free()
    g.free()
    dev.close()
    # ---- the model
    m = HipGCNModel(ds, seed=1, hidden_dim=128, dropout=0.5)
    m.run_epochs(epochs, want_trace=False)
    test = ds["split"] == 3
    label = ds["label"][test]
    p0, _ = m.predict()
    p1, _ = m.correct_and_smooth(scores=False)
    p2, _ = m.label_propagation()
    res.update(epochs=epochs, test_rows=int(test.sum()), acc_predict=float(np.mean(p0[test] == label)),
               acc_correct_and_smooth=float(np.mean(p1[test] == label)), acc_label_propagation=float(np.mean(p2[test] == label)))
    res["predict_wall_ms"] = wall(lambda: m.predict())
    res["correct_and_smooth_wall_ms"] = wall(lambda: m.correct_and_smooth(scores=False))
    res["correct_and_smooth_with_scores_wall_ms"] = wall(lambda: m.correct_and_smooth())
    res["label_propagation_wall_ms"] = wall(lambda: m.label_propagation())
    m.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
