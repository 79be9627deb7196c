"""Multi-label decision thresholds on reddit-syn (hidden 128, C = 121 multi-label), HIP events and wall time — the figures of
DESIGN §4.16:
  * the scan launch apart, gcnhip_threshold_scan next to gcnhip_rank_stats on the same sorted tables (the validation split and
    every row, keys of standard-normal scores): both walk a class's positives and search
    its negatives' column.  Three rounds, the two alternating, so that the spread between rounds stands next to the gap;
  * HipGCNModel.tune_thresholds(split=2) next to ranking(split=2) and evaluate(split=2): wall time with their synchronisation;
  * micro- and macro-F1 of the test split by the training rule z > 0 and by the cuts fitted on the validation split.
Prints one JSON line.  None of the values is a pass/fail threshold.  usage: bench_thresholds.py [dataset] [epochs]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_gcn_amd import datagen, ops
from cuda_gcn_amd.model import HipGCNModel
from cuda_gcn_amd.ops import Device, _ck
from tools.bench_calibration import timeit, wall

ROUNDS = 3


def launches(dev, N, c, rows, bits):
    """the stats and the scan launch over the sorted tables of `rows` (None: every row) of an [N x c] table; milliseconds"""
    lib = dev.lib
    rng = np.random.default_rng(0)
    table = dev.buf(rng.standard_normal((N, c)).astype(np.float32))
    n = N if rows is None else rows.size
    rb = dev.buf(rows) if rows is not None else None
    words = ops.pack_multihot(bits)
    wb = dev.buf(words)
    keys, scratch = dev.buf((2 * c, n), np.uint32), dev.buf((2 * c, n), np.uint32)
    counts = dev.buf((3 * c + 1,), np.int32)
    work = dev.buf((2 * c * ops.RANK_STATS_BLOCKS,), np.float64)
    u2, ap = dev.buf((c,), np.int64), dev.buf((c,), np.float64)
    thr, cnt, f, defined = dev.buf((c,), np.float32), dev.buf((3 * c,), np.int32), dev.buf((c,), np.float64), dev.buf((c,), np.int32)
    neg_keys = keys.ptr + 4 * c * n
    cp, cn, ci, cu = (counts.ptr + 4 * k * c for k in range(4))
    _ck(lib, lib.gcnhip_rank_keys(dev.ctx, table.ptr, c, N, rb.ptr if rb else None, n, 0, c, c, None, wb.ptr, words.shape[1], keys.ptr, neg_keys, n,
                                  cp, cn, ci, cu), "keys")
    _ck(lib, lib.gcnhip_sort_segments_u32(dev.ctx, keys.ptr, scratch.ptr, n, 2 * c, n), "sort")

    def do_stats():
        _ck(lib, lib.gcnhip_rank_stats(dev.ctx, keys.ptr, neg_keys, n, n, c, cp, cn, work.ptr, u2.ptr, ap.ptr), "stats")

    def do_scan():
        _ck(lib, lib.gcnhip_threshold_scan(dev.ctx, keys.ptr, neg_keys, n, n, c, cp, cn, 1.0, work.ptr, thr.ptr, cnt.ptr, f.ptr, defined.ptr), "scan")

    res = dict(rows=n, classes=c, positives=int(counts.download()[:c].sum()), stats_ms=[], scan_ms=[])
    for _ in range(ROUNDS):
        res["stats_ms"].append(timeit(dev, do_stats, iters=200))
        res["scan_ms"].append(timeit(dev, do_scan, iters=200))
    for b in (table, rb, wb, keys, scratch, counts, work, u2, ap, thr, cnt, f, defined):
        if b is not None:
            b.free()
    return res


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    name = argv[0] if argv else "reddit-syn"
    epochs = int(argv[1]) if len(argv) > 1 else 10
    ds = datagen.make_dataset(name)
    N = ds["num_nodes"]
    y = datagen.multilabel_from_communities(ds["label"], classes=121)
    val = np.flatnonzero(ds["split"] == 2).astype(np.int32)
    res = dict(dataset=name, nodes=N, val_rows=int(val.size), classes=121)
    dev = Device(0)
    for where, rows in (("val", val), ("all", None)):
        res[f"launches_{where}"] = launches(dev, N, 121, rows, y)
    dev.close()
    print("launches:", json.dumps(res), file=sys.stderr, flush=True)         # kept should the model below fail
    m = HipGCNModel(ds, seed=1, hidden_dim=128, dropout=0.5, multilabel=y)
    m.run_epochs(epochs, want_trace=False)
    r = dict(epochs=epochs, tune_val_wall_ms=[], ranking_val_wall_ms=[], evaluate_val_wall_ms=[])
    for _ in range(ROUNDS):
        r["tune_val_wall_ms"].append(wall(lambda: m.tune_thresholds(split=2), reps=20))
        r["ranking_val_wall_ms"].append(wall(lambda: m.ranking(split=2), reps=20))
        r["evaluate_val_wall_ms"].append(wall(lambda: m.evaluate(split=2), reps=20))
    fit = m.tune_thresholds(split=2)
    base_val, base_test, tuned_test = m.evaluate(split=2), m.evaluate(split=3), m.evaluate(split=3, thresholds=fit)
    r.update(classes_defined=int(fit["defined"].sum()), val_macro_f1_default=base_val["macro_f1"], val_macro_f1_tuned=fit["macro_f1"],
             test_micro_f1_default=base_test["micro_f1"], test_micro_f1_tuned=tuned_test["micro_f1"],
             test_macro_f1_default=base_test["macro_f1"], test_macro_f1_tuned=tuned_test["macro_f1"])
    m.close()
    res["model"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
