"""Split conformal prediction sets on reddit-syn (hidden 128, 41 classes), HIP events — the figures of DESIGN §4.14:
  * one gcnhip_conformal_scores launch (lac and aps) and one gcnhip_conformal_sets_rows launch (bits, sizes and counts) over
    ALL rows of an [N x C] table, beside the bytes they move;
  * HipGCNModel.conformal_fit() and coverage() as a whole against predict() of all nodes in the same run, wall time with a
    synchronisation, without and with diffusion;
  * coverage and mean set size of the test split for lac, aps and aps with diffusion.
Prints one JSON line.  None of the values is a pass/fail threshold.  usage: bench_conformal.py [dataset] [epochs] [alpha]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_gcn_amd import datagen
from cuda_gcn_amd.model import HipGCNModel
from cuda_gcn_amd.ops import Device, _ck
from tools.bench_calibration import timeit, wall


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "reddit-syn"
    epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    alpha = float(sys.argv[3]) if len(sys.argv) > 3 else 0.1
    ds = datagen.make_dataset(name)
    N, c = ds["num_nodes"], ds["output_dim"]
    res = dict(dataset=name, nodes=N, classes=c, alpha=alpha)
    # ---- one launch each over every row of an [N x C] table
    dev = Device(0)
    lib = dev.lib
    rng = np.random.default_rng(0)
    z = rng.standard_normal((N, c)).astype(np.float32) * 2
    z -= z.max(axis=1, keepdims=True)
    ld = (c + 15) // 16 * 16 if c > 32 else (c + 3) // 4 * 4
    wpr = (c + 31) // 32
    logp = dev.buf(z - np.log(np.exp(z).sum(axis=1, keepdims=True)))
    table = dev.buf(np.zeros((N, ld), np.float32))
    truth = dev.buf(ds["label"].astype(np.int32))
    thresh = dev.buf(np.full(c, 0.9, np.float32))
    bits, size, counts = dev.buf((N, wpr), np.uint32), dev.buf((N,), np.int32), dev.buf((4 + 3 * c + 1,), np.int32)
    for key, method in (("scores_lac", 0), ("scores_aps", 1)):
        res[key + "_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_conformal_scores(dev.ctx, logp.ptr, c, N, None, N, c, 1.0, method, 0.0, 0, table.ptr, ld),
                                                   key))
    res["scores_bytes"] = N * 8 * c                               # a row read, a row written
    res["sets_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_conformal_sets_rows(dev.ctx, table.ptr, ld, N, None, N, c, thresh.ptr, truth.ptr, bits.ptr,
                                                                                 size.ptr, counts.ptr), "sets"))
    res["sets_counts_only_ms"] = timeit(dev, lambda: _ck(lib, lib.gcnhip_conformal_sets_rows(dev.ctx, table.ptr, ld, N, None, N, c, thresh.ptr, truth.ptr,
                                                                                             None, None, counts.ptr), "sets"))
    res["sets_bytes"] = N * (4 * c + 4 + 4 * wpr + 4)             # the row and its truth read, its bits and size written
    for k, b in (("scores_lac", "scores_bytes"), ("scores_aps", "scores_bytes"), ("sets", "sets_bytes")):
        res[k + "_gb_s"] = res[b] / (res[k + "_ms"] * 1e-3) / 1e9
    for b in (logp, table, truth, thresh, bits, size, counts):
        b.free()
    dev.close()
    # ---- the model
    m = HipGCNModel(ds, seed=1, hidden_dim=128, dropout=0.5)
    m.run_epochs(epochs, want_trace=False)
    res["epochs"] = epochs
    res["predict_wall_ms"] = wall(lambda: m.predict())
    for key, kw in (("lac", dict(method="lac")), ("aps", dict(method="aps")), ("aps_diffusion", dict(method="aps", diffusion=0.5))):
        fit = m.conformal_fit(alpha=alpha, **kw)
        cov = m.coverage(fit, split=3)
        res[key] = dict(threshold=fit["threshold"], cal_rows=int(fit["n_cal"][0]), test_rows=cov["rows"], test_coverage=cov["coverage"],
                        test_mean_set_size=cov["mean_size"], test_empty=cov["empty"],
                        fit_wall_ms=wall(lambda: m.conformal_fit(alpha=alpha, **kw)), coverage_wall_ms=wall(lambda: m.coverage(fit, split=3)))
    m.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
