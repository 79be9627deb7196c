"""Ranking metrics on reddit-syn (hidden 128), HIP events and wall time — the figures of DESIGN §4.15:
  * the three launches of csrc/ranking.hip apart — gcnhip_rank_keys, gcnhip_sort_segments_u32 (2 C segments: the positives' and
    the negatives' table in one call) and gcnhip_rank_stats — for the test split and for every row, with int32 truth at C = 41
    and bit-row truth at C = 121.  The sort works in place, so it is timed behind a keys launch that rewrites its input and the
    keys launch alone is subtracted;
  * the sort against torch.sort(dim=1) of an int32 tensor of the same [2 C x n] extent on the same device in the same process, and
    against its byte floor: 2 . 4 . S . n bytes per pass actually made (the tile pass and every merge pass read and write each
    key once) at the Infinity Cache rate while the two tables fit it, else at the HBM rate (DESIGN §4.11's figures);
  * HipGCNModel.ranking() against evaluate() — one forward plus counts — and against what the parent commit offers: predict()
    (predict_multilabel(prob=True)) of the same rows plus the numpy reference on the host; wall time with a synchronisation.
Prints one JSON line.  None of the values is a pass/fail threshold.  usage: bench_ranking.py [dataset] [epochs] [--no-torch]"""
import json
import os
import sys

import numpy as np

if "--no-torch" not in sys.argv:
    import torch  # noqa: F401  (before the native libraries: one HIP runtime in the process)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_gcn_amd import datagen, ops
from cuda_gcn_amd.model import HipGCNModel
from cuda_gcn_amd.ops import Device, _ck
from tests import ranking_ref
from tools.bench_calibration import timeit, wall

IC_RATE, HBM_RATE, IC_BYTES = 8.6e12, 6.3e12, 256 << 20


def launches(dev, N, c, rows, truth, bits):
    """one keys / sort / stats launch each over `rows` (None: every row) of an [N x c] table; milliseconds"""
    lib = dev.lib
    rng = np.random.default_rng(0)
    table = dev.buf(rng.standard_normal((N, c)).astype(np.float32))
    n = N if rows is None else rows.size
    rb = dev.buf(rows) if rows is not None else None
    tb = dev.buf(truth.astype(np.int32)) if truth is not None else None
    words = ops.pack_multihot(bits) if bits is not None else None
    wb = dev.buf(words) if words is not None else None
    keys, scratch = dev.buf((2 * c, n), np.uint32), dev.buf((2 * c, n), np.uint32)
    counts = dev.buf((3 * c + 1,), np.int32)
    work = dev.buf((2 * c * ops.RANK_STATS_BLOCKS,), np.float64)
    u2, ap = dev.buf((c,), np.int64), dev.buf((c,), np.float64)
    neg_keys = keys.ptr + 4 * c * n
    cp, cn, ci, cu = (counts.ptr + 4 * k * c for k in range(4))

    def do_keys():
        _ck(lib, lib.gcnhip_rank_keys(dev.ctx, table.ptr, c, N, rb.ptr if rb else None, n, 0, c, c, tb.ptr if tb else None, wb.ptr if wb else None,
                                      words.shape[1] if words is not None else 0, keys.ptr, neg_keys, n, cp, cn, ci, cu), "keys")

    def do_sort():
        _ck(lib, lib.gcnhip_sort_segments_u32(dev.ctx, keys.ptr, scratch.ptr, n, 2 * c, n), "sort")

    def do_stats():
        _ck(lib, lib.gcnhip_rank_stats(dev.ctx, keys.ptr, neg_keys, n, n, c, cp, cn, work.ptr, u2.ptr, ap.ptr), "stats")

    res = dict(rows=n, classes=c, segments=2 * c)
    res["keys_ms"] = timeit(dev, do_keys)
    res["keys_sort_ms"] = timeit(dev, lambda: (do_keys(), do_sort()))
    res["sort_ms"] = res["keys_sort_ms"] - res["keys_ms"]
    res["sort_of_sorted_ms"] = timeit(dev, do_sort)
    res["stats_ms"] = timeit(dev, do_stats)
    passes = 1 + int(np.ceil(np.log2(max(1, -(-n // ops.SORT_TILE)))))
    table_bytes = 4 * 2 * c * n
    rate = IC_RATE if 2 * table_bytes <= IC_BYTES else HBM_RATE
    res.update(sort_passes=passes, sort_bytes=2 * table_bytes * passes, sort_floor_ms=1e3 * 2 * table_bytes * passes / rate,
               sort_floor_rate="infinity cache 8.6 TB/s" if rate == IC_RATE else "HBM 6.3 TB/s")
    res["sort_tb_s"] = res["sort_bytes"] / (res["sort_ms"] * 1e-3) / 1e12
    res["keys_bytes"] = n * c * 4 + 2 * table_bytes
    for b in (table, rb, tb, wb, keys, scratch, counts, work, u2, ap):
        if b is not None:
            b.free()
    return res


def torch_sort_ms(s, n, iters=20):
    x =torch.randint(-2 ** 31, 2 ** 31 - 1, (s, n), dtype=torch.int32, device="cuda")
    for _ in range(3):
        torch.sort(x, dim=1)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        torch.sort(x, dim=1)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def host_metrics(scores, truth):
    st = ranking_ref.table_stats(scores, truth)
    return ranking_ref.report(st["u2"], st["ap_sum"], st["pos"], st["neg"])


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    name = argv[0] if argv else "reddit-syn"
    epochs = int(argv[1]) if len(argv) > 1 else 10
    ds = datagen.make_dataset(name)
    N, c = ds["num_nodes"], ds["output_dim"]
    y = datagen.multilabel_from_communities(ds["label"], classes=121)
    test = np.flatnonzero(ds["split"] == 3).astype(np.int32)
    res = dict(dataset=name, nodes=N, test_rows=int(test.size), sort_tile=ops.SORT_TILE)
    dev = Device(0)
    for key, cc, truth, bits in (("c41", c, ds["label"], None), ("c121", 121, None, y)):
        for where, rows in (("test", test), ("all", None)):
            res[f"{key}_{where}"] = launches(dev, N, cc, rows, truth, bits)
    dev.close()
    if "--no-torch" not in sys.argv:
        for key, cc in (("c41", c), ("c121", 121)):
            for where, n in (("test", int(test.size)), ("all", N)):
                res[f"{key}_{where}"]["torch_sort_ms"] = torch_sort_ms(2 * cc, n)
    print("launches:", json.dumps(res), file=sys.stderr, flush=True)         # kept should a model below fail
    for key, kw in (("single_label", {}), ("multilabel", dict(multilabel=y))):
        m = HipGCNModel(ds, seed=1, hidden_dim=128, dropout=0.5, **kw)
        m.run_epochs(epochs, want_trace=False)
        r = dict(epochs=epochs)
        for where, q in (("test", dict(split=3)), ("all", dict(split=None))):
            r[f"ranking_{where}_wall_ms"] = wall(lambda: m.ranking(**q))
            r[f"evaluate_{where}_wall_ms"] = wall(lambda: m.evaluate(q["split"]))
            nodes = test if where == "test" else None
            if kw:
                truth = y[test] if where == "test" else y[m.row_ids()[0]]
                r[f"predict_host_{where}_wall_ms"] = wall(lambda: host_metrics(m.predict_multilabel(nodes=nodes, prob=True)[1], truth), reps=2)
            else:
                truth = ds["label"][test] if where == "test" else ds["label"][m.row_ids()[0]]
                r[f"predict_host_{where}_wall_ms"] = wall(lambda: host_metrics(m.predict(nodes=nodes, logp=True)[2], truth), reps=2)
        got = m.ranking()
        r.update(macro_auc=got["macro_auc"], macro_ap=got["macro_ap"], classes_defined=got["classes_defined"])
        m.close()
        res[key] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
