"""Time HipGCNModel.predict() on reddit-syn (hidden 128, 41 classes): every node, and a query of 1 024 nodes, against one
evaluation forward (eval(2)) of the same model.  Each figure is the mean over --iters synchronised calls after --warmup calls,
timed with HIP events (torch.cuda.Event, recorded before and after the calls; every call synchronises its own stream) and
with the host clock.  predict() = the evaluation forward with the prediction epilogue in the logit aggregation + the copy of
pred / prob to the host (+ a row subset registered for a new query).  The script ends itself after --limit seconds.

    python tools/bench_predict.py [--dataset reddit-syn] [--iters 20] [--warmup 3] [--limit 600]
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="reddit-syn")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=600)
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: sys.exit("bench_predict: time limit reached"))
    signal.alarm(a.limit)
    import torch
    from cuda_gcn_amd import datagen
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.make_dataset(a.dataset)
    m = HipGCNModel(ds, seed=1, hidden_dim=128, dropout=0.5)
    for _ in range(3):
        m.train_epoch()
    q = np.random.default_rng(0).permutation(ds["num_nodes"])[:1024].astype(np.int32)

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
        return e0.elapsed_time(e1) / a.iters, 1e3 * (time.perf_counter() - t0) / a.iters
    ev_ms, ev_host = timed(lambda: m.eval(2))
    all_ms, all_host = timed(lambda: m.predict())
    q_ms, q_host = timed(lambda: m.predict(nodes=q))
    m.close()
    out = dict(dataset=a.dataset, nodes=int(ds["num_nodes"]), iters=a.iters, eval_forward_ms=round(ev_ms, 4),
               predict_all_ms=round(all_ms, 4), predict_all_share_of_eval=round(all_ms / ev_ms, 3),
               predict_1024_ms=round(q_ms, 4), predict_1024_share_of_eval=round(q_ms / ev_ms, 3),
               host_clock_ms=dict(eval=round(ev_host, 4), predict_all=round(all_host, 4), predict_1024=round(q_host, 4)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
