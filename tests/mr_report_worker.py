"""Worker of the several-rank evaluation test (tests/test_report_gpu.py): one process per rank, torch.distributed gloo
rendezvous on 127.0.0.1, every rank on GPU 0 with the host-staged transport (the callbacks of tests/mr_worker.py).
Each rank loads the weights file it is given, calls evaluate() for the three splits and for all nodes (a collective: every
rank gets the totals over all ranks), predicts its own rows and reports them by dataset node id; rank 0 writes every rank's
totals and the union of the predictions.  argv: dataset (a datagen name, or `multilabel-<C>` for
datagen.planted_multilabel(classes=C)), weights file, output .npz, flags, hidden width."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.mr_worker import make_callbacks  # noqa: E402


def main():
    name, weights, out, flags, hidden = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from cuda_gcn_amd import datagen, model
    ml = name.startswith("multilabel-")
    ds = datagen.planted_multilabel(classes=int(name.split("-")[1])) if ml else datagen.make_dataset(name)
    ag, ar = make_callbacks(dist, world)
    m = model.HipGCNModel(ds, seed=11, device=0, flags=flags, rank=rank, world=world, host_allgather=ag, host_allreduce=ar,
                          hidden_dim=hidden, dropout=0.5, multilabel=ds["multilabel"] if ml else None)
    m.load_weights(weights)
    ids, _ = m.row_ids()
    key = ("tp", "fp", "fn") if ml else ("confusion",)
    totals = {}
    for tag, kw in (("s1", dict(split=1)), ("s2", dict(split=2)), ("s3", dict(split=3)), ("all", dict())):
        r = m.evaluate(**kw)
        totals[tag] = np.stack([r[k] for k in key]) if ml else r["confusion"]
        totals[tag + "_rows"] = np.array([r["rows"], r.get("unlabelled", 0)], np.int64)
    # a query of some of this rank's own nodes (with a repeat): the other ranks pass theirs, the totals cover all of them
    q = np.concatenate([ids[::3], ids[:1]]).astype(np.int32)
    r = m.evaluate(nodes=q)
    totals["query"] = np.stack([r[k] for k in key]) if ml else r["confusion"]
    pred = m.predict_multilabel() if ml else m.predict()[0]
    m.close()
    gathered = [None] * world
    dist.all_gather_object(gathered, (ids, pred, q, totals))
    if rank == 0:
        N = ds["num_nodes"]
        P = np.zeros((N, ds["multilabel"].shape[1]), bool) if ml else np.full(N, -1, np.int32)
        for i, p, _, _ in gathered:
            P[i] = p
        save = dict(pred=P, query=np.concatenate([g[2] for g in gathered]))
        for r_, g in enumerate(gathered):
            for k, v in g[3].items():
                save[f"r{r_}_{k}"] = v
        np.savez(out, **save)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
