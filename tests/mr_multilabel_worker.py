"""Worker of the two-rank multi-label test (tests/test_multilabel_gpu.py): one process per rank, torch.distributed gloo on
127.0.0.1, every rank on GPU 0 with the host-staged transport (tests/mr_worker.py).  Each rank loads the initial weights,
trains 5 epochs (train + validation), then loads the one-rank model's final weights and predicts its own rows; rank 0 writes
the trace and the union of the predicted sets by dataset node id.  argv: initial weights, final weights, output .npz, flags."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.mr_worker import make_callbacks  # noqa: E402


def main():
    w0, w, out, flags = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from cuda_gcn_amd import datagen, model
    ds = datagen.planted_multilabel(classes=121)
    ag, ar = make_callbacks(dist, world)
    m = model.HipGCNModel(ds, seed=11, device=0, flags=flags, rank=rank, world=world, host_allgather=ag, host_allreduce=ar,
                          hidden_dim=16, dropout=0.0, multilabel=ds["multilabel"])
    m.load_weights(w0)
    trace = np.array([m.train_epoch() + m.eval(2) for _ in range(5)], np.float32)
    m.load_weights(w)
    ids, renumbered = m.row_ids()
    sets, prob = m.predict_multilabel(prob=True)
    q = np.random.default_rng(rank).permutation(ids)[:min(40, ids.size)]
    pos = {int(n): i for i, n in enumerate(ids)}
    assert np.array_equal(m.predict_multilabel(nodes=q), sets[[pos[int(n)] for n in q]])
    m.close()
    gathered = [None] * world
    dist.all_gather_object(gathered, (ids, sets, prob, renumbered))
    if rank == 0:
        N, C = ds["num_nodes"], 121
        S, P = np.zeros((N, C), bool), np.full((N, C), np.nan, np.float32)
        for i, s, p, _ in gathered:
            S[i], P[i] = s, p
        np.savez(out, sets=S, prob=P, trace=trace, renumbered=np.array(any(g[3] for g in gathered)))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
