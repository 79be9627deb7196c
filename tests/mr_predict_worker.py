"""Worker of the several-rank prediction test (tests/test_predict_gpu.py): one process per rank, torch.distributed gloo
rendezvous on 127.0.0.1, every rank on GPU 0 with the host-staged transport (the callbacks of tests/mr_worker.py).
Each rank loads the weights file it is given, predicts its own rows and reports them by dataset node id; rank 0 writes
the union.  argv: dataset (a datagen name, or `planted` for datagen.planted_communities()), weights file, output .npz,
flags, hidden width."""
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
    ds = datagen.planted_communities() if name == "planted" else datagen.make_dataset(name)
    ag, ar = make_callbacks(dist, world)
    m = model.HipGCNModel(ds, seed=11, device=0, flags=flags, rank=rank, world=world, host_allgather=ag, host_allreduce=ar,
                          hidden_dim=hidden, dropout=0.5)
    m.load_weights(weights)
    ids, renumbered = m.row_ids()
    pred, prob, logp = m.predict(logp=True)
    # a query of this rank's own nodes, in dataset ids and shuffled, gives the same bits
    rng = np.random.default_rng(rank)
    q = rng.permutation(ids)[:min(50, ids.size)]
    qp, qq = m.predict(nodes=q)
    pos = {int(n): i for i, n in enumerate(ids)}
    sel = np.array([pos[int(n)] for n in q], np.int64)
    assert np.array_equal(qp, pred[sel]) and np.array_equal(qq.view(np.uint32), prob[sel].view(np.uint32))
    # a node of another rank is an error, not a silent answer
    others = np.setdiff1d(np.arange(ds["num_nodes"]), ids)
    try:
        m.predict(nodes=others[:1])
        raise AssertionError("a node of another rank was accepted")
    except model.GcnHostError as e:
        assert "is not a row of rank" in str(e), e
    test = m.eval(3)
    m.close()
    gathered = [None] * world
    dist.all_gather_object(gathered, (ids, pred, prob, logp, renumbered))
    if rank == 0:
        N, C = ds["num_nodes"], ds["output_dim"]
        P, Q, L = np.full(N, -1, np.int32), np.full(N, np.nan, np.float32), np.full((N, C), np.nan, np.float32)
        for i, p, q2, lp, _ in gathered:
            P[i], Q[i], L[i] = p, q2, lp
        np.savez(out, pred=P, prob=Q, logp=L, renumbered=np.array(any(g[4] for g in gathered)), test=np.array(test, np.float32))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
