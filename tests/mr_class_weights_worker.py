"""Worker of the two-rank class-weights test (tests/test_class_weights_gpu.py): one process per rank, torch.distributed gloo on
127.0.0.1, every rank on GPU 0 with the host-staged transport (tests/mr_worker.py).  Each rank loads the initial weights and
trains 5 epochs (train + validation); rank 0 writes the trace.  argv: initial weights, output .npz, multilabel (0 / 1)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.mr_worker import make_callbacks  # noqa: E402

ID_PARTITION = 4194304


def dataset_and_weights(multilabel):
    """(ds, Y or None, weights).  Single-label: unshuffled communities (ids in community order), 8 classes over 8 communities, so
    every node of class 7 — the class with by far the largest weight — has an id in the second half: rank 0 of 2 owns none."""
    from cuda_gcn_amd import datagen
    if multilabel:
        ds = datagen.planted_multilabel(classes=121)
        y = ds["multilabel"]
        pw = np.random.default_rng(2).uniform(0.1, 10, 121).astype(np.float32)
        return ds, y, pw
    ds = datagen.planted_communities(n_comm=8, size=256, classes=8, shuffle=False)
    w = np.array([1, 0.5, 2, 1, 0.25, 1.5, 1, 25], np.float32)
    return ds, None, w


def main():
    w0, out, multilabel = sys.argv[1], sys.argv[2], int(sys.argv[3])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from cuda_gcn_amd import model
    ds, y, w = dataset_and_weights(multilabel)
    ag, ar = make_callbacks(dist, world)
    m = model.HipGCNModel(ds, seed=11, device=0, flags=ID_PARTITION, rank=rank, world=world, host_allgather=ag, host_allreduce=ar,
                          hidden_dim=16, dropout=0.0, multilabel=y, class_weights=w)
    m.load_weights(w0)
    trace = np.array([m.train_epoch() + m.eval(2) for _ in range(5)], np.float32)
    ids, renumbered = m.row_ids()
    assert not renumbered
    rare = int(np.sum(ds["label"][ids] == 7)) if not multilabel else -1
    m.close()
    gathered = [None] * world
    dist.all_gather_object(gathered, rare)
    if rank == 0:
        np.savez(out, trace=trace, rank0_rare_rows=np.array(gathered[0]))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
