"""The CPU-measured figures of DESIGN §4.12 ("what it is for"), with no GPU: the CPU oracle trains the planted-communities model
(8 x 128 nodes, deg 16, p_in 0.5, 32 features, 8 classes, seed 5; hidden 16, no dropout, seed 5, 30 epochs) and the float64
reference of tests/explain_ref.py explains every test node for its predicted class.  Prints, and returns from measure():
the share of test nodes whose largest feature share is the planted column pred % feats (REF_TOP_FEATURE of
tests/test_explain_model_gpu.py), the share of open queries (REF_OPEN), and the share of sum |share| on the 8 informative columns."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from cuda_gcn_amd import datagen
from tests import explain_ref as R


def measure(oracle=None, epochs=30):
    if oracle is None:
        from oracle.pyoracle import Oracle
        oracle = Oracle()
    ds = datagen.planted_communities(n_comm=8, size=128, deg=16, p_in=0.5, feats=32, classes=8, seed=5)
    n, nf, nc, h = ds["num_nodes"], ds["input_dim"], ds["output_dim"], 16
    m = oracle.model(ds, seed_time=5, hidden_dim=h, dropout=0.0)
    for _ in range(epochs):
        m.train_epoch()
    test_acc = m.eval(3)[1]
    w1, w2, h1 = np.array(m.var(2)).reshape(nf, h), np.array(m.var(5)).reshape(h, nc), np.array(m.var(3)).reshape(n, h)
    m.close()
    ip, ix = ds["g_indptr"].astype(np.int64), ds["g_indices"].astype(np.int64)
    deg = np.diff(ip).astype(np.float64)
    src = np.repeat(np.arange(n), np.diff(ip))
    coef = 1 / np.sqrt(deg[src] * deg[ix])
    s, s_abs, terms = R.layer1(ip, ix, coef, ds["f_val"].reshape(n, nf).astype(np.float64))
    pred = R.layer1(ip, ix, coef, h1.astype(np.float64) @ w2)[0].argmax(1)
    test = np.flatnonzero(ds["split"] == 3)
    refs = [R.explain64(ip, ix, coef, h1, w2, int(v), int(pred[v]), w1=w1, s=s, s_abs=s_abs, terms=terms) for v in test]
    hit, opened, _ = R.top_feature_agreement(None, refs, pred[test] % nf)
    mass = float(np.mean([np.abs(r["feat"][:nc]).sum() / np.abs(r["feat"]).sum() for r in refs]))
    return dict(test_nodes=int(test.size), test_acc=float(test_acc), top_feature=hit, open=opened, informative_mass=mass)


if __name__ == "__main__":
    print(measure())
