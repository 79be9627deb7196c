"""Exact t-SNE on the GPU (csrc/tsne.hip through ops.py and the model) against the float64 reference of tests/tsne_ref.py; the
real-valued cases inside 8 times the reference's own sensitivity to f32 distances, never below 2^-20."""
import os
import subprocess
import threading

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import tsne_ref as R
from tests.silhouette_ref import blobs
from tests.test_kmeans_gpu import dev, integer_table, row_list, same_bits, strides      # noqa: F401 (dev: the Device fixture)
from tests.test_silhouette_gpu import trained_planted                                    # noqa: F401 (the planted-communities model)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")
DIMS = [1, 5, 16, 41, 128, 256]
FLOOR = 2.0 ** -20


@pytest.mark.parametrize("dim", DIMS)
def test_bandwidths_on_integer_tables(dev, dim):
    """193 positions with repeats, -1 and an id past the table; a duplicated row; a row far from all others.  Where the float64
    reference's own search cannot converge (more exact copies of a row than the perplexity) the kernel must not either:
    unconverged is the reference's count, 0 wherever the reference converges."""
    t = integer_table(283, dim, 40 + dim)
    rows = row_list(283, dim)                                     # 193 positions
    t[rows[3]] = t[rows[4]]
    t[rows[8]] = 50.0                                             # d2 stays an exact f32 integer: 256 . 53^2 < 2^24
    assert rows.size == 193
    xs, ok = R.scaled_rows(t, rows)
    d2 = R.dist2(xs, ok)
    plan = dev.tsne_plan(193, dim)
    for perplexity in (2.0, 30.0):
        _, conv = R.bandwidths(d2, perplexity)
        got = []
        for sbytes in (plan["bytes"], plan["bytes_min"], (plan["bytes"] + plan["bytes_min"]) // 2 // 16 * 16):
            pk = dev.tsne_pack(t, rows=rows, ld=strides(dim, 1), scratch_bytes=sbytes)
            assert pk["points"] == int(ok.sum()) == 191
            got.append(dev.tsne_bandwidths(pk, perplexity))
            assert all(same_bits(got[0][key], got[-1][key]) for key in ("beta", "m", "inv_z")), sbytes
        b = got[0]
        assert all(np.all(np.isnan(b[key][~ok])) for key in ("beta", "m", "inv_z")) and np.all(np.isfinite(b["beta"][ok]))
        H, z, m = R.entropy(d2[ok], b["beta"][ok])
        assert same_bits(b["m"][ok], m.astype(np.float32))
        err = np.abs(H - np.log(perplexity))[conv[ok]]
        print(f"dim {dim} perplexity {perplexity}: unconverged {b['unconverged']}, |H - target| max {err.max(initial=0):.3e}")
        assert b["unconverged"] == int((ok & ~conv).sum()) and np.all(err <= 1e-5 + 1e-9)
        assert np.all(np.abs(b["inv_z"][ok] * z - 1.0) <= 1e-12) and np.isfinite(b["inv_z"][8]) and b["inv_z"][8] > 0


def reference_pair(x, perplexity):
    """(P from float64 d2, P from the kernel's f32 d2), each with its own float64 bandwidths"""
    xs, ok = R.scaled_rows(x)
    out = []
    for f32 in (False, True):
        d2 = R.dist2(xs, ok, f32=f32)
        out.append(R.joint(d2, R.bandwidths(d2, perplexity)[0]))
    return out


@pytest.mark.parametrize("n,dim", [(193, d) for d in DIMS] + [(2100, 16)])
def test_gradient_on_real_tables(dev, n, dim):
    x = blobs(n, dim, 8, 7 + dim)[0]
    P64, P32 = reference_pair(x, 30.0)
    pk = dev.tsne_pack(x, ld=strides(dim, 0))
    small = dev.tsne_pack(x, scratch_bytes=dev.tsne_plan(n, dim)["bytes_min"])
    for p in (pk, small):
        assert dev.tsne_bandwidths(p, 30.0)["unconverged"] == 0
    rng = np.random.default_rng(dim)
    for k, scale, ex in [(k, s, e) for k in (2, 3) for s in (1e-4, 1.0, 20.0) for e in (1.0, 12.0)]:
        y = (scale * rng.standard_normal((n, k))).astype(np.float32)
        g64, zq, kl = R.gradient(P64, y, ex)
        g32, _, kl32 = R.gradient(P32, y, ex)
        tol_g = max(8 * np.abs(g32 - g64).max() / np.abs(g64).max(), FLOOR)
        tol_kl = max(8 * abs(kl32 - kl) / abs(kl), FLOOR)
        got = dev.tsne_gradient(pk, y, exaggeration=ex)
        err_g, err_kl = np.abs(got["grad"] - g64).max() / np.abs(g64).max(), abs(got["kl"] - kl) / abs(kl)
        print(f"n {n} dim {dim} k {k} scale {scale} exaggeration {ex}: grad {err_g:.2e} (allowed {tol_g:.2e}), kl {err_kl:.2e} ({tol_kl:.2e}), "
              f"zq {abs(got['zq'] - zq) / zq:.2e}")
        assert err_g <= tol_g and err_kl <= tol_kl and abs(got["zq"] - zq) <= FLOOR * zq
        assert abs(got["grad_norm"] - np.sqrt((g64 ** 2).sum())) <= 2 * tol_g * np.sqrt((g64 ** 2).sum())
        for p in (pk, small):                                     # a second launch, and the least scratch
            again = dev.tsne_gradient(p, y, exaggeration=ex)
            assert same_bits(again["grad"], got["grad"]) and again["kl"] == got["kl"] and again["zq"] == got["zq"]
        assert same_bits(dev.tsne_gradient(pk, y, exaggeration=ex, want_kl=False)["grad"], got["grad"])


def test_iterations_follow_the_float64_trajectory(dev):
    """the margin is the reference's own f32-d2 trajectory against its float64 one, times 8"""
    x = blobs(193, 16, 8, 3)[0]
    P64, P32 = reference_pair(x, 30.0)
    y0 = 1e-4 * np.random.default_rng(5).standard_normal((193, 2))
    want, near = R.run(P64, y0, 20, exaggeration_iters=10), R.run(P32, y0, 20, exaggeration_iters=10)
    tol = max(8 * np.abs(near - want).max() / np.abs(want).max(), FLOOR)
    got = dev.tsne_run(x, y0, iters=20, exaggeration_iters=10, kl_every=8)
    err = np.abs(got["coords"] - want).max() / np.abs(want).max()
    print(f"trajectory: {err:.2e} (allowed {tol:.2e}); history {got['history'].tolist()}")
    assert err <= tol and got["learning_rate"] == 50.0 and got["points"] == 193 and got["unconverged"] == 0
    assert np.array_equal(got["history"][:, 0], [7, 15, 19]) and got["kl"] == got["history"][-1, 1]
    pk = dev.tsne_pack(x)                                         # the last history row is the gradient call at the map of 19 iterations
    dev.tsne_bandwidths(pk, 30.0)
    last = dev.tsne_gradient(pk, dev.tsne_run(x, y0, iters=19, exaggeration_iters=10)["coords"])
    assert got["kl"] == last["kl"] and got["history"][-1, 2] == last["grad_norm"]


def test_tsne_is_the_ops_path_on_the_models_rows(dev, trained_planted):
    ds, m = trained_planted
    before = m.predict(logp=True)
    got = m.tsne(split=3, iters=30)
    assert all(same_bits(a, b) for a, b in zip(before, m.predict(logp=True)))
    table = m.embed()
    test_nodes = np.flatnonzero(np.asarray(ds["split"]) == 3).astype(np.int32)
    co = m.pca(k=2, split=3)["coords"].astype(np.float64)
    y0 = co * float(np.float32(1e-4 / co[:, 0].std()))
    want = dev.tsne_run(table, y0, iters=30, rows=test_nodes, inv_norm=dev.embed_inv_norms(table))
    assert same_bits(got["coords"], want["coords"]) and same_bits(got["beta"], want["beta"]) and same_bits(got["history"], want["history"])
    assert got["kl"] == want["kl"] and got["points"] == test_nodes.size and got["unconverged"] == 0 and got["learning_rate"] == want["learning_rate"]
    other = m.tsne(k=3, data=m.pca(k=5)["coords"], iters=3, init=np.random.default_rng(0).standard_normal((1024, 3)), scratch_bytes=1)
    assert other["coords"].shape == (1024, 3) and np.all(np.isfinite(other["coords"]))


def test_a_tsne_call_between_epochs_changes_nothing():
    from cuda_gcn_amd import model as M
    ds = datagen.make_dataset("cora-syn")
    a = M.HipGCNModel(ds, seed=6, hidden_dim=16, dropout=0.5)
    b = M.HipGCNModel(ds, seed=6, hidden_dim=16, dropout=0.5)
    ta, tb = [a.run_epochs(3)], [b.run_epochs(3)]
    b.tsne(split=3, iters=5)
    ta.append(a.run_epochs(2))
    tb.append(b.run_epochs(2))
    ta, tb = np.concatenate(ta), np.concatenate(tb)
    assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32)), (ta, tb)
    assert a.eval(3) == b.eval(3) and all(same_bits(a.var(v), b.var(v)) for v in (2, 3, 5, 6))
    a.close()
    b.close()


def test_it_is_a_map(dev):
    """on this input the float64 reference reaches a label share of 0.83 to 0.84 from 50 iterations on, the PCA coordinates 0.786"""
    x, lab = blobs(1024, 16, 8, 1)
    co, y0 = R.pca_start(x)
    got = dev.tsne_run(x, y0, iters=100)
    share, yard = R.label_share(got["coords"], lab), R.label_share(co, lab)
    print(f"10-neighbour label share: t-SNE {share:.4f}, PCA {yard:.4f}, kl {got['kl']:.4f}")
    assert share >= yard and got["unconverged"] == 0


def test_refusals(dev):
    from cuda_gcn_amd import model as M
    from cuda_gcn_amd.model import HipGCNModel, GcnHostError
    from cuda_gcn_amd.ops import GcnHipError
    from tests.mr_threads import ThreadWorld
    x = blobs(64, 4, 2, 0)[0]
    pk = dev.tsne_pack(x)
    for perplexity in (63.0, 0.5):
        with pytest.raises(GcnHipError, match=r"perplexity must be in \[1, n_points - 1\)"):
            dev.tsne_bandwidths(pk, perplexity)
    dev.tsne_bandwidths(pk, 5.0)
    with pytest.raises(GcnHipError, match="k must be 2 or 3"):
        dev.tsne_gradient(pk, np.zeros((64, 4)))
    ds = datagen.make_dataset("tiny-syn")
    n = ds["num_nodes"]
    m = HipGCNModel(ds, seed=1, hidden_dim=16)
    for kwargs, msg in ((dict(k=4), "k must be 2 or 3"), (dict(perplexity=n - 1, iters=2), "perplexity must be in"),
                        (dict(init=np.zeros((n, 3))), "the start must have shape"), (dict(split=3, init=np.zeros((n, 2))), "the query lists")):
        with pytest.raises(GcnHostError, match="tsne: " + msg):
            m.tsne(**kwargs)
    m.close()
    bf = HipGCNModel(ds, seed=1, flags=M.BF16_TABLES, hidden_dim=16)
    with pytest.raises(GcnHostError, match="tsne: not with bf16 tables"):
        bf.tsne(init=np.zeros((n, 2)))
    bf.close()
    tw = ThreadWorld(2)
    seen, errors = [None, None], []

    def body(rank):
        try:
            ag, ar = tw.callbacks(rank)
            r = HipGCNModel(ds, seed=4, device=0, rank=rank, world=2, host_allgather=ag, host_allreduce=ar, hidden_dim=16, dropout=0.5)
            try:
                r.tsne(init=np.zeros((n, 2)))
                seen[rank] = "no error"
            except GcnHostError as e:
                seen[rank] = str(e)
            r.close()
        except BaseException as e:                                # a failed rank must not leave the other at a barrier forever
            errors.append((rank, e))
            tw.barrier.abort()
    threads = [threading.Thread(target=body, args=(r,)) for r in range(2)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errors, errors
    assert all("tsne: one rank only" in s for s in seen), seen


def test_cli_tsne(tmp_path):
    """GCN_TSNE writes the map m.tsne gives for the test split, to %.9g; a run without the variable prints what it printed before"""
    from cuda_gcn_amd.model import HipGCNModel, read_tsne
    ds = datagen.make_dataset("cora-syn")
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "cora-syn.gcnbin"))
    m = HipGCNModel(ds, seed=3, hidden_dim=16, dropout=0.5)
    m.run_epochs(6, want_trace=False)
    w = str(tmp_path / "w.gcnw")
    m.save_weights(w)
    want = m.tsne(split=3, perplexity=20.0, iters=25)
    m.close()
    args = ["timeout", "-k", "10", "50", HIP, "cora-syn", "-", "-", "16", "-", "0.5", "-", "-", "0"]
    env = dict(os.environ, GCN_SEED="3", GCN_LOAD_WEIGHTS=w)
    [env.pop(key, None) for key in ("GCN_TSNE", "GCN_TSNE_ITERS", "GCN_TSNE_PERPLEXITY")]
    out = str(tmp_path / "t.txt")
    r0 = subprocess.run(args, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    r1 = subprocess.run(args, cwd=str(tmp_path), env=dict(env, GCN_TSNE=out, GCN_TSNE_ITERS="25", GCN_TSNE_PERPLEXITY="20"), capture_output=True, text=True)
    assert r0.returncode == 0 and r1.returncode == 0, (r0.stderr[-1000:], r1.stderr[-1000:])
    l0, l1 = r0.stdout.strip().splitlines(), r1.stdout.strip().splitlines()
    assert len(l1) == len(l0) + 1 and "tsne" not in r0.stdout and [s.split("=")[0] for s in l1[-1].split()] == [
        "tsne_rows", "tsne_perplexity", "tsne_iters", "tsne_kl", "tsne_unconverged"]
    fields = dict(p.split("=") for p in l1[-1].split())
    got = read_tsne(out)
    assert np.array_equal(got["node"], np.flatnonzero(np.asarray(ds["split"]) == 3)) and int(fields["tsne_rows"]) == got["node"].size
    assert np.array_equal(got["coords"], np.array([[float("%.9g" % v) for v in row] for row in want["coords"]]))
    assert float(fields["tsne_kl"]) == float("%.9g" % want["kl"]) and fields["tsne_unconverged"] == "0" and fields["tsne_iters"] == "25"
