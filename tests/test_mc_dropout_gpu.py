"""Monte Carlo dropout on the GPU (csrc/mcdropout.hip, ModelQueries::mc_dropout): the two kernels through ops.Device against
the float64 reference within its carried bounds, the model's per-sample log-softmax rows against the reference forward whose
masks come from tests/dropout_ref.keep, the statistics against the kernels bit for bit, first_sample, p = 0, the temperature,
no side effect on training (between epochs), the refusals, and the command line (GCN_UNCERTAINTY).

Measured on an MI355X (largest error / tolerance over every sample, rate and row of the per-sample comparison, tolerance
2e-5 . max(1, |z|max)): see DESIGN §4.18."""
import faulthandler
import os
import signal
import subprocess
import threading

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import mc_dropout_ref as R
from tests.mr_threads import ThreadWorld

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")
TEST_LIMIT_S = 120
SENTINEL = -12345.0
FLOATS = ("confidence", "entropy", "expected_entropy", "mutual_information", "variation_ratio")


@pytest.fixture(autouse=True)
def _time_limit():
    """every test of this file ends within TEST_LIMIT_S: an alarm fails it; if the process is stuck inside a call that never
    returns, faulthandler prints the stacks and ends the process shortly after"""
    def expire(signum, frame):
        raise TimeoutError(f"test exceeded {TEST_LIMIT_S} s")
    old = signal.signal(signal.SIGALRM, expire)
    signal.alarm(TEST_LIMIT_S)
    faulthandler.dump_traceback_later(TEST_LIMIT_S + 30, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


# ---- the kernels through ops.Device ---------------------------------------------------------------------------------------

def check_against_reference(ref, acc, votes, out, C, ld_mp, fill):
    ok = ~ref["ambiguous_rows"]
    assert np.array_equal(votes, ref["votes"])                 # exact f32 inputs: no sample is ambiguous
    with np.errstate(invalid="ignore"):
        assert np.all(np.abs(acc - ref["acc"]) <= R.V * 8 * (acc.shape[1] + 8) * np.maximum(1.0, np.abs(ref["acc"])))
    assert np.array_equal(out["pred"][ok], ref["pred"][ok])
    for k in FLOATS:
        err = np.abs(out[k].astype(np.float64) - ref[k])
        assert np.all(err[ok if k == "confidence" else slice(None)] <= R.bound(ref, k)[ok if k == "confidence" else slice(None)]), (k, err.max())
    mp = out["mean_prob"]
    assert np.all(np.abs(mp[:, :C].astype(np.float64) - ref["mean_prob"]) <= R.bound(ref, "mean_prob"))
    assert np.all(mp[:, C:] == fill)                           # padding columns keep their fill


@pytest.mark.parametrize("C", [1, 2, 7, 41, 64])
def test_kernels_against_the_reference(C):
    from cuda_gcn_amd.ops import Device
    dev = Device(0)
    for n_table in (0, 1, 5, 257):
        for S in (1, 2, 5):
            l = R.kernel_samples(n_table, C, S)
            for ld in (C, C + 3):
                for rows in R.row_lists(n_table):
                    ref = R.statistics(l, rows)
                    acc, votes = dev.mc_accumulate_rows(l, rows=rows, ld=ld, fill=(SENTINEL, -777))     # `first` stores over the sentinels
                    assert acc.shape == ref["acc"].shape and votes.shape == ref["votes"].shape
                    out = dev.mc_finalize_rows(acc, votes, S, ld_mp=ld, fill=SENTINEL)
                    check_against_reference(ref, acc, votes, out, C, ld, SENTINEL)
                    # two runs give the same bits
                    acc2, votes2 = dev.mc_accumulate_rows(l, rows=rows, ld=ld, fill=(7.0, 3))
                    assert np.array_equal(bits(acc), bits(acc2)) and np.array_equal(votes, votes2)
                    out2 = dev.mc_finalize_rows(acc2, votes2, S, ld_mp=ld, fill=SENTINEL)
                    for k in out:
                        assert np.array_equal(bits(out[k]), bits(out2[k])), k
    # the planted rows, spelled out (rows in table order): the exact tie goes to the lowest class, -1e4 and -inf weigh nothing
    if C > 1:
        l = R.kernel_samples(5, C, 2)
        acc, votes = dev.mc_accumulate_rows(l)
        out = dev.mc_finalize_rows(acc, votes, 2)
        assert votes[0, 0] == 2 and out["pred"][0] == 0 and out["variation_ratio"][0] == 0
        assert acc[1, C // 2] == 0 and acc[2, 0] == 0
        assert np.all(np.isfinite(acc)) and all(np.all(np.isfinite(out[k])) for k in FLOATS)
        assert out["expected_entropy"][3] == 0                 # one-hot samples
        if C >= 4:                                             # hot classes 0 and 3: entropy ln 2, the lower class predicted
            assert out["pred"][3] == 0 and abs(out["entropy"][3] - np.log(2)) < 1e-6 and out["variation_ratio"][3] == 0.5


def test_kernels_null_outputs_out_of_table_rows_and_refusals():
    from cuda_gcn_amd.ops import Device, GcnHipError
    dev = Device(0)
    C, S = 7, 3
    l = R.kernel_samples(9, C, S)
    acc, votes = dev.mc_accumulate_rows(l)
    full = dev.mc_finalize_rows(acc, votes, S)
    # NULL outputs leave the others unchanged
    for name in Device.MC_OUTPUTS:
        part = dev.mc_finalize_rows(acc, votes, S, outputs=tuple(k for k in Device.MC_OUTPUTS if k != name))
        assert name not in part
        for k in part:
            assert np.array_equal(bits(part[k]), bits(full[k])), (name, k)
    one = dev.mc_finalize_rows(acc, votes, S, outputs=("entropy",))
    assert list(one) == ["entropy"] and np.array_equal(bits(one["entropy"]), bits(full["entropy"]))
    # a listed id outside the table adds nothing; a row listed twice has two accumulators
    rows = np.array([3, 3, -1, 9, 0], np.int32)
    ref = R.statistics(l, rows)
    acc, votes = dev.mc_accumulate_rows(l, rows=rows, fill=(SENTINEL, -777))
    assert np.array_equal(votes, ref["votes"]) and np.all(acc[2:4] == 0) and np.array_equal(bits(acc[0]), bits(acc[1]))
    # refusals: -1 with a message naming the entry point
    with pytest.raises(GcnHipError, match="gcnhip_mc_accumulate_rows: 1 <= num_classes <= 64"):
        dev.mc_accumulate_rows(np.zeros((1, 2, 65), np.float32))
    with pytest.raises(GcnHipError, match="gcnhip_mc_accumulate_rows: a row stride is below num_classes"):
        dev.mc_accumulate_rows(l, ld=C - 1)
    with pytest.raises(GcnHipError, match="gcnhip_mc_accumulate_rows: without a row list n is at most n_table"):
        dev.mc_accumulate_rows(l, n=10)
    with pytest.raises(GcnHipError, match="gcnhip_mc_finalize_rows: samples must be >= 1"):
        dev.mc_finalize_rows(acc, votes, 0)
    with pytest.raises(GcnHipError, match="gcnhip_mc_finalize_rows: a row stride is below num_classes"):
        dev.mc_finalize_rows(acc, votes, S, ld_mp=C - 1)
    with pytest.raises(GcnHipError, match="gcnhip_mc_finalize_rows: 1 <= num_classes <= 64"):
        dev.mc_finalize_rows(np.zeros((2, 66)), np.zeros((2, 65), np.int32), 1)


# ---- the model ----------------------------------------------------------------------------------------------------------------

def make_model(name, flags=0, **kw):
    from cuda_gcn_amd import model as M
    f = 0
    for k in str(flags).split("|"):
        f |= getattr(M, k) if k != "0" else 0
    ds = R.model_dataset(name)
    hyper = dict(hidden_dim=R.model_hidden(name), dropout=R.MODEL_DROPOUT)
    hyper.update(kw)
    m = M.HipGCNModel(ds, seed=R.MODEL_SEED, flags=f, **hyper)
    m.set_weights(*R.model_weights(name))
    return ds, m


@pytest.mark.parametrize("name,flags", R.MODEL_CASES)
def test_samples_match_the_reference_forward(name, flags):
    """samples=3 at the model's rate and at 0.25: every l_s against the float64 forward at the weights read back, whose masks
    come from dropout_ref.keep; tolerance 2e-5 . max(1, |z|max), test_predict_gpu.py's rule for the reference's operation order"""
    ds, m = make_model(name, flags)
    w1, w2 = m.var(2), m.var(5)
    worst = 0.0
    for p in R.MODEL_RATES:
        out = m.mc_dropout(samples=3, p=p, return_samples=True, votes=True, mean_prob=True)
        rate = R.MODEL_DROPOUT if p is None else p
        assert out["seed"] == m.stream_seed ^ R.KEY_MC_DROPOUT and out["p"] == np.float32(rate) and out["samples"] == 3 and out["first_sample"] == 0
        got = out["samples_logp"]
        assert got.shape == (3, ds["num_nodes"], ds["output_dim"]) and got.dtype == np.float32
        z, l = R.samples(ds, w1, w2, rate, out["seed"], 0, 3)
        tol = R.logit_tol(z)
        ratio = float(np.abs(got - l).max()) / tol
        worst = max(worst, ratio)
        print(f"mc_dropout {name} flags={flags} p={rate}: |z|max {np.abs(z).max():.3f} largest error / tolerance {ratio:.4f}")
        assert ratio <= 1.0, (p, ratio)
        # the statistics of the model's own rows, against the reference on those rows (votes exact outside ambiguous samples)
        ref = R.statistics(got)
        ok = ~ref["ambiguous_rows"]
        assert np.array_equal(out["votes"], ref["votes"]) and np.array_equal(out["pred"][ok], ref["pred"][ok])
        for k in FLOATS:
            sel = ok if k == "confidence" else slice(None)
            assert np.all(np.abs(out[k].astype(np.float64) - ref[k])[sel] <= R.bound(ref, k)[sel]), k
        assert np.all(np.abs(out["mean_prob"].astype(np.float64) - ref["mean_prob"]) <= R.bound(ref, "mean_prob"))
        assert float(out["mutual_information"].mean()) > 1e-3  # dropout at this rate moves the rows: the samples are not one forward
    m.close()


def test_statistics_are_the_kernels_on_the_returned_samples():
    """the two kernels through ops.Device on samples_logp give the model's outputs bit for bit — for every row, a split, and a
    query with repeats in shuffled order"""
    from cuda_gcn_amd.ops import Device
    ds, m = make_model("cora-syn")
    dev = Device(0)
    rng = np.random.default_rng(3)
    q = rng.permutation(ds["num_nodes"])[:301].astype(np.int32)
    q = np.concatenate([q, q[:7]])
    everything = m.mc_dropout(samples=4, return_samples=True)
    for kw in (dict(), dict(split=3), dict(nodes=q)):
        out = m.mc_dropout(samples=4, return_samples=True, votes=True, mean_prob=True, **kw)
        s = out["samples_logp"]
        ids = np.arange(ds["num_nodes"]) if not kw else (np.flatnonzero(ds["split"] == 3) if "split" in kw else q)
        assert s.shape[1] == ids.size
        assert np.array_equal(bits(s), bits(everything["samples_logp"][:, ids]))     # list order, the same rows whatever the subset
        acc, votes = dev.mc_accumulate_rows(s)
        fin = dev.mc_finalize_rows(acc, votes, 4)
        assert np.array_equal(votes, out["votes"])
        for k in FLOATS + ("pred", "mean_prob"):
            assert np.array_equal(bits(fin[k]), bits(out[k])), (kw.keys(), k)
    m.close()


def test_first_sample_continues_the_sequence_and_reaches_a_training_epoch():
    ds, m = make_model("planted-dense", "NO_GRAPH", learning_rate=0.0)
    a = m.mc_dropout(samples=4, return_samples=True)["samples_logp"]
    b = m.mc_dropout(samples=2, return_samples=True)["samples_logp"]
    c = m.mc_dropout(samples=2, first_sample=2, return_samples=True)["samples_logp"]
    assert np.array_equal(bits(a), bits(np.concatenate([b, c])))
    assert not np.array_equal(a[0], a[1])
    # seed = the model's own and first_sample = e: the masks of training epoch e.  With a zero learning rate the weights stay
    # the planted ones, so after two passes var(3) is the hidden layer of training epoch 1 at those weights: its zero pattern is
    # the reference's (ReLU and keep), and the query's rows are the reference's rows under the same masks
    w1, w2 = m.var(2), m.var(5)
    m.train_epoch()
    m.train_epoch()
    assert np.array_equal(m.var(2), w1) and np.array_equal(m.var(5), w2)
    h = m.var(3)
    e = 1
    adj = R.adjacency(ds)
    pre = R.aggregate(adj, R.masked_features(ds, R.MODEL_DROPOUT, m.stream_seed, e) @ w1.astype(np.float64))
    keep = R.D.keep((m.stream_seed ^ R.KEY_HIDDEN_DROPOUT) & R.M64, e, np.arange(pre.size, dtype=np.uint64), R.D.thr16(R.MODEL_DROPOUT)).reshape(pre.shape)
    edge = 1e-4 * max(1.0, float(np.abs(pre).max()))
    assert np.all(h[~keep] == 0) and np.all(h[pre < -edge] == 0) and np.all(h[keep & (pre > edge)] > 0)
    assert 0.3 < keep.mean() < 0.7
    out = m.mc_dropout(samples=1, seed=m.stream_seed, first_sample=e, return_samples=True)
    assert out["seed"] == m.stream_seed and out["first_sample"] == e
    z, l = R.samples(ds, w1, w2, R.MODEL_DROPOUT, m.stream_seed, e, 1)
    assert float(np.abs(out["samples_logp"] - l).max()) <= R.logit_tol(z)
    m.close()


def test_without_dropout_every_sample_is_the_same_forward():
    """p = 0: the samples are bit-identical, every vote agrees, pred is predict()'s on clear rows, and the mutual information is 0
    up to the float64 rounding of its two terms — entropy is formed from ln(mean_prob), expected_entropy from the f32 l itself, and
    ln(exp(l)) is l only to a rounding, so max(0, entropy - expected_entropy) is not exactly 0 on every row.  Measured on an
    MI355X (917 rows, 3 samples): largest value 6.7e-16, above 0 on 200 rows; the reference's bound for this case is 6.2e-14, and
    that bound — not a figure taken from the kernel — is what is asserted."""
    from tests.test_predict_gpu import clear_rows
    ds, m = make_model("planted-dense")
    out = m.mc_dropout(samples=3, p=0.0, return_samples=True, votes=True)
    s = out["samples_logp"]
    assert np.array_equal(bits(s[0]), bits(s[1])) and np.array_equal(bits(s[0]), bits(s[2]))
    # identical samples: the float64 work leaves at most the reference's own bound of entropy - expected entropy
    ref = R.statistics(s)
    print(f"mc_dropout p=0: largest mutual information {out['mutual_information'].max():.3e}, rows above 0: "
          f"{int((out['mutual_information'] > 0).sum())} of {out['pred'].size}, bound {ref['K']:.3e}")
    assert np.all(out["mutual_information"] <= ref["K"])
    assert np.all(out["variation_ratio"] == 0) and np.all(out["votes"].max(axis=1) == 3)
    pred, prob, logp = m.predict(logp=True)
    z = R.sample_logits(ds, m.var(2), m.var(5), 0.0, 0, 0)
    tol = 1e-4 * max(1.0, float(np.abs(z).max()))              # predict's evaluation forward reassociates its f32 sums
    ok = clear_rows(z, tol)
    assert ok.mean() > 0.9
    assert np.array_equal(out["pred"][ok], pred[ok])
    assert np.abs(s[0] - logp).max() <= tol
    m.close()


def test_temperature_scales_the_samples():
    ds, m = make_model("cora-syn")
    a = m.mc_dropout(samples=2, return_samples=True, nodes=np.array([5, 9, 5, 2000, 9], np.int32))
    full = m.mc_dropout(samples=2, return_samples=True)
    m.set_temperature(2.0)
    b = m.mc_dropout(samples=2, return_samples=True, nodes=np.array([5, 9, 5, 2000, 9], np.int32))     # a repeated node is scaled once
    full2 = m.mc_dropout(samples=2, return_samples=True)
    m.set_temperature(1.0)
    for x, y in ((a, b), (full, full2)):
        for s in range(2):
            want = R.log_softmax(x["samples_logp"][s].astype(np.float64) / 2.0)
            tol = 2e-5 * max(1.0, float(np.abs(want).max()))
            assert np.abs(y["samples_logp"][s] - want).max() <= tol
    assert np.array_equal(bits(b["samples_logp"][:, 0]), bits(b["samples_logp"][:, 2]))
    m.close()


@pytest.mark.parametrize("flags", [0, "NO_GRAPH"])
def test_a_query_between_epochs_leaves_training_alone(flags):
    """train 3 epochs, query, train 3 more: weights and metrics have the bits of a twin that never made the query (the query
    redraws the feature object's dropout bits, which the dense weight gradient reads: every training pass draws its own
    before its backward); predict() before and after the query gives the same bits"""
    from cuda_gcn_amd import model as M
    ds = datagen.make_dataset("reddit-mini")                   # dense X at hidden width 128: the split-K weight gradient reuses the forward's bits
    f = getattr(M, flags) if flags else 0
    twin, m = (M.HipGCNModel(ds, seed=R.MODEL_SEED, flags=f, hidden_dim=128, dropout=0.5) for _ in range(2))
    t1, m1 = twin.run_epochs(3), m.run_epochs(3)
    assert np.array_equal(bits(t1), bits(m1))
    before = m.predict(logp=True)
    out = m.mc_dropout(samples=3, split=3)
    assert out["pred"].size == int((ds["split"] == 3).sum())
    m.mc_dropout(samples=2, p=0.25, nodes=np.array([1, 2, 3], np.int32))
    after = m.predict(logp=True)
    for x, y in zip(before, after):
        assert np.array_equal(bits(x), bits(y))
    t2, m2 = twin.run_epochs(3), m.run_epochs(3)
    assert np.array_equal(bits(t2), bits(m2))
    for k in (2, 5):
        assert np.array_equal(bits(twin.var(k)), bits(m.var(k))), k
    assert twin.train_epoch() == m.train_epoch() and twin.eval(3) == m.eval(3)
    twin.close()
    m.close()


def test_refusals_leave_the_model_answering():
    """every refusal of the host call (through the C entry, past the Python checks), then a predict()"""
    import ctypes as C
    from cuda_gcn_amd import model as M
    from cuda_gcn_amd.model import HipGCNModel, GcnHostError, _ck
    ds, m = make_model("cora-syn")
    before = m.predict()
    n_nodes = ds["num_nodes"]

    def direct(model, split=0, nodes=None, samples=2, p=None, first=0):
        q = None if nodes is None else np.ascontiguousarray(nodes, np.int32)
        pp = C.c_float(p) if p is not None else None
        rows = C.c_int64()
        pred = np.zeros(n_nodes, np.int32)
        rc = model.lib.gcnhost_model_mc_dropout(model.h, split, q.ctypes.data if q is not None else None, 0 if q is None else q.size, samples,
                                                C.byref(pp) if pp is not None else None, None, first, n_nodes, pred.ctypes.data, *([None] * 10),
                                                C.byref(rows))
        _ck(model.lib, rc, "call")

    for kw, match in ((dict(samples=0), "samples must be in 1..1024"), (dict(samples=1025), "samples must be in 1..1024"),
                      (dict(p=1.0), r"p must be in \[0, 1\)"), (dict(p=-0.5), r"p must be in \[0, 1\)"), (dict(p=float("nan")), r"p must be in \[0, 1\)"),
                      (dict(first=2 ** 32 - 1, samples=2), "first_sample \\+ samples is above 2\\^32"), (dict(split=4), "split is 0 with a node query"),
                      (dict(split=-1), "split is 0 with a node query"), (dict(nodes=[0, n_nodes]), "is not a node of the dataset"),
                      (dict(nodes=[-1]), "is not a node of the dataset")):
        with pytest.raises(GcnHostError, match="mc_dropout: .*" + match):
            direct(m, **kw)
    with pytest.raises(GcnHostError, match="mc_dropout: the query lists 3 rows"):
        rows = C.c_int64()
        q = np.array([1, 2, 3], np.int32)
        pred = np.zeros(2, np.int32)
        _ck(m.lib, m.lib.gcnhost_model_mc_dropout(m.h, 0, q.ctypes.data, 3, 2, None, None, 0, 2, pred.ctypes.data, *([None] * 10), C.byref(rows)), "call")
    after = m.predict()
    assert np.array_equal(before[0], after[0]) and np.array_equal(bits(before[1]), bits(after[1]))
    assert m.mc_dropout(samples=1, nodes=np.zeros(0, np.int32))["pred"].size == 0           # an empty query is a query
    m.close()
    # models the call does not take: each refusal, then a prediction of its own kind
    y = np.zeros((n_nodes, 9), bool)
    y[np.arange(n_nodes), ds["label"] % 9] = True
    ml = HipGCNModel(ds, seed=1, multilabel=y, hidden_dim=16)
    with pytest.raises(GcnHostError, match="mc_dropout: this is a multi-label model"):
        direct(ml)
    assert ml.predict_multilabel().shape == (n_nodes, 9)
    ml.close()
    wide = HipGCNModel(dict(ds, output_dim=65), seed=1, hidden_dim=16)
    with pytest.raises(GcnHostError, match="mc_dropout: at most 64 classes"):
        direct(wide)
    wide.close()
    bf = HipGCNModel(ds, seed=1, flags=M.BF16_TABLES, hidden_dim=16)
    with pytest.raises(GcnHostError, match="mc_dropout: not with bf16 tables"):
        direct(bf)
    assert bf.predict()[0].size == n_nodes
    bf.close()
    tiny = datagen.make_dataset("tiny-syn")
    n_nodes = tiny["num_nodes"]
    fat = HipGCNModel(tiny, seed=1, hidden_dim=257)
    with pytest.raises(GcnHostError, match="mc_dropout: a hidden width of at most 256"):
        direct(fat)
    assert fat.predict()[0].size == n_nodes
    fat.close()
    # two logical ranks: refused on each, predict works
    tw = ThreadWorld(2)
    seen, errors = [None, None], []

    def body(rank):
        try:
            ag, ar = tw.callbacks(rank)
            r = HipGCNModel(tiny, seed=4, device=0, rank=rank, world=2, host_allgather=ag, host_allreduce=ar, hidden_dim=16, dropout=0.5)
            try:
                direct(r)
                msg = "no error"
            except GcnHostError as e:
                msg = str(e)
            seen[rank] = (msg, r.predict()[0].size)
            r.close()
        except BaseException as e:                                # a failed rank must not leave the other at a barrier forever
            errors.append((rank, e))
            tw.barrier.abort()
    threads = [threading.Thread(target=body, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert all("mc_dropout: one rank only" in msg and n > 0 for msg, n in seen), seen


# ---- the command line -----------------------------------------------------------------------------------------------------------

def test_cli_uncertainty_file_equals_the_python_call(tmp_path):
    """gcn-hip cora-syn with GCN_SAVE_WEIGHTS and GCN_UNCERTAINTY: the printed line parses, and the file equals the Python call on
    the loaded weights with the same seed and samples"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.make_dataset("cora-syn")
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "cora-syn.gcnbin"))
    w, u = str(tmp_path / "w.gcnw"), str(tmp_path / "u.txt")
    r = subprocess.run(["timeout", "-k", "10", "60", HIP, "cora-syn", "-", "-", "16", "-", "0.5", "-", "-", "5"], cwd=str(tmp_path),
                       env=dict(os.environ, GCN_SEED="3", GCN_SAVE_WEIGHTS=w, GCN_UNCERTAINTY=u, GCN_MC_SAMPLES="6", GCN_MC_SEED="12345"),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    mc = [x for x in lines if x.startswith("mc_samples=")]
    assert len(mc) == 1 and lines[-1] == mc[0] and lines[-2].startswith("test_loss="), lines[-3:]     # after the test line
    f = dict(kv.split("=") for kv in mc[0].split())
    assert list(f) == ["mc_samples", "mc_test_acc", "mc_mean_entropy", "mc_mean_mutual_information"] and f["mc_samples"] == "6"
    rows = np.loadtxt(u, ndmin=2)
    test = np.flatnonzero(ds["split"] == 3)
    assert rows.shape == (test.size, 5) and np.array_equal(rows[:, 0].astype(np.int64), test)
    m = HipGCNModel(ds, seed=3, hidden_dim=16, dropout=0.5)
    m.load_weights(w)
    out = m.mc_dropout(nodes=test.astype(np.int32), samples=6, seed=12345)
    m.close()
    assert np.array_equal(rows[:, 1].astype(np.int32), out["pred"])
    for col, k in ((2, "confidence"), (3, "entropy"), (4, "mutual_information")):
        assert np.array_equal(rows[:, col].astype(np.float32), out[k]), k                       # %.9g is exact for every f32
    assert f"{np.mean(out['pred'] == ds['label'][test]):.5f}" == f["mc_test_acc"]
    assert abs(float(f["mc_mean_entropy"]) - float(out["entropy"].astype(np.float64).mean())) < 1e-5
    assert abs(float(f["mc_mean_mutual_information"]) - float(out["mutual_information"].astype(np.float64).mean())) < 1e-5
