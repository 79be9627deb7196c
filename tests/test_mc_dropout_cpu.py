"""Monte Carlo dropout without a GPU: the closed forms of the float64 reference (tests/mc_dropout_ref.py), the conditions the
GPU tests' inputs must meet — checked here so that the reference alone meets them —, the exported symbols and the argument
refusals of HipGCNModel.mc_dropout that need no device."""
import numpy as np
import pytest

from tests import mc_dropout_ref as R


# ---- closed forms of the reference --------------------------------------------------------------------------------------

def test_identical_samples_carry_no_mutual_information():
    l = R.kernel_samples(9, 7, 1)[0]
    for S in (1, 2, 5):
        ref = R.statistics(np.stack([l] * S))
        one = R.statistics(l[None])
        assert np.all(ref["mutual_information"] <= 2 * ref["K"])
        assert np.allclose(ref["entropy"], ref["expected_entropy"], rtol=0, atol=2 * ref["K"])
        assert np.allclose(ref["entropy"], one["entropy"], rtol=0, atol=2 * ref["K"])
        assert np.all(ref["variation_ratio"] == 0)
        assert np.array_equal(ref["pred"], one["pred"])


def test_two_one_hot_samples_on_different_classes():
    C = 5
    l = np.full((2, 1, C), -np.inf, np.float32)
    l[0, 0, 3] = 0
    l[1, 0, 1] = 0
    ref = R.statistics(l)
    assert abs(ref["entropy"][0] - np.log(2)) < 1e-15
    assert ref["expected_entropy"][0] == 0
    assert abs(ref["mutual_information"][0] - np.log(2)) < 1e-15
    assert ref["variation_ratio"][0] == 0.5
    assert ref["pred"][0] == 1                                 # the lower class of the two
    assert ref["confidence"][0] == 0.5
    assert np.array_equal(ref["votes"][0], [0, 1, 0, 1, 0])
    assert not ref["ambiguous_rows"][0]                        # sums of zeros and ones are exact: a tie, not an ambiguity


def test_one_class_gives_zeros():
    ref = R.statistics(np.zeros((3, 4, 1), np.float32))
    for k in ("entropy", "expected_entropy", "mutual_information", "variation_ratio"):
        assert np.all(ref[k] == 0), k
    assert np.all(ref["pred"] == 0) and np.all(ref["confidence"] == 1) and np.all(ref["votes"] == 3)


def test_minus_infinity_contributes_zero_not_nan():
    l = np.array([[[np.log(0.5), np.log(0.5), -np.inf]]], np.float32)
    ref = R.statistics(l)
    for k in ("mean_prob", "entropy", "expected_entropy", "mutual_information", "confidence"):
        assert np.all(np.isfinite(ref[k])), k
    assert abs(ref["entropy"][0] - np.log(2)) < 1e-7 and abs(ref["expected_entropy"][0] - np.log(2)) < 1e-7
    big = np.array([[[0.0, -1e4]]], np.float32)               # exp(-1e4) is 0 in float64 too: the column weighs nothing
    ref = R.statistics(big)
    assert ref["entropy"][0] == 0 and ref["expected_entropy"][0] == 0


def test_rows_outside_the_table_and_repeats():
    l = R.kernel_samples(5, 4, 2)
    ref = R.statistics(l, rows=[3, 3, -1, 7, 0])
    assert np.array_equal(ref["acc"][0], ref["acc"][1])        # a row listed twice: two independent, equal accumulators
    assert np.all(ref["acc"][2:4] == 0) and np.all(ref["votes"][2:4] == 0)


def test_forward_reduces_to_the_plain_forward_at_p_zero():
    name = "planted-dense"
    ds, (w1, w2) = R.model_dataset(name), R.model_weights(name)
    adj = R.adjacency(ds)
    z = R.sample_logits(ds, w1, w2, 0.0, 5, 0, adj)
    x = np.asarray(ds["f_val"], np.float64).reshape(ds["num_nodes"], ds["input_dim"])
    want = R.aggregate(adj, np.maximum(R.aggregate(adj, x @ w1), 0) @ w2)
    assert np.array_equal(z, want)
    assert np.array_equal(z, R.sample_logits(ds, w1, w2, 0.0, 99, 7, adj))     # no rate: neither seed nor sample matters


# ---- conditions on the GPU tests' inputs ---------------------------------------------------------------------------------

KERNEL_CASES = [(C, n_table, S) for C in (1, 2, 7, 41, 64) for n_table in (0, 1, 5, 257) for S in (1, 2, 5)]


def test_kernel_inputs_are_decided():
    """ambiguous rows are at most 1 % of the listed rows for every kernel case (the planted exact ties are not ambiguous: equal
    columns give equal sums, and the lowest class wins on both sides)"""
    for C, n_table, S in KERNEL_CASES:
        l = R.kernel_samples(n_table, C, S)
        for rows in R.row_lists(n_table):
            ref = R.statistics(l, rows)
            n = max(ref["pred"].size, 1)
            assert ref["ambiguous_rows"].sum() <= 0.01 * n, (C, n_table, S)
            assert not ref["ambiguous_samples"].any()
            if n_table > 0 and C > 1 and rows is None:
                assert np.all(ref["votes"][0, 0] == S)         # the planted tie votes for class 0


@pytest.mark.parametrize("name", sorted({name for name, _ in R.MODEL_CASES}))
def test_model_inputs_are_decided_and_powerful(name):
    """for the model cases: samples whose two largest logits lie within the logit tolerance, and rows whose two largest mean
    probabilities do, are at most 1 % of the rows; and the comparison has power — computing sample s with the masks of s + 1,
    or with the two keys swapped, moves l_s by more than 100 x the tolerance on at least 90 % of the rows"""
    ds, (w1, w2) = R.model_dataset(name), R.model_weights(name)
    adj = R.adjacency(ds)
    N = ds["num_nodes"]
    for elems in (N * R.model_hidden(name), np.asarray(ds["f_val"]).size):       # several Philox blocks and a partial one
        assert elems > 4 * 128 and elems % 128
    for p in R.MODEL_RATES:
        rate = R.MODEL_DROPOUT if p is None else p
        z, l = R.samples(ds, w1, w2, rate, R.MODEL_SEED ^ R.KEY_MC_DROPOUT, 0, 3)
        tol = R.logit_tol(z)
        ref = R.statistics(l.astype(np.float32), tol=2 * tol)
        assert ref["ambiguous_samples"].sum() <= 0.01 * N, (p, int(ref["ambiguous_samples"].sum()))
        assert ref["ambiguous_rows"].sum() <= 0.01 * N, (p, int(ref["ambiguous_rows"].sum()))
        for s in range(2):
            moved = np.abs(l[s] - l[s + 1]).max(axis=1) > 100 * tol
            assert moved.mean() >= 0.9, (p, s, moved.mean())
        swapped = R.log_softmax(R.sample_logits(ds, w1, w2, rate, R.MODEL_SEED ^ R.KEY_MC_DROPOUT, 0, adj, swap_keys=True))
        moved = np.abs(l[0] - swapped).max(axis=1) > 100 * tol
        assert moved.mean() >= 0.9, (p, "keys", moved.mean())


# ---- the interface, without a device -------------------------------------------------------------------------------------

def test_symbols_are_exported():
    from cuda_gcn_amd import _lib
    hip, host = _lib.gcnhip(), _lib.gcnhost()
    for n in ("gcnhip_mc_accumulate_rows", "gcnhip_mc_finalize_rows"):
        assert n in _lib.GCNHIP_SYMBOLS and getattr(hip, n)
    assert "gcnhost_model_mc_dropout" in _lib.GCNHOST_SYMBOLS and host.gcnhost_model_mc_dropout


class _Params:
    output_dim, hidden_dim = 7, 16


def _shell(multilabel=False, classes=7, hidden=16):
    """a HipGCNModel without a device: only what the argument checks read"""
    from cuda_gcn_amd.model import HipGCNModel
    m = object.__new__(HipGCNModel)
    m.multilabel = multilabel
    m.params = _Params()
    m.params.output_dim, m.params.hidden_dim = classes, hidden
    m.h = None
    return m


@pytest.mark.parametrize("kw,match", [
    (dict(samples=0), "samples must be an integer in 1..1024"),
    (dict(samples=1025), "samples must be an integer in 1..1024"),
    (dict(samples=2.5), "samples must be an integer"),
    (dict(p=1.0), r"p must be in \[0, 1\)"),
    (dict(p=-0.1), r"p must be in \[0, 1\)"),
    (dict(p=float("nan")), r"p must be in \[0, 1\)"),
    (dict(first_sample=2 ** 32 - 3, samples=4), "first_sample"),
    (dict(first_sample=-1), "first_sample"),
    (dict(split=4), "split is 1"),
    (dict(split=0), "split is 1"),
    (dict(split=3, nodes=[1]), "not both"),
    (dict(seed=-1), "seed"),
    (dict(seed=2 ** 64), "seed"),
])
def test_python_refusals_need_no_gpu(kw, match):
    from cuda_gcn_amd.model import GcnHostError
    with pytest.raises(GcnHostError, match=match):
        _shell().mc_dropout(**kw)


def test_python_refuses_models_the_query_does_not_take():
    from cuda_gcn_amd.model import GcnHostError
    with pytest.raises(GcnHostError, match="multi-label"):
        _shell(multilabel=True).mc_dropout()
    with pytest.raises(GcnHostError, match="at most 64 classes"):
        _shell(classes=65).mc_dropout()
    with pytest.raises(GcnHostError, match="hidden width"):
        _shell(hidden=257).mc_dropout()
