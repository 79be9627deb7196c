"""The float64 reference of the explanation kernels and its acceptance rule, without a GPU: the three splits add up to the
logit, a float32 evaluation of the same definition is accepted, and wrong answers are not."""
import numpy as np
import pytest

from tests import explain_ref as R


def small_net(seed, n=60, h=12, F=9, C=4):
    """a random graph with self loops, one-way and repeated edges, symmetric-normalised coefficients, and a consistent two-layer
    net: H1 = f32(ReLU(S W1))"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        k = int(rng.integers(0, 9))
        nb = rng.integers(0, n, k)
        if k > 2 and i % 5 == 0:
            nb[1] = nb[0]                                         # a repeated edge
        rows.append(np.concatenate([[i], nb]))
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum([r.size for r in rows])
    indices = np.concatenate(rows).astype(np.int64)
    deg = np.diff(indptr).astype(np.float64)
    src = np.repeat(np.arange(n), np.diff(indptr))
    coef = (1.0 / np.sqrt(deg[src] * deg[indices])).astype(np.float32)
    x = rng.standard_normal((n, F)).astype(np.float32) * (rng.random((n, F)) < 0.6)
    w1 = (rng.standard_normal((F, h)) * 0.5).astype(np.float32)
    w2 = (rng.standard_normal((h, C)) * 0.5).astype(np.float32)
    s, s_abs, terms = R.layer1(indptr, indices, coef, x)
    h1 = np.maximum(s.astype(np.float32) @ w1, 0).astype(np.float32)
    return dict(indptr=indptr, indices=indices, coef=coef, x=x, w1=w1, w2=w2, s=s, s_abs=s_abs, terms=terms, h1=h1, n=n, C=C)


def ref_of(net, v, c, **kw):
    return R.explain64(net["indptr"], net["indices"], net["coef"], net["h1"], net["w2"], v, c, w1=net["w1"], s=net["s"], s_abs=net["s_abs"],
                       terms=net["terms"], **kw)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_three_splits_sum_to_the_float64_logit(seed):
    net = small_net(seed)
    z = R.layer1(net["indptr"], net["indices"], net["coef"], net["h1"].astype(np.float64) @ net["w2"].astype(np.float64))[0]
    for v in range(net["n"]):
        for c in (0, net["C"] - 1):
            ref = ref_of(net, v, c)
            scale = ref["E_logit"] / R.U + 1e-300
            assert abs(ref["nbr"].sum() - ref["logit"]) <= 1e-12 * scale
            assert abs(ref["hid"].sum() - ref["logit"]) <= 1e-12 * scale
            assert abs(ref["logit"] - z[v, c]) <= 1e-12 * scale                  # the forward's own logit
            assert abs(ref["feat"].sum() - ref["logit"]) <= ref["layer1_gap"] + 1e-12 * scale
            assert ref["rows"].size == net["indptr"][v + 1] - net["indptr"][v]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_a_float32_evaluation_is_accepted(seed):
    net = small_net(seed)
    for v in range(net["n"]):
        c = v % net["C"]
        ref = ref_of(net, v, c)
        got = R.explain_f32(net["indptr"], net["indices"], net["coef"], net["h1"], net["w2"], v, c, w1=net["w1"], s=net["s"])
        assert R.violations(got, ref) == [], (v, c)
        assert R.sum_violations(got, ref) == [], (v, c)


def test_wrong_answers_are_rejected():
    net = small_net(4)
    rng = np.random.default_rng(0)
    other_h1 = np.maximum(net["h1"] + rng.standard_normal(net["h1"].shape).astype(np.float32), 0)
    seen = dict(off=0, dropped=0, swapped=0, gate=0)
    for v in range(net["n"]):
        c = v % net["C"]
        ref = ref_of(net, v, c)
        good = {k: (None if ref[k] is None else np.array(ref[k], copy=True)) for k in ("rows", "logit", "nbr", "hid", "feat")}
        assert R.violations(good, ref) == []
        # a share off by 3 E
        for name, err in (("nbr", "E_nbr"), ("hid", "E_hid"), ("feat", "E_feat")):
            j = int(np.argmax(ref[err]))
            if ref[err][j] > 0:
                bad = dict(good); bad[name] = good[name].copy(); bad[name][j] += 3 * ref[err][j]
                assert R.violations(bad, ref) != [], (v, name)
                seen["off"] += 1
        if ref["E_logit"] > 0:
            bad = dict(good); bad["logit"] = ref["logit"] - 3 * ref["E_logit"]
            assert R.violations(bad, ref) != []
        # a dropped neighbour
        if ref["rows"].size > 1:
            bad = dict(good); bad["rows"], bad["nbr"] = good["rows"][:-1], good["nbr"][:-1]
            assert R.violations(bad, ref) != []
            seen["dropped"] += 1
        # the answer of another class
        wrong = ref_of(net, v, (c + 1) % net["C"])
        if abs(wrong["logit"] - ref["logit"]) > ref["E_logit"]:
            assert R.violations({k: wrong[k] for k in good}, ref) != []
            seen["swapped"] += 1
        # gates taken from another H1
        gated = ref_of(net, v, c, gate_from=other_h1)
        if np.any(np.abs(gated["feat"] - ref["feat"]) > ref["E_feat"]):
            bad = dict(good); bad["feat"] = gated["feat"]
            assert R.violations(bad, ref) != []
            seen["gate"] += 1
    assert all(n >= net["n"] // 2 for n in seen.values()), seen


def test_open_queries_and_the_expected_column():
    """top_feature_agreement: a query whose two top shares lie within 2 (E_a + E_b) is open and is not held against the answer"""
    ref = dict(feat=np.array([1.0, 1.0 - 1e-9, 0.2]), E_feat=np.array([1e-8, 1e-8, 1e-8]))
    clear = dict(feat=np.array([0.1, 1.0, 0.2]), E_feat=np.array([1e-8, 1e-8, 1e-8]))
    hit, opened, agree = R.top_feature_agreement(np.array([[0.9, 1.0, 0.0], [0.0, 1.0, 0.5]]), [ref, clear], [0, 1])
    assert (hit, opened, agree) == (1.0, 0.5, True)
    assert R.top_feature_agreement(np.array([[0.9, 1.0, 0.0], [0.0, 0.4, 0.5]]), [ref, clear], [0, 1])[2] is False


def test_the_recorded_planted_figures_are_reproduced(oracle):
    """REF_TOP_FEATURE / REF_OPEN of the GPU test are what tests/validation/explain_planted_cpu.py measures: the
    CPU oracle's weights, the float64 reference, no GPU"""
    from tests.validation.explain_planted_cpu import measure
    from tests.test_explain_model_gpu import REF_OPEN, REF_TOP_FEATURE
    got = measure(oracle)
    assert got["test_nodes"] == 193
    assert round(got["top_feature"], 4) == REF_TOP_FEATURE and got["open"] == REF_OPEN
    assert 0.5 < got["informative_mass"] < 0.56
