"""What the kernel two-sample test needs without a GPU: the statistics against their formulas, the argument checks, the C symbols."""
import ctypes

import numpy as np
import pytest

from cuda_gcn_amd import _lib
from cuda_gcn_amd import model as M
from tests import mmd_ref as R


@pytest.mark.parametrize("m,rest", [(1, 1), (1, 5), (7, 1), (40, 60)])
def test_mmd_stats_are_the_formulas(m, rest):
    """on the float64 sums of a small sample; a group of one row has no pair of distinct rows: its unbiased term is NaN"""
    rng = np.random.default_rng(m + rest)
    x = rng.standard_normal((m + rest, 3)).astype(np.float32)
    sums = np.delete(R.sums64(x, np.ones(m + rest, bool), R.membership(m + rest, m, 30, rng), 0.5)["sums"], 0, 1)
    got, (biased, unbiased, p) = M.mmd_stats(sums, m, rest), R.stats64(sums, m, rest)
    assert np.allclose(got["biased"], biased, rtol=1e-13, atol=0) and got["p_value"] == p and 1 / 31 <= p <= 1
    assert np.all(np.isnan(got["unbiased"])) if min(m, rest) == 1 else np.allclose(got["unbiased"], unbiased, rtol=1e-12, atol=1e-16)
    assert M.mmd_stats(sums[:, :1], m, rest)["p_value"] == 1.0


def test_mmd_stats_refusals():
    for args in ((np.zeros((3, 0)), 2, 2), (np.zeros((2, 4)), 2, 2), (np.zeros((3, 4)), 0, 2), (np.zeros((3, 4)), 2, 0)):
        with pytest.raises(M.GcnHostError):
            M.mmd_stats(*args)


@pytest.mark.parametrize("kw", [dict(gamma=0.0), dict(gamma=-1.0), dict(gamma=np.inf), dict(gamma=np.nan), dict(gamma="x"), dict(gamma=[1, 2, 3, 4, 5]),
                                dict(gamma=[]), dict(gamma=[1.0, 0.0]), dict(permutations=-1), dict(permutations=2.5), dict(permutations=None),
                                dict(seed=-1), dict(seed=1.5), dict(a=np.arange(0)), dict(b=np.arange(0)), dict(b=np.array([9, 2]))])
def test_mmd_argument_checks(kw):
    """the checks of HipGCNModel.mmd that need no model: gamma, permutations, the seed, an empty group, overlapping groups"""
    args = dict(dict(gamma=None, permutations=10, seed=None, a=np.arange(3), b=np.arange(5, 9)), **kw)
    with pytest.raises(M.GcnHostError):
        M.HipGCNModel._mmd_args(None, "mmd", **args)
    g, perms = M.HipGCNModel._mmd_args(None, "mmd", [0.5, 2], 0, 7, np.arange(3), np.arange(5, 9))
    assert g.tolist() == [0.5, 2.0] and perms == 0


def test_c_symbols_are_present():
    hip, host = _lib.gcnhip(), _lib.gcnhost()
    for name in ("gcnhip_mmd_plan", "gcnhip_mmd_walk", "gcnhip_mmd_fold"):
        assert hasattr(hip, name) and name in _lib.GCNHIP_SYMBOLS, name
    for name in ("gcnhost_model_mmd", "gcnhost_mmd_stats"):
        assert hasattr(host, name) and name in _lib.GCNHOST_SYMBOLS, name
    a, b = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.gcnhip_mmd_plan(2100, 130, 48, 1, ctypes.byref(a), ctypes.byref(b)) == 0                        # no GPU needed
    fixed = 1280 + 2112 * 16 + 2112 * 144 * 4 + 2112 * 4 + 256 * 2 + (33 * 48 * 8 + 255) // 256 * 256          # 33 tiles, ldx 144
    part = (33 * 3 * 48 * 8 + 255) // 256 * 256 + 2112 * 16
    assert (a.value, b.value) == (fixed + 3 * part, fixed + part)
    for bad in ((10, 257, 16), (10, 16, 24), (10, 16, 272), (-1, 16, 16)):
        assert hip.gcnhip_mmd_plan(*bad, 0, None, None) == -1
    assert b"multiple of 16" in hip.gcnhip_last_error() or b"invalid" in hip.gcnhip_last_error()
