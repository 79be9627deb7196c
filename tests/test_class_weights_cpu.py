"""Class weights without a GPU: the `balanced` rules against a direct numpy restatement, the weights file reader and its
refusals, the option checks of the model constructor that need no device, and gcn-hip refusing a bad GCN_CLASS_WEIGHTS before
the GPU is touched."""
import os
import subprocess

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from cuda_gcn_amd import model as M
from tests.class_weights_ref import balanced_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")


@pytest.mark.parametrize("C", [1, 7, 41, 256])
def test_balanced_single_label_against_numpy(C):
    rng = np.random.default_rng(C)
    n = 3000
    label = rng.integers(0, C, n).astype(np.int32)
    if C > 2:
        label[label == C - 2] = 0                  # an empty class
    label[rng.random(n) < 0.1] = -1                # unlabelled rows
    split = rng.integers(0, 4, n).astype(np.int32)
    for s in (1, 2):
        got = M.balanced_class_weights(label, split, C, which_split=s)
        want = balanced_reference(label, split, C, s)
        assert got.dtype == np.float32 and got.shape == (C,)
        assert np.allclose(got, want, rtol=1e-6, atol=0)
        if C > 2:
            assert got[C - 2] == 0.0
    # scikit-learn's identity: the weighted class counts are all n / C
    lab = label[(split == 1) & (label >= 0)]
    cnt = np.bincount(lab, minlength=C)
    w = M.balanced_class_weights(label, split, C)
    assert np.allclose((w * cnt)[cnt > 0], lab.size / C, rtol=1e-5)


@pytest.mark.parametrize("C", [1, 41, 121])
def test_balanced_multilabel_against_numpy(C):
    rng = np.random.default_rng(C + 1)
    n = 2000
    y = rng.random((n, C)) < rng.random(C) * 0.3
    if C > 1:
        y[:, 1] = False                            # a class without positives: weight 1
    split = rng.integers(0, 4, n).astype(np.int32)
    got = M.balanced_class_weights(y, split, C)
    assert np.allclose(got, balanced_reference(y, split, C), rtol=1e-6, atol=0)
    if C > 1:
        assert got[1] == 1.0
    with pytest.raises(ValueError):
        M.balanced_class_weights(y[:, :-1] if C > 1 else y[:-1], split, C)


def test_weights_file_round_trip(tmp_path):
    w = np.array([0.5, 1, 2.25, 0, 1e-3, 10], np.float32)
    p = tmp_path / "w.txt"
    p.write_text("".join(f"{x!r}\n" for x in w.tolist()))
    assert np.array_equal(M.read_class_weights(str(p)), w)
    assert np.array_equal(M.read_class_weights(str(p), num_classes=6), w)
    p.write_text(" 1.5 \n2\n3e0")                    # spaces around a value, no final newline
    assert np.array_equal(M.read_class_weights(str(p), 3), np.array([1.5, 2, 3], np.float32))


@pytest.mark.parametrize("text,kw,msg", [
    ("1\n2\n3\n", dict(num_classes=4), "3 lines for 4 classes"),
    ("1\n2\n3\n4\n5\n", dict(num_classes=4), "5 lines for 4 classes"),
    ("1\nabc\n3\n", {}, "line 2"),
    ("1\n2 3\n", {}, "line 2"),
    ("1\n2\n-0.5\n", {}, "line 3"),
    ("nan\n2\n", {}, "line 1"),
    ("1\ninf\n", {}, "line 2"),
    ("1\n\n3\n", {}, "line 2"),
    ("", {}, "no weights"),
])
def test_weights_file_refusals(tmp_path, text, kw, msg):
    p = tmp_path / "w.txt"
    p.write_text(text)
    with pytest.raises(M.GcnHostError, match=msg):
        M.read_class_weights(str(p), **kw)


def test_missing_weights_file(tmp_path):
    with pytest.raises(M.GcnHostError, match="cannot open"):
        M.read_class_weights(str(tmp_path / "none.txt"))


def test_constructor_refuses_bad_weights_before_the_gpu():
    """length and spelling are checked in Python; sign, NaN, infinity and an all-zero split by HipGCN before it creates a context"""
    ds = datagen.make_dataset("cora-syn")
    C = ds["output_dim"]
    with pytest.raises(ValueError, match="weights for"):
        M.HipGCNModel(ds, class_weights=np.ones(C + 1))
    with pytest.raises(ValueError, match="balanced"):
        M.HipGCNModel(ds, class_weights="balance")
    for bad, msg in ((-1.0, "finite and not negative"), (np.nan, "finite and not negative"), (np.inf, "finite and not negative")):
        w = np.ones(C, np.float32)
        w[2] = bad
        with pytest.raises(M.GcnHostError, match=msg):
            M.HipGCNModel(ds, class_weights=w)
    with pytest.raises(M.GcnHostError, match="sum to 0"):
        M.HipGCNModel(ds, class_weights=np.zeros(C, np.float32))
    wide = dict(ds, output_dim=300)
    with pytest.raises(M.GcnHostError, match="256"):
        M.HipGCNModel(wide, class_weights=np.ones(300, np.float32))


@pytest.mark.parametrize("text,msg", [("1\n2\n", "lines for"), ("1\n1\n1\nx\n1\n1\n1\n", "line 4"), ("1\n1\n-1\n1\n1\n1\n1\n", "line 3")])
def test_cli_refuses_a_bad_weights_file_before_the_gpu(tmp_path, text, msg):
    ds = datagen.make_dataset("cora-syn")
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "cora-syn.gcnbin"))
    f = tmp_path / "w.txt"
    f.write_text(text)
    r = subprocess.run([HIP, "cora-syn"], cwd=str(tmp_path), env=dict(os.environ, GCN_CLASS_WEIGHTS=str(f)), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0
    assert "GCN_CLASS_WEIGHTS" in r.stderr and msg in r.stderr, r.stderr
    assert "RUNNING ON GPU" not in r.stdout


def test_entry_points_are_exported_and_declared():
    from cuda_gcn_amd import _lib
    for n in ("gcnhip_wxent_fwd_rows", "gcnhip_wbce_fwd_rows"):
        assert n in _lib.GCNHIP_SYMBOLS and hasattr(_lib.gcnhip(), n)
    for n in ("gcnhost_model_create_weighted", "gcnhost_balanced_class_weights", "gcnhost_class_weights_read"):
        assert n in _lib.GCNHOST_SYMBOLS and hasattr(_lib.gcnhost(), n)
