"""The multi-label truth file without a GPU (host/labels.{h,cpp}, model.read_labels, gcnhost_labels_read): round trips,
a hand-written file, refusals with a message, and gcn-hip refusing a bad GCN_MULTILABEL file before it touches the GPU."""
import os
import subprocess

import numpy as np
import pytest

from cuda_gcn_amd import datagen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")


def test_round_trip(tmp_path):
    from cuda_gcn_amd.model import read_labels, write_labels
    rng = np.random.default_rng(0)
    for C in (1, 31, 32, 33, 121, 256):
        y = rng.random((57, C)) < 0.2
        y[:, C - 1] |= rng.random(57) < 0.5          # the last class occurs: C = largest id + 1
        y[3] = False                                  # a node with no class (empty line)
        p = str(tmp_path / f"l{C}.txt")
        write_labels(p, y)
        got = read_labels(p)
        assert got.shape == y.shape and got.dtype == bool and np.array_equal(got, y)
        assert np.array_equal(read_labels(p, num_nodes=57, num_classes=C + 5)[:, :C], y)


def test_hand_written_file(tmp_path):
    from cuda_gcn_amd.model import read_labels
    p = tmp_path / "l.txt"
    p.write_text("0,2\n\n5\n 1 , 3 ,1\r\n2")          # an empty line, spaces, a repeat, CRLF, no final newline
    y = read_labels(str(p))
    want = np.zeros((5, 6), bool)
    want[0, [0, 2]] = want[2, 5] = want[3, [1, 3]] = want[4, 2] = True
    assert np.array_equal(y, want)
    assert read_labels(str(p), num_nodes=5, num_classes=8).shape == (5, 8)
    p.write_text("\n\n")                              # two nodes, no class at all: C = 1
    assert read_labels(str(p)).shape == (2, 1) and not read_labels(str(p)).any()


@pytest.mark.parametrize("text,kw,msg", [
    ("1\n2\n3\n", dict(num_nodes=4), "3 lines, but the dataset has 4 nodes"),
    ("1\n2\n3\n4\n5\n", dict(num_nodes=4), "5 lines"),
    ("1\n2,x\n", {}, ":2: bad token 'x'"),
    ("1\n2,,3\n", {}, ":2: bad token ''"),
    ("1.5\n", {}, ":1: bad token '1.5'"),
    ("0\n3,-2\n", {}, ":2: negative class id '-2'"),
    ("0\n7\n", dict(num_classes=5), ":2: class id 7 is not below the number of classes 5"),
    ("99999999999\n", {}, "too large"),
])
def test_refusals(tmp_path, text, kw, msg):
    from cuda_gcn_amd.model import GcnHostError, read_labels
    p = tmp_path / "bad.txt"
    p.write_text(text)
    with pytest.raises(GcnHostError, match=None) as e:
        read_labels(str(p), **kw)
    assert msg in str(e.value), str(e.value)


def test_missing_file(tmp_path):
    from cuda_gcn_amd.model import GcnHostError, read_labels
    with pytest.raises(GcnHostError, match="cannot open"):
        read_labels(str(tmp_path / "none.txt"))


def test_generator_is_deterministic_and_multilabel():
    a = datagen.planted_multilabel(n_comm=8, size=64, classes=121)
    b = datagen.planted_multilabel(n_comm=8, size=64, classes=121)
    y = a["multilabel"]
    assert y.shape == (512, 121) and y.dtype == bool and a["output_dim"] == 121
    assert np.array_equal(y, b["multilabel"])
    assert y.sum(1).mean() > 2.5                      # several classes per node
    assert 0 < y.mean() < 0.2


@pytest.mark.parametrize("text,msg", [("0\n", "1 lines, but the dataset has"), ("0\n1,q\n", "bad token 'q'")])
def test_cli_refuses_a_bad_label_file_before_the_gpu(tmp_path, text, msg):
    """the label file is read and checked right after the dataset, before any GPU call: on a machine with or without a GPU
    the run ends with the file's message and no RUNNING ON GPU line"""
    ds = datagen.make_dataset("tiny-syn")
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "tiny.gcnbin"))
    p = tmp_path / "labels.txt"
    p.write_text(text)
    r = subprocess.run(["timeout", "-k", "10", "60", HIP, "tiny"], cwd=str(tmp_path), env=dict(os.environ, GCN_MULTILABEL=str(p)),
                       capture_output=True, text=True)
    assert r.returncode != 0
    assert "GCN_MULTILABEL" in r.stderr and msg in r.stderr, r.stderr
    assert "RUNNING ON GPU" not in r.stdout and "no GPU" not in r.stderr
