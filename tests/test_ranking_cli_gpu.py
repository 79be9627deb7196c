"""gcn-hip with GCN_RANKING: the file it writes parses and agrees with HipGCNModel.ranking for the same saved weights; stdout
and the GCN_REPORT file are the same bytes with and without it."""
import os
import re
import subprocess

import numpy as np
import pytest

from cuda_gcn_amd import datagen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")
CLASS = re.compile(r"class (\d+) pos (\d+) neg (\d+) auc (\S+) ap (\S+)")
TOTAL = re.compile(r"macro_auc (\S+) macro_ap (\S+) weighted_auc (\S+) weighted_ap (\S+) classes (\d+)")


def timeless(stdout):
    return re.sub(r"time=\S+", "time=*", stdout)


def test_cli_ranking(tmp_path):
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.make_dataset("cora-syn")
    # class 6 loses its test nodes to the validation split: no positive there, `undefined` in the file
    ds = dict(ds, split=np.where((ds["split"] == 3) & (ds["label"] == 6), 2, ds["split"]).astype(np.int32))
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "cora-syn.gcnbin"))
    c = ds["output_dim"]
    m = HipGCNModel(ds, seed=3, hidden_dim=16, dropout=0.5)
    m.run_epochs(6, want_trace=False)
    w = str(tmp_path / "w.gcnw")
    m.save_weights(w)
    want = m.ranking(split=3)
    m.close()
    assert not want["ap_defined"][6] and want["classes_defined"] == c - 1
    args = ["cora-syn", "-", "-", "16", "-", "0.5", "-", "-", "0"]
    rep_a, rep_b, out = str(tmp_path / "report_a.txt"), str(tmp_path / "report_b.txt"), str(tmp_path / "ranking.txt")
    base = dict(os.environ, GCN_SEED="3", GCN_LOAD_WEIGHTS=w)
    plain = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=dict(base, GCN_REPORT=rep_a), capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr[-2000:]
    r = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=dict(base, GCN_REPORT=rep_b, GCN_RANKING=out),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert timeless(r.stdout) == timeless(plain.stdout) and open(rep_a, "rb").read() == open(rep_b, "rb").read()
    assert "ranking metrics of the test split" in r.stderr
    lines = open(out).read().splitlines()
    assert len(lines) == c + 1
    for j, line in enumerate(lines[:c]):
        g = CLASS.fullmatch(line)
        assert g, line
        assert int(g.group(1)) == j and int(g.group(2)) == want["pos"][j] and int(g.group(3)) == want["neg"][j]
        for text, value, defined in ((g.group(4), want["auc"][j], want["auc_defined"][j]), (g.group(5), want["ap"][j], want["ap_defined"][j])):
            assert (text == "undefined") == (not defined), line
            assert not defined or abs(float(text) - value) <= 5.1e-10, (line, value)      # nine decimals
    g = TOTAL.fullmatch(lines[c])
    assert g, lines[c]
    for text, k in zip(g.groups()[:4], ("macro_auc", "macro_ap", "weighted_auc", "weighted_ap")):
        assert abs(float(text) - want[k]) <= 5.1e-10, (k, text, want[k])
    assert int(g.group(5)) == want["classes_defined"]
    bad = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=dict(base, GCN_RANKING=out, GCN_GPUS="2"),
                         capture_output=True, text=True)
    assert bad.returncode != 0 and "GCN_RANKING runs on one GPU" in bad.stderr, bad.stderr[-500:]
