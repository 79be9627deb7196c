"""gcn-hip with GCN_THRESHOLDS / GCN_APPLY_THRESHOLDS on saved weights of a planted multi-label model: the file it writes reads
back as HipGCNModel.tune_thresholds' cuts, the printed F1s are evaluate()'s, GCN_PREDICT and GCN_REPORT decide by the cuts, a
run that applies the file reproduces the tuned numbers and files, the refusals exit non-zero before training, and without the
variables stdout has no line more."""
import os
import re
import subprocess

import numpy as np
import pytest

from cuda_gcn_amd import datagen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "cuda_gcn_amd", "bin", "gcn-hip")
FIT_LINE = re.compile(r"thresholds_beta=(\S+) val_macro_f1_default=(\S+) val_macro_f1_tuned=(\S+) test_micro_f1_default=(\S+) test_micro_f1_tuned=(\S+) "
                      r"test_macro_f1_default=(\S+) test_macro_f1_tuned=(\S+)")
NOTE = re.compile(r"(\S+) # class (\d+) pos (\d+) neg (\d+) tp (\d+) fp (\d+) fn (\d+) f (\S+)")


def timeless(stdout):
    return re.sub(r"time=\S+", "time=*", stdout)


def read_sets(path, n, c):
    sets = np.zeros((n, c), bool)
    lines = open(path).read().splitlines()
    assert len(lines) == n
    for i, line in enumerate(lines):
        parts = line.split(" ")
        assert int(parts[0]) == i and len(parts) <= 2
        if len(parts) == 2:
            sets[i, [int(k) for k in parts[1].split(",")]] = True
    return sets


def test_cli_thresholds(tmp_path):
    from cuda_gcn_amd.model import HipGCNModel, read_thresholds, write_labels
    ds = datagen.planted_multilabel(classes=41)
    n, c = ds["num_nodes"], 41
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "planted.gcnbin"))
    lab, w = str(tmp_path / "labels.txt"), str(tmp_path / "w.gcnw")
    write_labels(lab, ds["multilabel"])
    m = HipGCNModel(ds, seed=3, hidden_dim=32, dropout=0.5, learning_rate=0.05, multilabel=ds["multilabel"])
    for _ in range(15):
        m.train_epoch()
    m.save_weights(w)
    fit, fit_half = m.tune_thresholds(), m.tune_thresholds(beta=0.5)
    val = m.evaluate(split=2), m.evaluate(split=2, thresholds=fit)
    test = m.evaluate(split=3), m.evaluate(split=3, thresholds=fit)
    ids, _ = m.row_ids()
    tuned_sets = m.predict_multilabel(thresholds=fit)[np.argsort(ids)]
    default_sets = m.predict_multilabel()[np.argsort(ids)]
    m.close()
    assert not np.array_equal(tuned_sets, default_sets)

    args = ["planted", "-", "-", "32", "-", "0.5", "-", "-", "0"]
    base = dict(os.environ, GCN_SEED="3", GCN_LOAD_WEIGHTS=w, GCN_MULTILABEL=lab)
    path = lambda name: str(tmp_path / name)

    def run(**env):
        return subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=dict(base, **env), capture_output=True, text=True)

    plain = run(GCN_REPORT=path("report_a.txt"), GCN_PREDICT=path("pred_a.txt"))
    assert plain.returncode == 0, plain.stderr[-2000:]
    assert "thresholds" not in plain.stdout and np.array_equal(read_sets(path("pred_a.txt"), n, c), default_sets)
    r = run(GCN_REPORT=path("report_b.txt"), GCN_PREDICT=path("pred_b.txt"), GCN_THRESHOLDS=path("thr.txt"))
    assert r.returncode == 0, r.stderr[-2000:]
    out, before = r.stdout.splitlines(), plain.stdout.splitlines()
    assert len(out) == len(before) + 1 and timeless("\n".join(out[:-1])) == timeless("\n".join(before))
    assert "decision thresholds of 41 classes" in r.stderr
    g = FIT_LINE.fullmatch(out[-1])
    assert g, out[-1]
    want = (1.0, val[0]["macro_f1"], val[1]["macro_f1"], test[0]["micro_f1"], test[1]["micro_f1"], test[0]["macro_f1"], test[1]["macro_f1"])
    for text, value in zip(g.groups(), want):
        assert abs(float(text) - value) <= 5.1e-6, (out[-1], want)                # five decimals
    assert float(g.group(3)) >= float(g.group(2))
    # the file: the fit's cuts bit for bit, its counts in the comments
    thr = read_thresholds(path("thr.txt"), num_classes=c)
    assert thr.tobytes() == fit["threshold"].tobytes()
    lines = open(path("thr.txt")).read().splitlines()
    assert len(lines) == c
    for j, line in enumerate(lines):
        q = NOTE.fullmatch(line)
        assert q, line
        assert np.float32(q.group(1)) == fit["threshold"][j]
        assert [int(x) for x in q.groups()[1:7]] == [j] + [int(fit[k][j]) for k in ("pos", "neg", "tp", "fp", "fn")]
        assert abs(float(q.group(8)) - fit["f"][j]) <= 5.1e-10
    # GCN_PREDICT and GCN_REPORT decide by the cuts
    assert np.array_equal(read_sets(path("pred_b.txt"), n, c), tuned_sets)
    rep = open(path("report_b.txt")).read().splitlines()
    total = [l for l in rep if l.startswith("macro_f1 ")]
    assert len(total) == 1 and abs(float(total[0].split()[1]) - test[1]["macro_f1"]) <= 5.1e-6 and abs(float(total[0].split()[3]) - test[1]["micro_f1"]) <= 5.1e-6
    assert open(path("report_a.txt"), "rb").read() != open(path("report_b.txt"), "rb").read()
    # another beta
    h = run(GCN_THRESHOLDS=path("thr_half.txt"), GCN_THRESHOLDS_BETA="0.5")
    assert h.returncode == 0, h.stderr[-2000:]
    assert h.stdout.splitlines()[-1].startswith("thresholds_beta=0.5 ")
    assert read_thresholds(path("thr_half.txt")).tobytes() == fit_half["threshold"].tobytes()
    # applying the file reproduces the tuned numbers and files
    a = run(GCN_REPORT=path("report_c.txt"), GCN_PREDICT=path("pred_c.txt"), GCN_APPLY_THRESHOLDS=path("thr.txt"))
    assert a.returncode == 0, a.stderr[-2000:]
    aout = a.stdout.splitlines()
    assert len(aout) == len(before) + 1 and aout[-1] == out[-1][out[-1].index("test_micro_f1_default="):]
    assert open(path("report_c.txt"), "rb").read() == open(path("report_b.txt"), "rb").read()
    assert open(path("pred_c.txt"), "rb").read() == open(path("pred_b.txt"), "rb").read()
    # refused before training
    with open(path("short.txt"), "w") as f:
        f.write("0.5\n0.25\n")
    single = {k: v for k, v in base.items() if k != "GCN_MULTILABEL"}
    for env, msg in ((dict(GCN_THRESHOLDS=path("x.txt"), GCN_GPUS="2"), "run on one GPU"),
                     (dict(GCN_APPLY_THRESHOLDS=path("thr.txt"), GCN_GPUS="2"), "run on one GPU"),
                     (dict(GCN_THRESHOLDS=path("x.txt"), GCN_APPLY_THRESHOLDS=path("thr.txt")), "exclude each other"),
                     (dict(GCN_THRESHOLDS=path("x.txt"), GCN_THRESHOLDS_BETA="0"), "GCN_THRESHOLDS_BETA finite and > 0"),
                     (dict(GCN_THRESHOLDS=path("x.txt"), GCN_THRESHOLDS_BETA="nan"), "GCN_THRESHOLDS_BETA finite and > 0"),
                     (dict(GCN_APPLY_THRESHOLDS=path("short.txt")), "2 thresholds for 41 classes"),
                     (dict(GCN_APPLY_THRESHOLDS=path("missing.txt")), "cannot open the thresholds file")):
        bad = run(**env)
        assert bad.returncode != 0 and msg in bad.stderr and "epoch=" not in bad.stdout and "test_loss" not in bad.stdout, (env, bad.stderr[-500:])
        assert not os.path.exists(path("x.txt"))
    for env in (dict(GCN_THRESHOLDS=path("x.txt")), dict(GCN_APPLY_THRESHOLDS=path("thr.txt"))):
        bad = subprocess.run(["timeout", "-k", "10", "50", HIP] + args, cwd=str(tmp_path), env=dict(single, **env), capture_output=True, text=True)
        assert bad.returncode != 0 and "need GCN_MULTILABEL" in bad.stderr and "test_" not in bad.stdout, bad.stderr[-500:]
