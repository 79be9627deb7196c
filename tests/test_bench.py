"""bench.py as the driver invokes it.

CPU: `python bench.py --gpus 2` with no WORLD_SIZE must start its own ranks as child processes (never exec
from a process that touched the GPU) and hand back their failure as a non-zero exit — here the children stop at
"no GPU visible".
GPU (-m gpu): a plain 1-GPU line carries the contract fields and nothing measured after the headline; with `--full`
it carries a roofline fraction <= 1 against the bound that binds; `--gpus 2 --full` self-launches two ranks (both on
GPU 0, host-staged transport: the one-GPU box has no second device for RCCL) and prints ONE JSON line with n_gpus = 2.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def run_bench(args, env=None, timeout=900):
    e = dict(os.environ, OMP_NUM_THREADS="1", **(env or {}))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        e.pop(k, None)
    p = subprocess.run([sys.executable, BENCH] + [str(a) for a in args], env=e, capture_output=True, text=True, timeout=timeout)
    return p


def json_lines(stdout):
    return [json.loads(ln) for ln in stdout.splitlines() if ln.startswith("{")]


def test_launcher_parent_returns_child_failure_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("CPU-only check")
    p = run_bench(["--gpus", 2, "--steps", 1, "--warmup", 0, "--eval-lane", "off"], env={"GCN_BENCH_TIMEOUT": "300"})
    assert p.returncode != 0
    assert "starting 2 ranks" in p.stderr and "no GPU visible" in p.stderr, p.stderr[-2000:]
    assert json_lines(p.stdout) == []


def test_launcher_does_not_touch_gpu_before_spawning():
    """the parent path of bench.py must not import torch or load a native library before it starts the ranks"""
    src = open(BENCH).read()
    main_body = src[src.index("def main():"):]
    spawn_at = main_body.index("launch_ranks(")
    assert "import torch" not in main_body[:spawn_at]
    assert "cuda_gcn_amd" not in main_body[:spawn_at]
    head = src[:src.index("def main():")]
    top_level_imports = [ln for ln in head.splitlines() if ln.startswith("import ") or ln.startswith("from ")]
    assert not any("torch" in ln or "cuda_gcn_amd" in ln or "numpy" in ln for ln in top_level_imports), top_level_imports



# ---- the N > 1 launcher's deadline logic, without a GPU: _run_ranks replaced by a stand-in (verdict r05 item 3)
def _fake_line(value, schedule):
    return json.dumps({"metric": "epochs_per_sec", "value": value, "ms_per_step": 1e3 / value, "config": {"schedule": schedule}, "cpu_baseline": None})


def _launcher(monkeypatch, capsys, behaviour, env):
    """run bench.launch_ranks(8, ...) with _run_ranks(n, extra, timeout, env) -> behaviour(extra, timeout); returns (rc, stdout JSON lines, calls)"""
    import importlib
    import time
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    calls = []

    def fake(n_gpus, extra, timeout, env=None):
        calls.append((list(extra), timeout, dict(env or {})))
        return behaviour(extra, timeout)
    monkeypatch.setattr(bench, "_run_ranks", fake)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("HIPGCN_EXCHANGE", raising=False)
    monkeypatch.delenv("GCN_BENCH_TRANSPORT", raising=False)
    t0 = time.monotonic()
    rc = bench.launch_ranks(8, ["--gpus", "8", "--steps", "3"])
    return rc, json_lines(capsys.readouterr().out), calls, time.monotonic() - t0


def _kind(extra):
    if "--selftest" in extra:
        return "selftest"
    if "on" in extra[extra.index("--overlap") + 1]:
        return "overlap"
    return "lane" if extra[extra.index("--eval-lane") + 1] == "on" else "plain"


def test_launcher_prints_the_safe_line_first_and_the_best_line_last(monkeypatch, capsys):
    def behaviour(extra, timeout):
        k = _kind(extra)
        return {"selftest": (0, json.dumps({"selftest": "ok"})), "plain": (0, _fake_line(100.0, "plain one-stream")),
                "overlap": (0, _fake_line(120.0, "exchange overlap")), "lane": (0, _fake_line(90.0, "validation lane"))}[k]
    rc, lines, calls, _ = _launcher(monkeypatch, capsys, behaviour, {"GCN_BENCH_DEADLINE": "420"})
    assert rc == 0 and [_kind(c[0]) for c in calls] == ["selftest", "plain", "overlap", "lane"]
    assert calls[1][2]["HIPGCN_EXCHANGE"] == "auto"
    assert lines[0]["value"] == 100.0 and lines[0]["config"]["schedule"] == "plain one-stream"
    assert lines[-1]["value"] == 120.0 and {o["value"] for o in lines[-1]["other_schedules"]} == {100.0, 90.0}
    assert all(c[1] <= 420 for c in calls)


def test_launcher_keeps_the_safe_line_when_an_optional_schedule_hangs(monkeypatch, capsys):
    import time

    def behaviour(extra, timeout):
        k = _kind(extra)
        if k == "selftest":
            return 0, json.dumps({"selftest": "ok"})
        if k == "plain":
            time.sleep(0.3)
            return 0, _fake_line(100.0, "plain one-stream")
        if k == "overlap":                      # hangs: the stand-in returns what _run_ranks returns after killing the group
            time.sleep(timeout)
            return 124, None
        return 0, _fake_line(101.0, "validation lane")
    rc, lines, calls, wall = _launcher(monkeypatch, capsys, behaviour, {"GCN_BENCH_DEADLINE": "8", "GCN_BENCH_PLAIN_ESTIMATE": "1", "GCN_BENCH_SELFTEST_TIMEOUT": "1"})
    assert rc == 0 and wall <= 8.5, wall
    assert lines[0]["value"] == 100.0                              # printed before the hang
    hung = [o for o in lines[-1]["other_schedules"] if "overlap on" in o["schedule"]]
    assert hung and hung[0]["failed_rc"] == 124
    lane = [o for o in lines[-1]["other_schedules"] if "eval-lane on" in str(o["schedule"])]
    assert lane and "skipped" in lane[0]                           # nothing left of the deadline for it
    assert lines[-1]["value"] == 100.0 and lines[-1]["launcher"]["used_s"] <= 8.5


def test_launcher_skips_what_the_deadline_cannot_hold(monkeypatch, capsys):
    import time

    def behaviour(extra, timeout):
        k = _kind(extra)
        assert k == "plain", "self-test and optional schedules must be skipped with this little time"
        time.sleep(1.0)
        return 0, _fake_line(50.0, "plain one-stream")
    # 7 s - 5 s margin: no room for a self-test beside the plain run's estimate, and after a 1 s plain run less than the 1.2 s
    # an optional schedule is expected to take
    rc, lines, calls, _ = _launcher(monkeypatch, capsys, behaviour, {"GCN_BENCH_DEADLINE": "7", "GCN_BENCH_PLAIN_ESTIMATE": "30"})
    assert rc == 0 and len(calls) == 1 and calls[0][2]["HIPGCN_EXCHANGE"] == "allgather"       # no self-test: pinned
    assert lines[0]["value"] == 50.0
    assert all("skipped" in o for o in lines[-1]["other_schedules"]) and len(lines[-1]["other_schedules"]) == 2


def test_a_hung_group_is_killed_with_its_ranks_in_their_own_sessions():
    """torch.distributed.run starts every rank in a session of its own: killing the launcher's process group leaves hung ranks
    alive, holding the pipe this parent reads (found on the GPU box, round 6: the safe line was out, the call never returned).
    _kill_tree signals the launcher's group AND every descendant found under it in /proc."""
    import importlib
    import time
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    code = ("import subprocess, sys, time; subprocess.Popen([sys.executable, '-c', 'import time; time.sleep(1000)'], start_new_session=True); "
            "print('started', flush=True); time.sleep(1000)")
    p = subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE, text=True, start_new_session=True)
    assert p.stdout.readline().strip() == "started"
    kids = bench._descendants(p.pid)
    assert len(kids) == 1 and os.getpgid(kids[0]) != os.getpgid(p.pid)
    t0 = time.monotonic()
    assert bench._kill_tree(p) == 2
    p.communicate(timeout=15)                                    # the pipe closes: nobody is left holding it
    assert time.monotonic() - t0 < 10 and p.returncode == -9
    for _ in range(50):
        if not os.path.exists(f"/proc/{kids[0]}") or open(f"/proc/{kids[0]}/stat").read().split(")")[-1].split()[0] == "Z":
            break
        time.sleep(0.1)
    else:
        raise AssertionError("the grandchild survived")


def test_launcher_retries_pinned_and_reports_plain_failure(monkeypatch, capsys):
    seen = []

    def behaviour(extra, timeout):
        k = _kind(extra)
        if k == "selftest":
            return 0, json.dumps({"selftest": "ok"})
        seen.append(k)
        return (1, None) if len(seen) == 1 else (0, _fake_line(70.0, "plain one-stream"))
    rc, lines, calls, _ = _launcher(monkeypatch, capsys, behaviour, {"GCN_BENCH_DEADLINE": "420", "GCN_BENCH_PLAIN_ESTIMATE": "1"})
    assert rc == 0 and calls[1][2]["HIPGCN_EXCHANGE"] == "auto" and calls[2][2]["HIPGCN_EXCHANGE"] == "allgather"
    assert lines[0]["value"] == 70.0
    rc, lines, calls, _ = _launcher(monkeypatch, capsys, lambda e, t: (0, "{}") if "--selftest" in e else (1, None), {"GCN_BENCH_DEADLINE": "420", "GCN_BENCH_PLAIN_ESTIMATE": "1"})
    assert rc == 1 and lines == []


def test_optional_schedules_do_not_overwrite_the_dumped_outputs():
    """N > 1: only the plain schedule's ranks get --dump-outputs; the optional schedules run without it"""
    import importlib
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    assert bench._without_dump(["--steps", "3", "--dump-outputs", "d", "--warmup", "1"]) == ["--steps", "3", "--warmup", "1"]
    assert bench._without_dump(["--dump-outputs=d", "--steps", "3"]) == ["--steps", "3"]
    assert bench.parse_args(["--dump-outputs", "d"]).dump_outputs == "d" and bench.parse_args([]).dump_outputs is None


CONTRACT = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"]


def test_full_is_off_by_default_and_reaches_every_rank(monkeypatch, capsys):
    """a plain run measures the headline alone; --full (what used to run by default) is passed on to the ranks of every
    schedule the N > 1 launcher starts, the self-test excepted"""
    import importlib
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    assert bench.parse_args([]).full is False and bench.parse_args(["--full"]).full is True
    calls = []

    def fake(n_gpus, extra, timeout, env=None):
        calls.append(list(extra))
        return (0, json.dumps({"selftest": "ok"})) if "--selftest" in extra else (0, _fake_line(100.0, "plain one-stream"))
    monkeypatch.setattr(bench, "_run_ranks", fake)
    monkeypatch.setenv("GCN_BENCH_DEADLINE", "420")
    for argv, full in ((["--gpus", "8", "--steps", "3"], False), (["--gpus", "8", "--steps", "3", "--full"], True)):
        calls.clear()
        assert bench.launch_ranks(8, argv) == 0
        assert [_kind(c) for c in calls] == ["selftest", "plain", "overlap", "lane"]
        assert all(("--full" in c) == (full and _kind(c) != "selftest") for c in calls), calls
    capsys.readouterr()


@pytest.mark.gpu
def test_bench_one_gpu_line():
    p = run_bench(["--dataset", "reddit-mini", "--steps", 4, "--warmup", 1, "--full", "--bursts", 1, "--no-cpu-baseline", "--no-extras"])
    assert p.returncode == 0, p.stderr[-3000:]
    lines = json_lines(p.stdout)
    assert len(lines) == 1
    out = lines[0]
    for k in CONTRACT:
        assert k in out, k
    assert out["n_gpus"] == 1 and out["steps"] == 4 and out["value"] > 0
    assert abs(out["ms_per_step"] * out["value"] - 1e3) < 1e-6 * 1e3
    assert out["full"] is True and len(out["bursts"]["epochs_per_s"]) == 2
    r = out["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["launches"] > 0 and r["avg_launch_ms"] > 0


@pytest.mark.gpu
def test_bench_plain_line():
    """no --full: the headline line with its contract fields, and nothing that takes a run of its own after the timed steps"""
    p = run_bench(["--dataset", "reddit-mini", "--steps", 4, "--warmup", 1])
    assert p.returncode == 0, p.stderr[-3000:]
    lines = json_lines(p.stdout)
    assert len(lines) == 1
    out = lines[0]
    for k in CONTRACT:
        assert k in out, k
    assert out["metric"] == "epochs_per_sec" and out["unit"] == "epochs/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["n_gpus"] == 1 and out["steps"] == 4 and out["warmup"] == 1 and out["value"] > 0
    assert abs(out["ms_per_step"] * out["value"] - 1e3) < 1e-6 * 1e3
    assert out["full"] is False and out["roofline"] is None and out["cpu_baseline"] is None
    assert out["config"]["eval_lane"] == "on" and 0 < out["final"]["train_loss"] < 10
    for k in ("bursts", "sustained", "breakdown_ms_per_epoch", "train_only_ms_per_epoch", "value_reference_op_order_all_rows",
              "value_no_row_groups", "value_no_label_hint", "value_f32_products", "structure_legs", "roofline_dense", "cli"):
        assert k not in out, k


@pytest.mark.gpu
def test_bench_dumps_the_last_step_outputs(tmp_path):
    """--dump-outputs: the timed path's trace (one row per timed step, the last one = the line's `final`), the weights and a
    seeded sample of the training logits, all float32 / float64 and small; the sampled rows are training rows"""
    import numpy as np
    d = tmp_path / "out"
    p = run_bench(["--dataset", "reddit-mini", "--steps", 3, "--warmup", 1, "--bursts", 0, "--no-cpu-baseline", "--no-extras",
                   "--dump-outputs", d])
    assert p.returncode == 0, p.stderr[-3000:]
    out = json_lines(p.stdout)[0]
    arrays = {f.stem: np.load(f) for f in d.glob("*.npy")}
    assert set(arrays) == {"trace", "w1", "w2", "train_logits_sample", "train_logits_sample_rows"}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 2**20
    tr = arrays["trace"]
    assert tr.shape == (3, 4) and np.isfinite(tr).all()
    f = out["final"]
    assert tr[-1].tolist() == [np.float32(f[k]) for k in ("train_loss", "train_acc", "val_loss", "val_acc")]
    assert arrays["w1"].shape == (602, 128) and arrays["w2"].shape == (128, 41)
    from cuda_gcn_amd import datagen
    ds = datagen.make_dataset("reddit-mini")
    rows = arrays["train_logits_sample_rows"].astype(np.int64)
    z = arrays["train_logits_sample"]
    assert z.shape == (rows.size, 41) and rows.size == min(4096, int((ds["split"] == 1).sum()))
    assert (ds["split"][rows] == 1).all() and np.isfinite(z).all() and np.abs(z).max() > 0


@pytest.mark.gpu
def test_bench_extras_on_a_small_graph():
    """the extra legs of the one-GPU line (label hint withheld, no row groups, reference operation order, the R-MAT leg of
    the roofline — here at a small scale, so the code path and not the HBM regime is what is exercised)"""
    p = run_bench(["--dataset", "reddit-mini", "--steps", 4, "--warmup", 1, "--full", "--bursts", 0, "--no-cpu-baseline", "--hbm-scale", 15])
    assert p.returncode == 0, p.stderr[-3000:]
    out = json_lines(p.stdout)[0]
    assert out["config"]["eval_lane"] == "on"                  # one GPU: validation forward on the second stream
    assert out["value_reference_op_order_all_rows"] > 0
    if out["config"]["aggregation_schedule"] == "label-major":
        assert out["value_no_label_hint"] > 0 and "aggregation_schedule_no_label_hint" in out["config"]
    if out["config"]["aggregation_schedule"] != "degree":
        assert out["value_no_row_groups"] > 0
    leg = out["roofline"]["hbm_regime"]
    assert "error" not in leg, leg
    assert leg["bound"] == "hbm" and leg["achieved"] > 0 and leg["launches"] > 0


@pytest.mark.gpu
def test_bench_two_ranks_self_launched():
    p = run_bench(["--gpus", 2, "--dataset", "reddit-mini", "--steps", 3, "--warmup", 1, "--full", "--bursts", 0, "--no-cpu-baseline"],
                  env={"GCN_BENCH_TRANSPORT": "host", "GCN_BENCH_DEVICE": "0", "GCN_BENCH_TIMEOUT": "600", "GCN_BENCH_DEADLINE": "600"})
    assert p.returncode == 0, p.stderr[-3000:]
    lines = json_lines(p.stdout)
    assert 1 <= len(lines) <= 2, p.stdout                     # the safe (plain-schedule) line at once, the best line last
    assert lines[0]["config"]["schedule"] == "plain one-stream"
    out = lines[-1]
    assert out["value"] >= lines[0]["value"]
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["value"] > 0
    assert out["config"]["parallelism"] == "row-partition x2"
    assert "comm" in out["breakdown_ms_per_epoch"]
    assert 0 < out["final"]["train_loss"] < 10
    assert len(out["other_schedules"]) == 2 and out["launcher"]["used_s"] <= out["launcher"]["deadline_s"]


@pytest.mark.gpu
def test_bench_safe_line_survives_a_hung_optional_schedule():
    """verdict r05 item 3: four ranks (host transport, all on GPU 0 — the box allows six GPU processes, so not eight), the
    children of the `--overlap on` schedule made to hang: the plain line is out before that leg starts, the leg is killed at
    what the deadline leaves, and the whole call ends inside the deadline with the safe line's N > 1 fields present."""
    import time
    deadline = 200
    t0 = time.monotonic()
    # (the hung schedule's own limit, 45 s, ends it long before the deadline would: the suite need not wait for that)
    p = run_bench(["--gpus", 4, "--dataset", "reddit-mini", "--steps", 3, "--warmup", 1, "--full", "--bursts", 0],
                  env={"GCN_BENCH_TRANSPORT": "host", "GCN_BENCH_DEVICE": "0", "GCN_BENCH_DEADLINE": str(deadline), "GCN_BENCH_LANE_TIMEOUT": "45",
                       "GCN_BENCH_TEST_HANG": "overlap"},
                  timeout=deadline + 60)
    wall = time.monotonic() - t0
    assert p.returncode == 0, p.stderr[-3000:]
    assert wall <= deadline + 15, wall
    lines = json_lines(p.stdout)
    assert lines, p.stdout
    safe = lines[0]
    assert safe["n_gpus"] == 4 and safe["value"] > 0 and safe["config"]["schedule"] == "plain one-stream"
    assert safe["config"]["transport"].startswith("host") and "rccl_ranks" in safe["config"]
    assert safe["roofline"]["collectives_per_epoch"] > 0
    assert safe["cpu_baseline"] is None                          # N > 1: the CPU baseline belongs to the N = 1 line
    last = lines[-1]
    hung = [o for o in last.get("other_schedules", []) if "overlap on" in str(o.get("schedule"))]
    assert hung and hung[0]["value"] is None and (hung[0].get("failed_rc") == 124 or "skipped" in hung[0]), last.get("other_schedules")
