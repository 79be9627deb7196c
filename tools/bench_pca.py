"""PCA of the hidden layer of reddit-syn (hidden 128) at k = 2 and k = 50, HIP events — the figures of DESIGN §4.21:
  * the mean launches, the scatter launches and the projection launch of csrc/pca.hip timed apart on the model's own hidden
    matrix with its inverse norms;
  * each against its byte floor at the HBM rate (6.3 TB/s): the mean reads the table once (n . h . 4 B), the scatter call —
    mean and scatter back to back, as pca() runs them — twice, the projection once (plus n . k . 4 B written);
  * each against one evaluation forward, timed the same way: wall time of the call with its synchronisation (`*_wall_ms`,
    `*_wall_over_eval_forward`; the HIP-event times of back-to-back launches are not divided by a wall time);
  * the host's eigen solver (model.sym_eigen) on planted scatter matrices of h = 128 and 256: wall time, residual and orthogonality
    ratios (DESIGN §4.21 defines them);
  * pca() as a whole (wall time) against embed() of every node plus numpy on the host (float64 covariance, numpy.linalg.eigh,
    the projection);
  * with --parent DIR (a built checkout of the parent commit): `python bench.py --gpus 1 --steps 50 --warmup 10` in DIR and here,
    alternating --rounds times (default 2): the epoch path is meant not to move.
Prints one JSON line, with the hashes of the sources it measured (cuda_gcn_amd/provenance.py); --out FILE also writes it there.
None of the values is a pass/fail threshold.  usage: bench_pca.py [dataset] [hidden] [epochs] [--out FILE] [--parent DIR] [--rounds N]"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_gcn_amd import datagen, provenance
from cuda_gcn_amd.model import HipGCNModel, sym_eigen
from cuda_gcn_amd.ops import Device, _ck

HBM_BYTES_S = 6.3e12


def timeit(dev, fn, iters, warmup=1):
    lib = dev.lib
    e0, e1 = C.c_void_p(), C.c_void_p()
    lib.gcnhip_event_create(C.byref(e0)); lib.gcnhip_event_create(C.byref(e1))
    for _ in range(warmup):
        fn()
    dev.sync()
    lib.gcnhip_event_record(dev.ctx, e0)
    for _ in range(iters):
        fn()
    lib.gcnhip_event_record(dev.ctx, e1)
    dev.sync()
    ms = C.c_float()
    lib.gcnhip_event_elapsed_ms(e0, e1, C.byref(ms))
    lib.gcnhip_event_destroy(e0); lib.gcnhip_event_destroy(e1)
    return ms.value / iters


def wall(fn, reps=3):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def note(text):
    print(f"bench_pca: {text}", file=sys.stderr, flush=True)


def epoch_path(parent, rounds):
    """bench.py on the parent checkout and on this one, alternating: epochs/s of every run"""
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = dict(parent=[], this=[])
    for _ in range(rounds):
        for label, root in (("parent", parent), ("this", here)):
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "50", "--warmup", "10"], cwd=root, capture_output=True, text=True,
                               timeout=600, check=True)
            out[label].append(json.loads(r.stdout.strip().splitlines()[-1])["value"])
            note(f"bench.py on {label}: {out[label][-1]}")
    return out


def host_pca(x, k):
    """what a user did before pca(): the exported rows, float64 covariance, eigh, projection"""
    x = x.astype(np.float64)
    c = x - x.mean(0)
    w, v = np.linalg.eigh(c.T @ c)
    return (c @ v[:, ::-1][:, :k]).astype(np.float32), w[::-1]


def solver_figures():
    """sym_eigen on the scatter matrix of a planted table (x = (z . s) Q + offset, s = 16, 8, 4, 2, 1.5, 1, .75, .5, 0.1, ..)"""
    out = {}
    eps = 2.0 ** -52
    for h in (128, 256):
        rng = np.random.default_rng(h)
        sp = np.array(([16, 8, 4, 2, 1.5, 1, .75, .5] + [0.1] * h)[:h])
        x = ((rng.standard_normal((1000, h)) * sp) @ np.linalg.qr(rng.standard_normal((h, h)))[0] + rng.uniform(0, 3, h)).astype(np.float32).astype(np.float64)
        c = x - x.mean(0)
        s = c.T @ c
        s = (s + s.T) / 2
        lam, v = sym_eigen(s)
        out[f"h{h}"] = dict(wall_ms=wall(lambda: sym_eigen(s), reps=3),
                            residual_ratio=float(np.linalg.norm(s @ v - v * lam, axis=0).max() / (h * eps * np.linalg.norm(s))),
                            orthogonality_ratio=float(np.abs(v.T @ v - np.eye(h)).max() / (h * eps)))
    return out


def main():
    args = sys.argv[1:]
    opts = {"--parent": None, "--rounds": "2", "--out": None}
    for flag in list(opts):
        if flag in args:
            i = args.index(flag)
            opts[flag] = args[i + 1]
            del args[i:i + 2]
    name = args[0] if len(args) > 0 else "reddit-syn"
    hidden = int(args[1]) if len(args) > 1 else 128
    epochs = int(args[2]) if len(args) > 2 else 5
    ds = datagen.make_dataset(name)
    N = ds["num_nodes"]
    res = dict(dataset=name, nodes=N, hidden=hidden, epochs=epochs)
    m = HipGCNModel(ds, seed=1, hidden_dim=hidden, dropout=0.5)
    m.run_epochs(epochs, want_trace=False)
    res["eval_forward_wall_ms"] = wall(lambda: m.eval(2), reps=9)
    note(f"model trained; evaluation forward {res['eval_forward_wall_ms']:.3f} ms")
    for k in (2, 50):
        out = {}
        fit = m.pca(k=k)
        out["pca_wall_ms"] = wall(lambda: m.pca(k=k), reps=3)
        out["pca_fit_only_wall_ms"] = wall(lambda: m.pca(k=k, coords=False), reps=3)
        out["rank"], out["ratio_first"] = fit["rank"], [float(v) for v in fit["explained_variance_ratio"][:min(k, 5)]]
        t0 = time.perf_counter()
        y, w = host_pca(m.embed(normalize=True), k)
        out["embed_plus_numpy_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        out["eigenvalue_max_rel_diff_to_numpy"] = float(np.abs(fit["eigenvalues"] - np.maximum(w, 0)).max() / w[0])
        res[f"k{k}"] = out
        note(f"pca() at k = {k}: {out}")
    emb = m.embed()
    m.close()
    # ---- the launches themselves, on the same matrix
    dev = Device(0)
    lib = dev.lib
    table, inv = dev.buf(emb), dev.buf((N,), np.float32)
    _ck(lib, lib.gcnhip_embed_inv_norms(dev.ctx, table.ptr, hidden, N, hidden, inv.ptr), "inv_norms")
    bytes_table = N * hidden * 4.0
    plan = dev.pca_plan(N, hidden)
    sb = dev.buf((plan["bytes_full"] // 4 + 4,), np.uint32)
    mb, cb, sc = dev.buf((hidden,), np.float64), dev.buf((1,), np.int32), dev.buf((hidden, hidden), np.float64)

    def mean():
        _ck(lib, lib.gcnhip_pca_mean(dev.ctx, table.ptr, hidden, N, hidden, inv.ptr, None, N, mb.ptr, cb.ptr, sb.ptr, plan["bytes_full"]), "mean")

    def scatter():
        _ck(lib, lib.gcnhip_pca_scatter(dev.ctx, table.ptr, hidden, N, hidden, inv.ptr, None, N, mb.ptr, sc.ptr, sb.ptr, plan["bytes_full"]), "scatter")

    mean(); scatter()
    launches = dict(mean_ms=timeit(dev, mean, 20), scatter_ms=timeit(dev, scatter, 20), scratch_mb=plan["bytes_full"] / 2 ** 20,
                    mean_floor_hbm_ms=1e3 * bytes_table / HBM_BYTES_S, mean_plus_scatter_floor_hbm_ms=2e3 * bytes_table / HBM_BYTES_S)
    launches["mean_plus_scatter_ms"] = launches["mean_ms"] + launches["scatter_ms"]
    launches["scatter_tflops_f64"] = 2.0 * N * hidden * hidden / 2 / (launches["scatter_ms"] * 1e-3) / 1e12     # the upper triangle
    for key, fn in (("mean", mean), ("scatter", scatter)):         # like for like with the forward: wall time with the synchronisation
        launches[key + "_wall_ms"] = wall(lambda: (fn(), dev.sync()), reps=9)
        launches[key + "_wall_over_eval_forward"] = launches[key + "_wall_ms"] / res["eval_forward_wall_ms"]
    res["launches"] = launches
    note(f"mean {launches['mean_ms']:.4f} ms, scatter {launches['scatter_ms']:.4f} ms (floors {launches['mean_floor_hbm_ms']:.4f} each)")
    for k in (2, 50):
        basis = np.ascontiguousarray(np.linalg.qr(np.random.default_rng(k).standard_normal((hidden, hidden)))[0][:, :k], np.float64)
        vb, ob = dev.buf(basis), dev.buf((N, k), np.float32)

        def project():
            _ck(lib, lib.gcnhip_pca_project(dev.ctx, table.ptr, hidden, N, hidden, inv.ptr, None, N, mb.ptr, vb.ptr, k, k, None, ob.ptr, k), "project")
        project()
        out = res[f"k{k}"]
        out["project_ms"] = timeit(dev, project, 20)
        out["project_floor_hbm_ms"] = 1e3 * (bytes_table + 4.0 * N * k) / HBM_BYTES_S
        out["project_wall_ms"] = wall(lambda: (project(), dev.sync()), reps=9)
        out["project_wall_over_eval_forward"] = out["project_wall_ms"] / res["eval_forward_wall_ms"]
        note(f"projection at k = {k}: {out['project_ms']:.4f} ms (floor {out['project_floor_hbm_ms']:.4f})")
        vb.free(); ob.free()
    for b in (sb, mb, cb, sc, table, inv):
        b.free()
    dev.close()
    res["sym_eigen"] = solver_figures()
    note(f"sym_eigen: {res['sym_eigen']}")
    if opts["--parent"]:
        runs = epoch_path(opts["--parent"], int(opts["--rounds"]))
        res["epoch_path"] = dict(runs, parent_median=float(np.median(runs["parent"])), this_median=float(np.median(runs["this"])))
    res["_meta"] = dict(sources=provenance.source_sha(["pca.hip", "embed.hip", "common.h", "cuda_gcn_amd/host/pca.cpp", "cuda_gcn_amd/host/pca_query.cpp"]))
    line = json.dumps(res)
    print(line)
    if opts["--out"]:
        with open(opts["--out"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
