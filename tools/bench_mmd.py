"""The kernel two-sample walk on the hidden layer of reddit-syn (hidden 128), HIP events over 10 launches — the figures of DESIGN §4.31:
  * over 4 096 rows, 16 384 rows and the train + test rows, at Bp = 16 and Bp = 256 columns of the membership matrix: gcnhip_mmd_walk
    (the pack, the walk launches and their folds) against the f32-MFMA floor 2 n^2 (dpad + Bp) / 157.3 TF, and beside it
    gcnhip_tsne_gradient on the same rows — the closest existing launch: one n x n product and an exponential-free kernel per entry;
  * mmd() as a whole (wall time, 8 192 + 8 192 rows, 200 permutations) against embed() plus the same statistic in numpy on the host
    (float64 Gram matrix, the same permutations);
  * with --parent DIR (a built checkout of the parent commit): `python bench.py --gpus 1 --steps 50 --warmup 10` in DIR and here,
    alternating --rounds times (default 3): the epoch path is meant not to move.
Prints one JSON line, with the hashes of the sources it measured (cuda_gcn_amd/provenance.py); --out FILE also writes it there.
None of the values is a pass/fail threshold.  usage: bench_mmd.py [dataset] [hidden] [epochs] [--out FILE] [--parent DIR] [--rounds N]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_kmeans import epoch_path, timeit, wall
from cuda_gcn_amd import datagen, provenance
from cuda_gcn_amd.model import HipGCNModel
from cuda_gcn_amd.ops import Device, _ck

MFMA_F32_FLOPS = 157.3e12
SCRATCH_CAP = 256 << 20


def note(text):
    print(f"bench_mmd: {text}", file=sys.stderr, flush=True)


def host_mmd(x, m, member):
    """the biased statistic of the observed groups and of every column of member, float64 numpy: one Gram matrix, then K . S"""
    x = x.astype(np.float64)
    x -= x.mean(0)
    xn = (x * x).sum(1)
    d2 = np.maximum(xn[:, None] + xn[None, :] - 2.0 * x @ x.T, 0.0)
    n = x.shape[0]
    k = np.exp(-(n - 1) / (2.0 * xn.sum()) * d2)
    s = member.astype(np.float64)
    t, r = k @ s, k.sum(1, keepdims=True)
    aa, ab, bb = (t * s).sum(0), (t * (1 - s)).sum(0), ((r - t) * (1 - s)).sum(0)
    return aa / m ** 2 + bb / (n - m) ** 2 - 2 * ab / (m * (n - m))


def launches(dev, emb, inv, rows, bp, out):
    lib = dev.lib
    N, h = emb.shape
    n = int(rows.size)
    rng = np.random.default_rng(0)
    member = rng.random((n, bp)) < 0.5
    member[:, 0] = True
    unit = emb[rows] * inv[rows][:, None]
    shift = unit.mean(0, dtype=np.float64).astype(np.float32)
    gamma = (n - 1) / (2.0 * ((unit - shift).astype(np.float64) ** 2).sum())
    plan = dev.mmd_plan(n, h, bp, False)
    sbytes = max(min(plan["bytes"], SCRATCH_CAP), plan["bytes_min"])
    table, invb, rb, hb = dev.buf(emb), dev.buf(inv), dev.buf(np.ascontiguousarray(rows, np.int32)), dev.buf(shift)
    bb, sb = dev.buf(np.packbits(member, axis=1, bitorder="little").ravel()), dev.buf((sbytes // 4 + 4,), np.uint32)

    def walk():
        _ck(lib, lib.gcnhip_mmd_walk(dev.ctx, table.ptr, h, N, h, invb.ptr, rb.ptr, n, hb.ptr, float(gamma), bb.ptr, bp, 0, sb.ptr, sbytes), "walk")
    dpad = (h + 15) // 16 * 16
    out.update(rows=n, bp=bp, scratch_mb=sbytes / 2 ** 20, full_scratch_mb=plan["bytes"] / 2 ** 20, walk_ms=timeit(dev, walk, 10))
    out["floor_mfma_ms"] = 1e3 * 2.0 * n * n * (dpad + bp) / MFMA_F32_FLOPS
    out["share_of_floor"] = out["floor_mfma_ms"] / out["walk_ms"]
    for b in (table, invb, rb, hb, bb, sb):
        b.free()


def tsne_gradient_ms(dev, emb, inv, rows, h):
    n = int(rows.size)
    plan = dev.tsne_plan(n, h)
    sbytes = max(min(plan["bytes"], SCRATCH_CAP), plan["bytes_min"])
    pk = dev.tsne_pack(emb, rows=rows, inv_norm=inv, scratch_bytes=sbytes)
    dev.tsne_bandwidths(pk, 30.0)
    y = dev.buf((1e-2 * np.random.default_rng(0).standard_normal((n, 2))).astype(np.float32))
    sums = dev.buf((n * 9,), np.float64)

    def grad():
        _ck(dev.lib, dev.lib.gcnhip_tsne_gradient(dev.ctx, pk["pack"].ptr, n, h, y.ptr, 2, 0, sums.ptr, pk["scratch"].ptr, sbytes), "gradient")
    return timeit(dev, grad, 10)


def main():
    args = sys.argv[1:]
    opts = {"--parent": None, "--rounds": "3", "--out": None}
    for flag in list(opts):
        if flag in args:
            i = args.index(flag)
            opts[flag] = args[i + 1]
            del args[i:i + 2]
    name = args[0] if len(args) > 0 else "reddit-syn"
    hidden = int(args[1]) if len(args) > 1 else 128
    epochs = int(args[2]) if len(args) > 2 else 5
    ds = datagen.make_dataset(name)
    N, split = ds["num_nodes"], np.asarray(ds["split"])
    res = dict(dataset=name, nodes=N, hidden=hidden, epochs=epochs)
    m = HipGCNModel(ds, seed=1, hidden_dim=hidden, dropout=0.5)
    m.run_epochs(epochs, want_trace=False)
    a, b = np.flatnonzero(split == 1)[:8192], np.flatnonzero(split == 3)[:8192]
    kw = dict(nodes_a=a, nodes_b=b, permutations=200, seed=0)
    got = m.mmd(**kw)
    whole = dict(m=got["m"], n=got["n"], permutations=200, mmd_wall_ms=wall(lambda: m.mmd(**kw), reps=2), mmd2_biased=got["mmd2_biased"],
                 p_value=got["p_value"], gamma=got["gamma"])
    t0 = time.perf_counter()
    x = m.embed(nodes=np.concatenate([a, b]), normalize=True)
    rng, member = np.random.default_rng(0), np.zeros((x.shape[0], 201), bool)
    member[:a.size, 0] = True
    for p in range(200):
        member[rng.permutation(x.shape[0])[:a.size], 1 + p] = True
    host = host_mmd(x, a.size, member)
    whole.update(embed_plus_numpy_wall_ms=1e3 * (time.perf_counter() - t0), numpy_mmd2_biased=float(host[0]),
                 numpy_p_value=(1 + int((host[1:] >= host[0]).sum())) / 201)
    res["whole"] = whole
    note(f"mmd() as a whole: {whole}")
    emb = m.embed()
    m.close()
    dev = Device(0)
    inv = dev.embed_inv_norms(emb)
    rng = np.random.default_rng(0)
    lists = dict(sample_4096=np.sort(rng.choice(N, min(4096, N), replace=False)), sample_16384=np.sort(rng.choice(N, min(16384, N), replace=False)),
                 train_test=np.flatnonzero((split == 1) | (split == 3)))
    for label, rows in lists.items():
        rows = rows.astype(np.int32)
        out = dict(tsne_gradient_ms=tsne_gradient_ms(dev, emb, inv, rows, hidden))
        for bp in (16, 256):
            one = {}
            launches(dev, emb, inv, rows, bp, one)
            out[f"bp{bp}"] = one
        res[label] = out
        note(f"{label}: {out}")
    dev.close()
    if opts["--parent"]:
        runs = epoch_path(opts["--parent"], int(opts["--rounds"]))
        res["epoch_path"] = dict(runs, parent_median=float(np.median(runs["parent"])), this_median=float(np.median(runs["this"])))
    res["_meta"] = dict(sources=provenance.source_sha(["mmd.hip", "tsne.hip", "pca.hip", "common.h", "cuda_gcn_amd/host/mmd_query.cpp"]))
    line = json.dumps(res)
    print(line)
    if opts["--out"]:
        with open(opts["--out"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
