"""The kernel two-sample sums on the GPU (csrc/mmd.hip, ops.Device.mmd_walk, HipGCNModel.mmd) against the float64 reference of
tests/mmd_ref.py: every sum inside the bound derived for the kernel's chains, integer tables exactly, the model against the chained
ops calls byte for byte and against Gaussian samples, the command line against mmd() on the same weights."""
import os
import subprocess

import numpy as np
import pytest

from cuda_gcn_amd import datagen
from tests import mmd_ref as R

pytestmark = pytest.mark.gpu
HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cuda_gcn_amd", "bin", "gcn-hip")
GROUPS = [(1, 1), (3, 70), (64, 64), (65, 130), (500, 525)]   # the last: one position more than a part of 1024, so two parts fold


@pytest.fixture(scope="module")
def dev():
    from cuda_gcn_amd.ops import Device
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def trained():
    from cuda_gcn_amd import model as M
    m = M.HipGCNModel(datagen.make_dataset("cora-syn"), seed=5, hidden_dim=16, dropout=0.5)
    m.run_epochs(5, want_trace=False)
    yield m
    m.close()


def case(m, rest, dim, bp):
    """positive rows far from the origin (ReLU rows), a table with spare rows and a row stride of dim + 5; beyond (1, 1) the list has
    one position more that names no row (its bits are set all the same: the kernel must not count them) and one repeated row; inverse
    norms for every other dim; group A shifted a little, so that the sums differ; the last column repeats column 1"""
    rng = np.random.default_rng(1000 * m + 10 * rest + dim)
    n = m + rest + (1 if m + rest > 2 else 0)
    n_table = n + 3
    table = np.abs(rng.standard_normal((n_table, dim)) + 1.0).astype(np.float32)
    rows = rng.permutation(n_table)[:n].astype(np.int32)
    table[rows[:m]] += np.float32(0.5)
    if n > 2:
        rows[-1], rows[m + 1] = n_table, rows[m]
    inv = (1.0 / np.linalg.norm(table, axis=1)).astype(np.float32) if dim % 2 else None
    x0, ok = R.operands(table, rows, inv, np.zeros(dim, np.float32))
    shift = x0[ok].astype(np.float64).mean(0).astype(np.float32)
    xp, ok = R.operands(table, rows, inv, shift)
    spread = float((xp[ok].astype(np.float64) ** 2).sum(1).mean())
    member = R.membership(n, m, bp - 3, rng, pad_to=bp)
    member[:, bp - 1] = member[:, 1]
    if n > 2:
        member[-1] = True
    return dict(table=table, rows=rows, inv=inv, shift=shift, xp=xp, ok=ok, member=member, gamma=0.5 / spread if spread > 0 else 0.7, dim=dim)


@pytest.mark.parametrize("dim", [1, 17, 128, 129, 256])
@pytest.mark.parametrize("m,rest", GROUPS)
def test_walk_holds_the_derived_bound(dev, m, rest, dim):
    bp = (16, 48, 256)[(GROUPS.index((m, rest)) + dim) % 3]
    c = case(m, rest, dim, bp)
    want = R.sums64(c["xp"], c["ok"], c["member"], c["gamma"])
    kw = dict(rows=c["rows"], inv_norm=c["inv"], ld=dim + 5, want_witness=True)
    got = dev.mmd_walk(c["table"], c["shift"], c["gamma"], c["member"], **kw)
    assert (got["points"], got["m"]) == (m + rest, m) == (want["m"] + want["rest"], want["m"])
    assert np.all(np.abs(got["sums"] - want["sums"]) <= want["err"]), (np.abs(got["sums"] - want["sums"]) / want["err"]).max()
    assert got["sums"][:, bp - 1].tobytes() == got["sums"][:, 1].tobytes()          # a permutation equal to the observed groups
    assert got["sums"][1, 0] == 0 and got["sums"][2, 0] == 0                         # nothing lies outside the column of ones
    ok = c["ok"]
    assert np.all(np.abs(got["witness"][ok] - want["witness"][ok]) <= want["witness_err"][ok]) and np.all(np.isnan(got["witness"][~ok]))
    least = dev.mmd_plan(got["points"] + (~ok).sum(), dim, bp, True)["bytes_min"]
    small = dev.mmd_walk(c["table"], c["shift"], c["gamma"], c["member"], scratch_bytes=least, **kw)
    assert small["sums"].tobytes() == got["sums"].tobytes() and small["witness"].tobytes() == got["witness"].tobytes()
    assert dev.mmd_walk(c["table"], c["shift"], c["gamma"], c["member"], **dict(kw, want_witness=False))["sums"].tobytes() == got["sums"].tobytes()


@pytest.mark.parametrize("n,dim,bp", [(200, 17, 16), (1100, 130, 48)])
def test_integer_rows_count_exactly(dev, n, dim, bp):
    """gamma = 0: every k is 1, so the sums are the int64 pair counts of groups of any size"""
    rng = np.random.default_rng(n)
    table = rng.integers(-3, 4, (n, dim)).astype(np.float32)
    member = rng.random((n, bp)) < 0.4
    member[:, 0] = True
    got = dev.mmd_walk(table, np.zeros(dim, np.float32), 0.0, member)
    a = member.sum(0).astype(np.int64)
    assert np.array_equal(got["sums"], np.stack([a * a, (n - a) * a, (n - a) * (n - a)]).astype(np.float64))


def chained(dev, x, m, perms, seed, gamma=None):
    """mmd()'s launches one by one on rows x whose first m are group A"""
    from cuda_gcn_amd import model as M
    n = x.shape[0]
    mean = dev.pca_mean(x)[0]
    shift = mean.astype(np.float32)
    g = (n - 1) / (2.0 * np.trace(dev.pca_scatter(x, mean=mean))) if gamma is None else gamma
    member = R.membership(n, m, perms, np.random.default_rng(seed))
    cols, wit = [], None
    for p0 in range(0, max(perms, 1), 254):
        chunk = min(254, perms - p0)
        s = np.zeros((n, (2 + chunk + 15) // 16 * 16), bool)
        s[:, :2], s[:, 2:2 + chunk] = member[:, :2], member[:, 2 + p0:2 + p0 + chunk]
        got = dev.mmd_walk(x, shift, g, s, want_witness=p0 == 0)
        cols.append(got["sums"][:, (1 if p0 == 0 else 2):2 + chunk])
        wit = got["witness"] if p0 == 0 else wit
    return dict(M.mmd_stats(np.concatenate(cols, 1), m, n - m), witness=wit, gamma=float(np.float32(g)))


@pytest.mark.parametrize("perms,gamma", [(300, None), (0, 0.25)])
def test_model_is_the_chained_ops_calls(dev, trained, perms, gamma):
    """byte for byte, over two chunks of permutations, under every scratch cap, and with the groups interleaved in data"""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((320, 17)).astype(np.float32)
    x[:150] += 0.3
    flag = np.zeros(320, bool)
    flag[rng.permutation(320)[:150]] = True
    data = np.zeros_like(x)
    data[flag], data[~flag] = x[:150], x[150:]
    kw = dict(data=data, groups=flag, permutations=perms, seed=9, gamma=gamma, normalize=False)
    got, want, small = trained.mmd(**kw), chained(dev, x, 150, perms, 9, gamma), trained.mmd(scratch_bytes=1, **kw)
    for res in (got, small):
        assert (res["mmd2_biased"], res["mmd2_unbiased"], res["p_value"], res["gamma"]) == (want["biased"][0], want["unbiased"][0], want["p_value"], want["gamma"])
        assert res["null"].tobytes() == want["biased"][1:].tobytes() and res["witness"].tobytes() == want["witness"].tobytes()
    assert (got["m"], got["n"], got["permutations"]) == (150, 170, perms) and np.array_equal(got["nodes"][:150], np.flatnonzero(flag))
    two = trained.mmd(**dict(kw, gamma=[0.25, 1.0], permutations=20))
    assert two["mmd2_biased"].shape == (2,) and two["null"].shape == (2, 20) and two["witness"].shape == (2, 320)
    assert two["mmd2_biased"][0] == trained.mmd(**dict(kw, gamma=0.25, permutations=20))["mmd2_biased"]


def test_model_tells_one_gaussian_from_two(trained):
    """seeds whose float64 reference (R.whole64 on the host) gives 0.876 and 1 / 201"""
    x = np.random.default_rng(11).standard_normal((200, 8))
    groups = np.arange(200) < 100
    assert R.whole64(x, 100, 200, 11)[1] > 0.05 and R.whole64(x + 2.0 * ~groups[:, None], 100, 200, 11)[1] == 1 / 201
    same = trained.mmd(data=x, groups=groups, permutations=200, seed=11, normalize=False, witness=False)
    far = trained.mmd(data=x + 2.0 * ~groups[:, None], groups=groups, permutations=200, seed=11, normalize=False)
    assert same["p_value"] > 0.05 and far["p_value"] == 1 / 201 and far["mmd2_biased"] > 10 * same["mmd2_biased"]
    assert np.all(far["witness"][:100] > 0) and np.all(far["witness"][100:] < 0)       # the witness is positive where A is denser


def test_model_on_embeddings(trained):
    """the trained model's own rows: train against test, the weights untouched, the refusals that need a model"""
    from cuda_gcn_amd import model as M
    before = [trained.var(v).tobytes() for v in (2, 5)]
    split = np.asarray(datagen.make_dataset("cora-syn")["split"])
    got = trained.mmd(permutations=50)
    assert (got["m"], got["n"]) == ((split == 1).sum(), (split == 3).sum()) and 1 / 51 <= got["p_value"] <= 1 and got["gamma"] > 0
    assert got["witness"].shape == (got["m"] + got["n"],) and np.array_equal(got["nodes"], np.concatenate([np.flatnonzero(split == 1), np.flatnonzero(split == 3)]))
    assert trained.mmd(permutations=50)["null"].tobytes() == got["null"].tobytes()
    half = trained.mmd(nodes_a=np.flatnonzero(split == 1), nodes_b=np.flatnonzero(split == 3), permutations=50, witness=False)
    assert half["mmd2_biased"] == got["mmd2_biased"] and half["p_value"] == got["p_value"] and "witness" not in half
    assert [trained.var(v).tobytes() for v in (2, 5)] == before
    for kw, word in ((dict(nodes_a=[1, 2], nodes_b=[2, 3]), "overlap"), (dict(nodes_a=[], nodes_b=[2, 3]), "empty group"), (dict(gamma=0.0), "gamma"),
                     (dict(gamma=[1, 2, 3, 4, 5]), "at most 4"), (dict(permutations=-1), "permutations"), (dict(split_a=4), "split"),
                     (dict(nodes_a=[10 ** 6], nodes_b=[1]), "node"), (dict(data=np.ones((4, 257), np.float32), groups=[1, 1, 0, 0]), "256")):
        with pytest.raises(M.GcnHostError, match=word):
            trained.mmd(**kw)
    bf = M.HipGCNModel(datagen.make_dataset("cora-syn"), seed=1, flags=M.BF16_TABLES, hidden_dim=16)
    with pytest.raises(M.GcnHostError, match="bf16"):
        bf.mmd()
    bf.close()


def test_cli_mmd(tmp_path):
    """GCN_MMD prints the numbers of m.mmd on the same weights and writes its witness; the permutations of the command line are its own
    (mt19937_64), so p is compared without any, where it is 1, and with 40 only held to its range"""
    from cuda_gcn_amd.model import HipGCNModel
    ds = datagen.make_dataset("cora-syn")
    (tmp_path / "data").mkdir()
    datagen.write_gcnbin(ds, str(tmp_path / "data" / "cora-syn.gcnbin"))
    m = HipGCNModel(ds, seed=3, hidden_dim=16, dropout=0.5)
    m.run_epochs(6, want_trace=False)
    w, out = str(tmp_path / "w.gcnw"), str(tmp_path / "mmd.txt")
    m.save_weights(w)
    want = m.mmd(split_a=2, split_b=3, permutations=0)
    m.close()
    args = ["timeout", "-k", "10", "50", HIP, "cora-syn", "-", "-", "16", "-", "0.5", "-", "-", "0"]
    env = dict(os.environ, GCN_SEED="3", GCN_LOAD_WEIGHTS=w, GCN_MMD=out, GCN_MMD_SPLITS="2,3", GCN_MMD_PERMS="0")
    r = subprocess.run(args, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-1000:]
    fields = dict(p.split("=") for p in r.stdout.strip().splitlines()[-1].split())
    assert list(fields) == ["mmd2", "mmd2_unbiased", "p", "gamma"]
    assert [float(v) for v in fields.values()] == [want["mmd2_biased"], want["mmd2_unbiased"], want["p_value"], want["gamma"]]
    got = np.loadtxt(out)
    assert np.array_equal(got[:, 0], want["nodes"]) and np.array_equal(got[:, 1], np.arange(len(got)) >= want["m"])
    assert np.array_equal(got[:, 2].astype(np.float32), want["witness"])                # %.9g: f32 exactly
    r = subprocess.run(args, cwd=str(tmp_path), env=dict(env, GCN_MMD_PERMS="40", GCN_MMD_GAMMA=repr(want["gamma"])), capture_output=True, text=True)
    fields = dict(p.split("=") for p in r.stdout.strip().splitlines()[-1].split())
    assert float(fields["mmd2"]) == want["mmd2_biased"] and 1 / 41 <= float(fields["p"]) <= 1
    bad = subprocess.run(args, cwd=str(tmp_path), env=dict(env, GCN_MMD_SPLITS="3,3"), capture_output=True, text=True)
    assert bad.returncode != 0 and "GCN_MMD needs GCN_MMD_SPLITS" in bad.stderr
