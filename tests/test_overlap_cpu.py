"""What of neighbourhood overlap needs no GPU: the Python sets of tests/overlap_ref.py against scipy, the measures of
host/overlap.h (through the C entry points and, under the sanitizers, a program of their own), the report file, the refusals."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from cuda_gcn_amd import model as M
from tests import overlap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_triangles_are_scipys():
    """on a symmetric simple graph t2 = the row sums of (A @ A) * A, and c(v) = t2 / (d (d - 1))"""
    rng = np.random.default_rng(4)
    a = np.triu(rng.random((200, 200)) < 0.08, 1)
    a = sp.csr_matrix((a | a.T).astype(np.int64))
    t2, deg, tot, skipped = R.rows(R.sets(a.indptr, a.indices))
    want = np.asarray((a @ a).multiply(a).sum(1)).ravel()
    assert np.array_equal(t2, want) and np.array_equal(deg, np.diff(a.indptr)) and skipped == 0 and tot[4] == want.sum() and tot[4] % 6 == 0
    got = M.overlap_metrics(tot, t2, deg)
    d = np.diff(a.indptr).astype(np.float64)
    assert np.array_equal(got["clustering"], np.divide(want, d * (d - 1), out=np.zeros(200), where=d >= 2))
    assert (got["triangles"], got["transitivity"], got["avg_clustering"]) == R.metrics(tot)
    assert abs(got["avg_clustering"] - got["clustering"].mean()) <= 2.0 ** -32


def test_the_reference_drops_repeats_self_entries_and_entries_outside():
    S = R.sets([0, 5, 7, 7], [1, 1, 0, 3, 2, 0, 0])
    assert S == [{1, 2}, {0}, set()]
    assert R.rows(S, [0, 0, -1, 3, 2]) == ([1 - 1, 0, 0, 0, 0], [2, 2, 0, 0, 0], [3, 2, 4, 4, 0, 0, 2, 0], 2)
    assert R.pairs(S, [0, 0, 5], [1, 0, 0], [7, 8, 9]) == ([0, 2, 0], [3, 2, 0], [0, 17, 0], 1)


def test_zero_denominators_give_zero():
    got = M.overlap_metrics(np.zeros(8, np.int64), [0, 0, 5], [0, 1, 1])
    assert got == dict(triangles=0, transitivity=0.0, avg_clustering=0.0, clustering=got["clustering"]) and not got["clustering"].any()
    assert M.overlap_metrics([3, 0, 3, 0, 0, 0, 1, 0]) == dict(triangles=0, transitivity=0.0, avg_clustering=0.0)


def test_refusals():
    for bad in ([1] * 7, [1, 0, -1, 0, 0, 0, 0, 0], [1, 2, 0, 0, 0, 0, 0, 0], [1, 1, 2, 2, 3, 0, 0, 0]):
        with pytest.raises(M.GcnHostError):
            M.overlap_metrics(bad)
    with pytest.raises(M.GcnHostError):
        M.overlap_metrics(np.zeros(8, np.int64), [1], None)
    with pytest.raises(M.GcnHostError):
        M.overlap_metrics(np.zeros(8, np.int64), [1, -1], [2, 2])
    with pytest.raises(M.GcnHostError, match="cannot open"):
        M.read_triangles("/nonexistent/t.txt")


def test_report_file_round_trips(tmp_path):
    node, deg, t2 = np.array([4, 9, 9, 11]), np.array([0, 1, 3, 200]), np.array([0, 0, 4, 39800 - 2])
    tot = [4, 2, 204, 6 + 39800, 39802, 39798, 200, ((4 << 32) // 6) + ((39798 << 32) // 39800)]
    path = tmp_path / "t.txt"
    M.write_triangles(path, node, deg, t2, tot)
    got = M.read_triangles(path)
    assert np.array_equal(got["node"], node) and np.array_equal(got["deg"], deg) and np.array_equal(got["t2"], t2) and got["totals"].tolist() == tot
    assert np.array_equal(got["clustering"], [0, 0, 4 / 6, 39798 / 39800]) and got["triangles"] == 39802 // 6
    lines = open(path).read().splitlines()
    assert lines[0] == "gcn-triangles 1 rows 4" and lines[-1].split()[:3] == ["11", "200", "39798"]


def test_host_overlap_under_the_sanitizers(tmp_path):
    """the ratio near 2^47, the metrics, the weights and the report, in a program of their own under ASan + UBSan"""
    exe = str(tmp_path / "overlap_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "overlap_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "overlap_check ok" in r.stdout, r.stderr[-2000:]


def test_ratio_sum_is_the_python_floor_sum_near_2_to_the_47(tmp_path):
    """floor(t2 . 2^32 / D) by two 16-bit division steps, as the kernel and host/overlap.h form it, against Python integers"""
    src = tmp_path / "ratio.cpp"
    src.write_text('#include "%s"\n#include <cstdlib>\nint main(int c, char **v) { for (int i = 1; i + 1 < c; i += 2) '
                   'printf("%%llu\\n", (unsigned long long)gcn_overlap_ratio(strtoull(v[i], 0, 10), strtoull(v[i + 1], 0, 10))); }\n'
                   % os.path.join(ROOT, "cuda_gcn_amd", "host", "overlap.h"))
    exe = str(tmp_path / "ratio")
    subprocess.run(["g++", "-std=c++17", "-O1", str(src), "-o", exe], check=True)
    rng = np.random.default_rng(8)
    cases = [(d * (d - 1) - k, d * (d - 1)) for d in (2, 3, 11585, (1 << 24) - 1, (1 << 24) - 7) for k in (0, 1, 2)]
    cases += [(int(t), int(D)) for D in rng.integers(1 << 46, 1 << 48, 40) for t in rng.integers(0, D, 2)]
    out = subprocess.run([exe] + [str(x) for c in cases for x in c], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [(t << 32) // D for t, D in cases]
    assert sum(int(x) for x in out) == sum((t << 32) // D for t, D in cases)

