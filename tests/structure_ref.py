"""The definitions of csrc/structure.hip in numpy and Python integers, and the measures of host/structure.h derived from the counts
independently in float64.  Shared by tests/test_structure_cpu.py and tests/test_structure_gpu.py.

A graph is (indptr, indices) with stored rows as the loader made them (self loop included, repeats counted, one-way entries
allowed); lab has one entry per column; label x is known when 0 <= x < C.  A query is a list of rows (None: position i is row i for
i < n); a position whose row is outside [0, n_rows) counts in `skipped` and nowhere else."""
import numpy as np

TWO32 = 1 << 32


def agreement(indptr, indices, lab, C, rows=None, n=None):
    """dict(deg, same, known int32 [n], mix int64 [C, C], class_rows int64 [C], totals int64 [8], skipped) by the definitions"""
    indptr, indices, lab = np.asarray(indptr, np.int64), np.asarray(indices, np.int64), np.asarray(lab, np.int64)
    n_rows = indptr.size - 1
    rows = np.arange(n_rows if n is None else n, dtype=np.int64) if rows is None else np.asarray(rows, np.int64).ravel()
    n = rows.size
    deg, same, known = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    mix, class_rows = np.zeros((C, C), np.int64), np.zeros(C, np.int64)
    in_range = labelled = with_known = self_seen = skipped = 0
    ratio_sum = 0                                              # a Python integer, reduced mod 2^64 at the end
    is_known = (lab >= 0) & (lab < C)
    for i, v in enumerate(rows):
        if v < 0 or v >= n_rows:
            skipped += 1
            continue
        in_range += 1
        u = indices[indptr[v]:indptr[v + 1]]
        self_seen += int((u == v).sum())
        u = u[u != v]
        deg[i] = u.size
        if not (v < lab.size and is_known[v]):
            continue
        labelled += 1
        class_rows[lab[v]] += 1
        lu = lab[u][is_known[u]]
        known[i] = lu.size
        same[i] = int((lu == lab[v]).sum())
        np.add.at(mix[lab[v]], lu, 1)
        if known[i] > 0:
            with_known += 1
            ratio_sum += (int(same[i]) * TWO32) // int(known[i])
    totals = np.array([in_range, labelled, with_known, int(deg.sum(dtype=np.int64)), int(known.sum(dtype=np.int64)), int(same.sum(dtype=np.int64)),
                       self_seen, 0], np.int64)
    totals[7] = np.array([ratio_sum % (1 << 64)], np.uint64).view(np.int64)[0]
    return dict(deg=deg, same=same, known=known, mix=mix, class_rows=class_rows, totals=totals, skipped=skipped)


def degree_bucket(d):
    return 0 if d <= 0 else int(d).bit_length()                # 1 + floor(log2 d)


def agreement_bucket(same, known, bins):
    return bins if known <= 0 else min(bins - 1, (int(same) * bins) // int(known))


def strata(deg, same, known, pred, truth, C, bins, rows=None):
    """(strata int64 [32, bins + 1, 2], unlabelled): pred and truth by row, deg / same / known by list position"""
    pred, truth = np.asarray(pred, np.int64), np.asarray(truth, np.int64)
    n = len(deg)
    rows = np.arange(n, dtype=np.int64) if rows is None else np.asarray(rows, np.int64).ravel()
    out = np.zeros((32, bins + 1, 2), np.int64)
    unlabelled = 0
    for i, r in enumerate(rows):
        if r < 0 or r >= truth.size:
            continue
        y = truth[r]
        if not 0 <= y < C:
            unlabelled += 1
            continue
        k = int(known[i])
        s = min(max(int(same[i]), 0), max(k, 0))
        cell = out[degree_bucket(int(deg[i])), agreement_bucket(s, k, bins)]
        cell[0] += 1
        cell[1] += int(pred[r] == y)
    return out, unlabelled


def metrics(mix, class_rows, totals=None, strata=None):
    """host/structure.h's measures from the formulas of the issue, in float64 on Python integers; a zero denominator gives 0"""
    mix = [[int(x) for x in row] for row in np.asarray(mix)]
    rows_c = [int(x) for x in np.asarray(class_rows)]
    C = len(mix)
    div = lambda a, b: float(a) / float(b) if b else 0.0
    r = [sum(row) for row in mix]
    E, R = sum(r), sum(rows_c)
    out = dict(edge_homophily=div(sum(mix[k][k] for k in range(C)), E),
               class_homophily=np.array([div(mix[k][k], r[k]) for k in range(C)]),
               compatibility=np.array([[div(mix[a][b], r[a]) for b in range(C)] for a in range(C)]).reshape(C, C),
               edges=E, labelled_rows=R)
    out["class_insensitive_homophily"] = sum(max(0.0, out["class_homophily"][k] - div(rows_c[k], R)) for k in range(C)) / (C - 1) if C > 1 else 0.0
    p2 = sum(div(r[k], E) ** 2 for k in range(C))
    out["adjusted_homophily"] = (out["edge_homophily"] - p2) / (1.0 - p2) if E and 1.0 - p2 > 0 else 0.0
    out["node_homophily"], out["rows_with_known"] = 0.0, 0
    if totals is not None:
        t = np.asarray(totals, np.int64)
        out["rows_with_known"] = int(t[2])
        out["node_homophily"] = div(int(t[7:8].view(np.uint64)[0]) / TWO32, int(t[2]))
    if strata is not None:
        s = np.asarray(strata, np.int64)
        bins = s.shape[1] - 1

        def table(counts, bounds):
            return [dict(lo=float(lo), hi=float(hi), rows=int(c[0]), correct=int(c[1]), accuracy=div(int(c[1]), int(c[0]))) for c, (lo, hi) in zip(counts, bounds)]
        out["strata_rows"] = int(s[:, :, 0].sum())
        out["by_degree"] = table(s.sum(axis=1), [(0, 0)] + [(2 ** (b - 1), 2 ** b - 1) for b in range(1, 32)])
        out["by_agreement"] = table(s.sum(axis=0), [(a / bins, (a + 1) / bins) for a in range(bins)] + [(-1, -1)])
    return out


def node_homophily_float(same, known):
    """the float64 mean of same / known over the rows with known > 0"""
    same, known = np.asarray(same, np.float64), np.asarray(known, np.float64)
    m = known > 0
    return float((same[m] / known[m]).mean()) if m.any() else 0.0


def random_labels(rng, n, C, unknown=0.1):
    """labels in [0, C) with a share of unknown ones: -1, C and INT32_MAX in turn"""
    lab = rng.integers(0, C, n).astype(np.int32)
    where = np.flatnonzero(rng.random(n) < unknown)
    lab[where] = np.array([-1, C, np.iinfo(np.int32).max], np.int32)[np.arange(where.size) % 3]
    return lab


def assert_metrics_close(got, want, tol=1e-12):
    for key, w in want.items():
        g = got[key]
        if key in ("by_degree", "by_agreement"):
            assert len(g) == len(w), key
            for a, b in zip(g, w):
                assert a["rows"] == b["rows"] and a["correct"] == b["correct"], (key, a, b)
                assert all(abs(a[f] - b[f]) <= tol for f in ("lo", "hi", "accuracy")), (key, a, b)
        elif isinstance(w, (int, np.integer)):
            assert g == w, (key, g, w)
        else:
            assert np.all(np.isfinite(np.asarray(g))), (key, g)
            assert np.max(np.abs(np.asarray(g, np.float64) - np.asarray(w, np.float64)), initial=0.0) <= tol, (key, g, w)
