// kmeans.h — the scores of a clustering against class labels, from the integer cluster x class table (beyond the reference).
// Host only: no GPU.  The ONE place where a contingency table becomes a report: ModelQueries::kmeans's callers (the Python
// binding, gcn-hip's GCN_CLUSTER) hand it what gcnhip_contingency_rows counted.  (host/cluster.h is the schedule's graph grouping.)
//
// counts [k x C], counts[a * C + y] = rows of cluster a with class y; a_a = row sums, b_y = column sums, N = their total.
//   purity        = sum_a max_y counts[a, y] / N
//   H(classes)    = -sum_y (b_y / N) (log b_y - log N)        H(clusters) likewise over a_a        (natural logarithm)
//   MI            = sum over non-zero cells of (n / N) ((log n - log a_a) + (log N - log b_y))
//   homogeneity   = MI / H(classes), 1 when H(classes) = 0;  completeness = MI / H(clusters), 1 when H(clusters) = 0
//   V-measure     = 2 h c / (h + c), 0 when h + c = 0         (Rosenberg & Hirschberg, 2007)
//   NMI           = MI / ((H(classes) + H(clusters)) / 2): the arithmetic-mean normalisation; 1 when both entropies are 0 (one
//                   cluster and one class: a perfect match), 0 when MI = 0 otherwise
//   ARI           = 2 (tp tn - fn fp) / ((tp + fn)(fn + tn) + (tp + fp)(fp + tn)) over the pairs of rows (Hubert & Arabie, 1985),
//                   tp = sum n^2 - N, fp = sum a^2 - sum n^2, fn = sum b^2 - sum n^2, tn = N^2 - N - tp - fp - fn (each counts
//                   ordered pairs); 1 when fp = fn = 0.  The products are formed in 128-bit integers.
// Empty rows and columns are allowed.  Everything else is float64 arithmetic; no rows at all gives purity 0, the other scores
// their perfect-match value and both entropies 0 — never NaN.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

struct ClusterReport {
    double purity = 0, homogeneity = 1, completeness = 1, v_measure = 1, nmi = 1, ari = 1, entropy_classes = 0, entropy_clusters = 0;
    int64_t rows = 0;
};

// 0, or -1 with the reason in *err (k or C below 1, a negative count, more than 2^31 rows)
inline int gcn_cluster_report(int k, int C, const int64_t *counts, ClusterReport *out, std::string *err) {
    auto fail = [&](const char *why) { if (err) *err = std::string("cluster_report: ") + why; return -1; };
    if (k < 1 || C < 1 || !counts || !out) return fail("invalid argument (a table of k >= 1 clusters by C >= 1 classes)");
    std::vector<int64_t> a((size_t)k, 0), b((size_t)C, 0);
    int64_t N = 0, best = 0;
    for (int i = 0; i < k; i++) {
        int64_t top = 0;
        for (int y = 0; y < C; y++) {
            const int64_t n = counts[(size_t)i * C + y];
            if (n < 0) return fail("a negative count");
            a[i] += n;
            b[y] += n;
            N += n;
            if (N > ((int64_t)1 << 31)) return fail("more than 2^31 rows");
            if (n > top) top = n;
        }
        best += top;
    }
    ClusterReport r;
    r.rows = N;
    if (N == 0) { *out = r; return 0; }
    const double dN = (double)N, logN = std::log(dN);
    r.purity = (double)best / dN;
    for (int y = 0; y < C; y++)
        if (b[y]) r.entropy_classes -= (double)b[y] / dN * (std::log((double)b[y]) - logN);
    for (int i = 0; i < k; i++)
        if (a[i]) r.entropy_clusters -= (double)a[i] / dN * (std::log((double)a[i]) - logN);
    if (r.entropy_classes < 0) r.entropy_classes = 0;           // -0.0 of a single class
    if (r.entropy_clusters < 0) r.entropy_clusters = 0;
    double mi = 0;
    __int128 sum_sq = 0, sum_a = 0, sum_b = 0;
    for (int i = 0; i < k; i++) {
        sum_a += (__int128)a[i] * a[i];
        for (int y = 0; y < C; y++) {
            const int64_t n = counts[(size_t)i * C + y];
            if (!n) continue;
            sum_sq += (__int128)n * n;
            mi += (double)n / dN * ((std::log((double)n) - std::log((double)a[i])) + (logN - std::log((double)b[y])));
        }
    }
    for (int y = 0; y < C; y++) sum_b += (__int128)b[y] * b[y];
    if (mi < 0) mi = 0;
    const double hc = r.entropy_classes, hk = r.entropy_clusters;
    r.homogeneity = hc > 0 ? mi / hc : 1.0;
    r.completeness = hk > 0 ? mi / hk : 1.0;
    r.v_measure = r.homogeneity + r.completeness > 0 ? 2.0 * r.homogeneity * r.completeness / (r.homogeneity + r.completeness) : 0.0;
    r.nmi = hc == 0 && hk == 0 ? 1.0 : (mi == 0 ? 0.0 : mi / ((hc + hk) / 2.0));
    const __int128 tp = sum_sq - N, fp = sum_a - sum_sq, fn = sum_b - sum_sq, tn = (__int128)N * N - N - tp - fp - fn;
    if (fp == 0 && fn == 0) r.ari = 1.0;
    else r.ari = 2.0 * (double)(tp * tn - fn * fp) / (double)((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn));   // N <= 2^31: below 2^126
    *out = r;
    return 0;
}
