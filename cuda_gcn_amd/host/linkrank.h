// linkrank.h — the link prediction metrics out of the integer counts of a rank query (csrc/linkrank.hip): the one place MRR, the mean
// rank and Hits@K are derived.  Host only, no GPU.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

struct LinkRankMetrics {
    int64_t queries = 0, invalid = 0;             // counted (both counts >= 0); left out (a count below 0: an end outside the table)
    double mrr = 0, mean_rank = 0;
};

// rank_i = 1 + above_i + equal_i / 2 (the realistic rank of OGB and PyKEEN); mrr = mean of 1 / rank, hits[j] = the share of queries
// with rank <= ks[j]; float64 sums in list order; no query: zeros, never NaN.  rank (may be NULL) [n]: NaN for a query left out.
// -1 with *err: n < 0, a NULL array, a k below 1.
inline int gcn_link_rank_metrics(const int32_t *above, const int32_t *equal, int64_t n, const int *ks, int n_ks, double *rank, double *hits,
                                 LinkRankMetrics *out, std::string *err) {
    if (n < 0 || n_ks < 0 || !out || (n > 0 && (!above || !equal)) || (n_ks > 0 && (!ks || !hits))) {
        if (err) *err = "link_rank_metrics: invalid argument";
        return -1;
    }
    for (int j = 0; j < n_ks; j++) {
        if (ks[j] < 1) {
            if (err) *err = "link_rank_metrics: every k of Hits@K is at least 1, got " + std::to_string(ks[j]);
            return -1;
        }
        hits[j] = 0;
    }
    LinkRankMetrics r;
    double inv_sum = 0, rank_sum = 0;
    for (int64_t i = 0; i < n; i++) {
        if (above[i] < 0 || equal[i] < 0) {
            r.invalid++;
            if (rank) rank[i] = NAN;
            continue;
        }
        const double rk = 1.0 + (double)above[i] + 0.5 * (double)equal[i];
        if (rank) rank[i] = rk;
        r.queries++;
        inv_sum += 1.0 / rk;
        rank_sum += rk;
        for (int j = 0; j < n_ks; j++) hits[j] += rk <= (double)ks[j] ? 1.0 : 0.0;
    }
    if (r.queries > 0) {
        r.mrr = inv_sum / (double)r.queries;
        r.mean_rank = rank_sum / (double)r.queries;
        for (int j = 0; j < n_ks; j++) hits[j] /= (double)r.queries;
    }
    *out = r;
    return 0;
}
