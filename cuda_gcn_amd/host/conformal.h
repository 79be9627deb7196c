// conformal.h — the quantile rule of split conformal prediction (beyond the reference).  Host only: no GPU.  The ONE place where
// calibration scores become a threshold: ModelQueries::conformal_fit and the Python binding (conformal_quantile) both call it.
//
// Scores are conformity scores of the TRUE class, never negative; a negative entry marks a row without a usable label
// (gcnhip_conformal_true_scores writes -1 there) and is dropped.  With n' entries left:
//   k = (int64) ceil((n' + 1) . (1 - alpha)),  evaluated in double — alpha is a double everywhere —,
//   q = the k-th smallest score (std::nth_element),  or +inf when k > n' (too few rows for this alpha: the set is every class).
// Then at least k of the n' scores are <= q, which is the finite-sample guarantee: a fresh exchangeable row's true class is in
// {j : score_j <= q} with probability >= 1 - alpha.  The per-class form (class-conditional coverage) groups the scores by label
// and applies the rule to every group; a label outside [0, C) is dropped like a negative score.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

// the rank of the order statistic for n kept scores
inline int64_t gcn_conformal_k(int64_t n, double alpha) { return (int64_t)std::ceil((double)(n + 1) * (1.0 - alpha)); }

// the k-th smallest of the kept scores (reorders `kept`), +inf when there are fewer than k
inline float gcn_conformal_kth(std::vector<float> &kept, double alpha, int64_t *k_out) {
    const int64_t n = (int64_t)kept.size(), k = gcn_conformal_k(n, alpha);
    if (k_out) *k_out = k;
    if (k > n) return std::numeric_limits<float>::infinity();
    std::nth_element(kept.begin(), kept.begin() + (k - 1), kept.end());
    return kept[k - 1];
}

// 0, or -1 with the reason in *err (alpha outside (0, 1), n < 0, a NaN score, num_classes outside 1..64 with labels).
// labels == NULL: thresh[0], n_cal[0], k[0] of all kept scores.  labels != NULL: thresh / n_cal / k [num_classes], scores grouped
// by labels[i].  n_cal and k may be NULL.
inline int gcn_conformal_quantile(const float *scores, int64_t n, double alpha, const int32_t *labels, int num_classes, float *thresh, int64_t *n_cal,
                                  int64_t *k, std::string *err) {
    auto fail = [&](const char *why) { if (err) *err = std::string("conformal_quantile: ") + why; return -1; };
    if (n < 0 || (n > 0 && !scores) || !thresh) return fail("invalid argument");
    if (!(alpha > 0.0 && alpha < 1.0)) return fail("alpha must be in (0, 1)");
    if (labels && (num_classes < 1 || num_classes > 64)) return fail("1 <= num_classes <= 64");
    const int groups = labels ? num_classes : 1;
    std::vector<std::vector<float>> kept(groups);
    for (int64_t i = 0; i < n; i++) {
        if (std::isnan(scores[i])) return fail("a score is NaN");
        if (scores[i] < 0.f) continue;
        if (!labels) kept[0].push_back(scores[i]);
        else if (labels[i] >= 0 && labels[i] < num_classes) kept[labels[i]].push_back(scores[i]);
    }
    for (int g = 0; g < groups; g++) {
        if (n_cal) n_cal[g] = (int64_t)kept[g].size();
        thresh[g] = gcn_conformal_kth(kept[g], alpha, k ? k + g : nullptr);
    }
    return 0;
}
