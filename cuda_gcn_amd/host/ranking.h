// ranking.h — per-class ROC-AUC and average precision from the integers and sums ModelQueries::ranking forms on the GPU (beyond
// the reference, which reports one accuracy per split).  Host only: no GPU.  The ONE place where the two metrics are derived:
// the Python binding (ranking_report) and gcn-hip's GCN_RANKING both call it.
//
// Per class, with P positives and N negatives among the scored rows:
//   u2     = sum over positives of #{negatives scored lower} + #{negatives scored not higher}   (an exact integer)
//   auc    = u2 / (2 P N)         — the Mann-Whitney statistic with mid-rank ties; one float64 division of two exact integers
//   ap     = ap_sum / P           — ap_sum = sum over positives of TP_ge / (TP_ge + FP_ge), thresholds grouped by distinct score
// A class with P = 0 or N = 0 has no AUC, one with P = 0 no AP: the value is 0 — never NaN, report.h's rule — and its `defined`
// flag is clear.  The macro averages run over the defined classes only (the OGB evaluator's convention), the weighted ones
// weigh a defined class by its positives; without a defined class they are 0.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

struct RankingReport {
    std::vector<double> auc, ap;
    std::vector<int32_t> auc_defined, ap_defined;
    double macro_auc = 0, macro_ap = 0, weighted_auc = 0, weighted_ap = 0;
    int classes_defined = 0;        // classes with an AUC
};

// 0, or -1 with the reason in *err: C < 1, a missing array, a negative count, u2 < 0 or u2 > 2 P N, an ap_sum that is NaN,
// negative or above P.
int gcn_ranking_report(int C, const int64_t *u2, const double *ap_sum, const int64_t *pos, const int64_t *neg, RankingReport *out, std::string *err);
// The text report gcn-hip writes for GCN_RANKING: one line per class `class <c> pos <P> neg <N> auc <a> ap <p>` with `undefined`
// in place of a value that is not defined, then `macro_auc <x> macro_ap <y> weighted_auc <u> weighted_ap <v> classes <k>`.
int gcn_ranking_report_write(const char *path, int C, const RankingReport &rep, const int64_t *pos, const int64_t *neg, std::string *err);
