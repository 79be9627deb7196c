// report.h — per-class metrics from integer counts (beyond the reference, which reports one accuracy per split).  Host only:
// no GPU.  The ONE place where precision / recall / F1 are derived: ModelQueries::evaluate's callers (the Python binding, gcn-hip's
// GCN_REPORT) hand it the counts the GPU formed.
//
// Everything is float64 arithmetic on integers: each per-class metric is one division of two exactly represented integers
// (counts stay far below 2^53), 0 when its denominator is 0 — never NaN.
//   support   = rows whose truth is the class          (TP + FN)
//   precision = TP / (TP + FP)      recall = TP / (TP + FN)      f1 = 2 TP / (2 TP + FP + FN)
//   macro_f1  = mean of f1 over all C classes, classes without support included (the usual convention with a fixed label set)
//   micro_f1  = 2 sum(TP) / (2 sum(TP) + sum(FP) + sum(FN))
//   accuracy  = trace / rows of the matrix (single-label only, where it equals micro_f1; 0 from TP / FP / FN vectors)
#pragma once
#include <cstdint>
#include <string>
#include <vector>

struct ClassReport {
    std::vector<int64_t> tp, fp, fn;
    std::vector<double> support, precision, recall, f1;
    double macro_f1 = 0, micro_f1 = 0, accuracy = 0;
    int64_t rows = 0;               // rows of the matrix (confusion given), else 0
};

// Either confusion [C x C] (row = truth, column = prediction: TP = the diagonal, FP = column sum - diagonal, FN = row sum -
// diagonal) or the three vectors tp / fp / fn [C].  0, or -1 with the reason in *err (C < 1, a negative count, both or neither
// form given).
int gcn_class_report(int C, const int64_t *confusion, const int64_t *tp, const int64_t *fp, const int64_t *fn, ClassReport *out,
                     std::string *err);
// The text report gcn-hip writes for GCN_REPORT: one line per class `class <c> support <n> precision <p> recall <r> f1 <f>`, a
// line `macro_f1 <x> micro_f1 <y>`, and, when confusion != NULL, a line `confusion` followed by C lines of C integers.
int gcn_class_report_write(const char *path, int C, const ClassReport &rep, const int64_t *confusion, std::string *err);
