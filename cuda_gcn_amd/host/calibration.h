// calibration.h — the reliability diagram and its summary from per-bin integer counts and confidence sums (beyond the
// reference).  Host only: no GPU.  The ONE place where (count, correct, conf_sum) become a report: ModelQueries::calibration's
// callers (the Python binding, gcn-hip's GCN_CALIBRATE) hand it what gcnhip_calib_bins_rows formed.
//
// Bin b holds the rows whose confidence (largest softmax probability) lies in (b / B, (b + 1) / B] (Guo et al., 2017).
//   accuracy[b]   = correct[b] / count[b]      confidence[b] = conf_sum[b] / count[b]      (both 0 for an empty bin)
//   ECE = sum_b (count[b] / rows) |accuracy[b] - confidence[b]|       MCE = max over non-empty bins of |accuracy[b] - confidence[b]|
// Everything is float64 arithmetic; no rows at all gives 0 everywhere — never NaN.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

struct CalibrationReport {
    std::vector<double> accuracy, confidence;
    double ece = 0, mce = 0;
    int64_t rows = 0;
};

// 0, or -1 with the reason in *err (bins < 1, a negative count, correct above count, a negative or non-finite confidence sum)
inline int gcn_calibration_report(int bins, const int64_t *count, const int64_t *correct, const double *conf_sum, CalibrationReport *out,
                                  std::string *err) {
    auto fail = [&](const char *why) { if (err) *err = std::string("calibration_report: ") + why; return -1; };
    if (bins < 1 || !count || !correct || !conf_sum || !out) return fail("invalid argument (bins >= 1, three arrays of that length)");
    CalibrationReport r;
    r.accuracy.assign(bins, 0.0);
    r.confidence.assign(bins, 0.0);
    for (int b = 0; b < bins; b++) {
        if (count[b] < 0 || correct[b] < 0 || correct[b] > count[b]) return fail("a bin needs 0 <= correct <= count");
        if (!(conf_sum[b] >= 0.0) || !std::isfinite(conf_sum[b])) return fail("a confidence sum is negative or not finite");
        r.rows += count[b];
    }
    for (int b = 0; b < bins; b++) {
        if (!count[b]) continue;
        r.accuracy[b] = (double)correct[b] / (double)count[b];
        r.confidence[b] = conf_sum[b] / (double)count[b];
        const double gap = std::fabs(r.accuracy[b] - r.confidence[b]);
        r.ece += (double)count[b] / (double)r.rows * gap;
        if (gap > r.mce) r.mce = gap;
    }
    *out = std::move(r);
    return 0;
}

// The table gcn-hip writes for GCN_CALIBRATE, appended to f: a line `temperature <T> rows <n> nll <x> ece <e> mce <m>`, then
// one line per bin `bin <b> lo <b/B> hi <(b+1)/B> count <n> accuracy <a> confidence <c>`.  False when a write failed.
inline bool gcn_calibration_table_write(FILE *f, double temperature, double nll, int bins, const int64_t *count, const CalibrationReport &rep) {
    bool ok = fprintf(f, "temperature %.6g rows %lld nll %.6f ece %.6f mce %.6f\n", temperature, (long long)rep.rows, nll, rep.ece, rep.mce) > 0;
    for (int b = 0; ok && b < bins; b++)
        ok = fprintf(f, "bin %d lo %.6g hi %.6g count %lld accuracy %.6f confidence %.6f\n", b, (double)b / bins, (double)(b + 1) / bins,
                     (long long)count[b], rep.accuracy[b], rep.confidence[b]) > 0;
    return ok;
}
