// thresholds.h — the thresholds file of a multi-label model: one decision cut per class, as ModelQueries::tune_thresholds fits
// them (csrc/thresholds.hip has the rule and the fit) and predict_multilabel / evaluate take them.  Host only, no GPU: the Python
// binding (read_thresholds / write_thresholds) and gcn-hip's GCN_THRESHOLDS / GCN_APPLY_THRESHOLDS both call it.
//
// Format: text, one line per class in class order.  The first token of a line is the threshold, written as %.9g (nine
// significant digits give every float32 back exactly; inf and -inf are written as such); everything from '#' on is ignored, and
// so are lines that hold nothing else.  The writer appends `# class c pos P neg N tp .. fp .. fn .. f ..` when it is given the fit.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

// what a fit knows of its classes, for the comments of the file; any pointer may be NULL (then no comment is written)
struct ThresholdFit {
    const int64_t *pos = nullptr, *neg = nullptr, *tp = nullptr, *fp = nullptr, *fn = nullptr;
    const double *f = nullptr;
};
// num_classes > 0: the file must hold that many thresholds; else the count is taken from the file.  A token that is not a number,
// a NaN, more than one token in front of the '#', no threshold at all or a wrong count is refused with the line named.
// 0, or -1 with the reason in *err.
int gcn_thresholds_read(const char *path, int num_classes, std::vector<float> &out, std::string *err);
int gcn_thresholds_write(const char *path, int num_classes, const float *thr, const ThresholdFit *fit, std::string *err);
