// class_weights.h — per-class loss weights (beyond the reference, whose loss weighs every row equally).  Host only.
//
// Single-label: w[C] scales the loss term and the gradient row of every node of class c (gcnhip_wxent_fwd_rows; the mean is
// the weighted one).  Multi-label: pos_weight[C] scales the positive term of class c (gcnhip_wbce_fwd_rows).
//  * gcn_class_weights_check: what HipGCN refuses — wrong length, a negative / NaN / infinite weight.
//  * gcn_balanced_class_weights: "balanced" weights from the labelled rows of one split.  Single-label: w_c = n / (C . n_c)
//    (n labelled rows of the split, n_c those of class c; 0 when n_c = 0) — scikit-learn's class_weight="balanced".
//    Multi-label: pw_c = (n - pos_c) / pos_c over the split's rows (1 when pos_c = 0) — the rule PyTorch documents for
//    BCEWithLogitsLoss(pos_weight=).
//  * gcn_class_weights_read: a text file of C lines, one float each (spaces around it allowed, a final newline optional);
//    a wrong line count, a token that is not a number, a negative, NaN or infinite value is refused with the line named.
//  * gcn_class_weight_sum: sum of w[label] over the rows of a split, in float64 — the gradient's divisor of the weighted
//    softmax loss (a row whose label is outside [0, C) has no weight).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

inline int gcn_class_weights_check(const float *w, size_t n, int num_classes, std::string *err) {
    if (n != (size_t)num_classes) {
        if (err) *err = "class weights: " + std::to_string(n) + " weights for " + std::to_string(num_classes) + " classes";
        return -1;
    }
    for (size_t c = 0; c < n; c++)
        if (!std::isfinite(w[c]) || w[c] < 0.f) {
            if (err) *err = "class weights: the weight of class " + std::to_string(c) + " is " + std::to_string(w[c]) + " (it must be finite and not negative)";
            return -1;
        }
    return 0;
}

// label: [num_nodes] (may be NULL when multihot is given); multihot: NULL (single-label) or [num_nodes x ceil(C / 32)] bit rows
inline int gcn_balanced_class_weights(int num_nodes, int num_classes, const int *split, const int *label, const uint32_t *multihot,
                                      int which_split, float *out, std::string *err) {
    if (num_nodes < 0 || num_classes < 1 || !split || !out || (!label && !multihot)) {
        if (err) *err = "balanced class weights: invalid argument";
        return -1;
    }
    std::vector<double> cnt(num_classes, 0.0);
    double n = 0;
    if (multihot) {
        const int wpr = (num_classes + 31) / 32;
        for (int i = 0; i < num_nodes; i++) {
            if (split[i] != which_split) continue;
            n += 1;
            for (int c = 0; c < num_classes; c++) cnt[c] += (multihot[(size_t)i * wpr + (c >> 5)] >> (c & 31)) & 1u;
        }
        for (int c = 0; c < num_classes; c++) out[c] = cnt[c] > 0 ? (float)((n - cnt[c]) / cnt[c]) : 1.f;
        return 0;
    }
    for (int i = 0; i < num_nodes; i++) {
        if (split[i] != which_split || label[i] < 0 || label[i] >= num_classes) continue;
        n += 1;
        cnt[label[i]] += 1;
    }
    for (int c = 0; c < num_classes; c++) out[c] = cnt[c] > 0 ? (float)(n / ((double)num_classes * cnt[c])) : 0.f;
    return 0;
}

inline double gcn_class_weight_sum(int num_nodes, int num_classes, const int *split, const int *label, int which_split, const float *w) {
    double s = 0;
    for (int i = 0; i < num_nodes; i++)
        if (split[i] == which_split && label[i] >= 0 && label[i] < num_classes) s += (double)w[label[i]];
    return s;
}

// num_classes > 0: the file must have that many lines; else the count is taken from the file.  0, or -1 with the reason.
inline int gcn_class_weights_read(const char *path, int num_classes, std::vector<float> &out, std::string *err) {
    auto fail = [&](const std::string &m) { if (err) *err = std::string(path ? path : "(null)") + ": " + m; return -1; };
    FILE *f = path ? fopen(path, "r") : nullptr;
    if (!f) return fail("cannot open the class weights file");
    std::string text;
    char buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    fclose(f);
    out.clear();
    size_t pos = 0;
    int line = 0;
    while (pos < text.size()) {
        size_t nl = text.find('\n', pos);
        if (nl == std::string::npos) nl = text.size();
        std::string tok = text.substr(pos, nl - pos);
        pos = nl + 1;
        line++;
        const size_t a = tok.find_first_not_of(" \t\r"), b = tok.find_last_not_of(" \t\r");
        if (a == std::string::npos) return fail("line " + std::to_string(line) + ": empty (one weight per line)");
        tok = tok.substr(a, b - a + 1);
        char *end = nullptr;
        const float v = strtof(tok.c_str(), &end);
        if (end == tok.c_str() || *end != 0) return fail("line " + std::to_string(line) + ": '" + tok + "' is not a number");
        if (!std::isfinite(v) || v < 0.f) return fail("line " + std::to_string(line) + ": the weight '" + tok + "' must be finite and not negative");
        out.push_back(v);
    }
    if (out.empty()) return fail("no weights in the file");
    if (num_classes > 0 && (int)out.size() != num_classes)
        return fail(std::to_string(out.size()) + " lines for " + std::to_string(num_classes) + " classes (one weight per line)");
    return 0;
}
