// thresholds.cpp — multi-label decision thresholds: the thresholds file of thresholds.h (host only) and
// ModelQueries::tune_thresholds on a built HipGCN, between passes (queries.h has the contract, csrc/thresholds.hip the kernels and
// the formulas).  Off the epoch path.
#include "thresholds.h"
#include "queries.h"
#include "gcn.h"
#include "hip_check.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

int gcn_thresholds_read(const char *path, int num_classes, std::vector<float> &out, std::string *err) {
    auto fail = [&](const std::string &m) { if (err) *err = std::string(path ? path : "(null)") + ": " + m; return -1; };
    FILE *f = path ? fopen(path, "r") : nullptr;
    if (!f) return fail("cannot open the thresholds file");
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
        tok = tok.substr(0, tok.find('#'));
        const size_t a = tok.find_first_not_of(" \t\r"), b = tok.find_last_not_of(" \t\r");
        if (a == std::string::npos) continue;                  // a comment or an empty line
        tok = tok.substr(a, b - a + 1);
        char *end = nullptr;
        const float v = strtof(tok.c_str(), &end);
        if (end == tok.c_str() || *end != 0) return fail("line " + std::to_string(line) + ": '" + tok + "' is not one number");
        if (std::isnan(v)) return fail("line " + std::to_string(line) + ": the threshold is NaN");
        out.push_back(v);
    }
    if (out.empty()) return fail("no thresholds in the file");
    if (num_classes > 0 && (int)out.size() != num_classes)
        return fail(std::to_string(out.size()) + " thresholds for " + std::to_string(num_classes) + " classes (one per line)");
    return 0;
}

int gcn_thresholds_write(const char *path, int num_classes, const float *thr, const ThresholdFit *fit, std::string *err) {
    auto fail = [&](const std::string &m) { if (err) *err = std::string(path ? path : "(null)") + ": " + m; return -1; };
    if (!path || !thr || num_classes < 1) return fail("thresholds_write: invalid argument");
    for (int c = 0; c < num_classes; c++)
        if (std::isnan(thr[c])) return fail("the threshold of class " + std::to_string(c) + " is NaN");
    const bool notes = fit && fit->pos && fit->neg && fit->tp && fit->fp && fit->fn && fit->f;
    FILE *f = fopen(path, "w");
    bool ok = f != nullptr;
    for (int c = 0; ok && c < num_classes; c++) {
        ok = fprintf(f, "%.9g", (double)thr[c]) > 0;
        if (ok && notes)
            ok = fprintf(f, " # class %d pos %lld neg %lld tp %lld fp %lld fn %lld f %.9f", c, (long long)fit->pos[c], (long long)fit->neg[c],
                         (long long)fit->tp[c], (long long)fit->fp[c], (long long)fit->fn[c], fit->f[c]) > 0;
        if (ok) ok = fputc('\n', f) != EOF;
    }
    if (f && fclose(f) != 0) ok = false;
    return ok ? 0 : fail("could not write the thresholds file");
}

int64_t ModelQueries::tune_thresholds(int split, const int *nodes, int n, double beta, size_t scratch_bytes, float *thr, int64_t *tp, int64_t *fp,
                                      int64_t *fn, double *f, int64_t *pos, int64_t *neg, int64_t *invalid, int32_t *defined) {
    const int C = m.params.output_dim;
    require("tune_thresholds", MULTI_LABEL | CLASS_AGGREGATION | ONE_RANK | AT_MOST_256);
    if (split < 0 || split > 3 || n < 0 || !thr || !tp || !fp || !fn || !f || !pos || !neg || !invalid || !defined)
        throw GcnHipFailure(-1, "tune_thresholds: invalid argument (split is 0 with a node query, or 1 train, 2 validation, 3 test)");
    if (!std::isfinite(beta) || !(beta > 0.0)) throw GcnHipFailure(-1, "tune_thresholds: beta must be finite and > 0");
    if ((!split && nodes ? n : m.n_local) > RANKING_ROWS_MAX) throw GcnHipFailure(-1, "tune_thresholds: at most 2^24 listed rows");
    const ScoredRows q = scored_rows("tune_thresholds", split, nodes, n);
    n = q.n;
    forward_redirect(q.subset);                                // the logits, scored as they are: ranking()'s table on a multi-label model
    // one block, one download: f [C] (float64) | thr [C] | {TP | FP | FN} [3 S] per batch, back to back | defined [C]
    const size_t words = 5 * (size_t)C;
    double *d_f = d_th_fit.need((size_t)C + (words + 1) / 2);
    float *d_thr = (float *)(d_f + C);
    int32_t *d_cnt = (int32_t *)(d_thr + C);
    std::vector<int> batch_of((size_t)C), batch_size((size_t)C);
    const int32_t *d_counts = sorted_class_batches(q, d_ml_logits.p, m.variables[6]->ld, scratch_bytes, [&](int c0, int S, const uint32_t *pos_keys,
                                                                                                             const uint32_t *neg_keys, int64_t stride,
                                                                                                             const int32_t *d_pos, const int32_t *d_neg,
                                                                                                             void *d_work) {
        GCNHIP_CHECK(gcnhip_threshold_scan(m.env.ctx, pos_keys, neg_keys, stride, n, S, d_pos, d_neg, beta, d_work, d_thr + c0, d_cnt + 3 * (size_t)c0, d_f + c0,
                                           d_cnt + 3 * (size_t)C + c0));
        for (int c = c0; c < c0 + S; c++) { batch_of[c] = c0; batch_size[c] = S; }
    });
    std::vector<int32_t> hc(3 * (size_t)C);
    std::vector<double> hfit((size_t)C + (words + 1) / 2);
    GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, hc.data(), d_counts, hc.size() * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, hfit.data(), d_f, hfit.size() * sizeof(double)));
    m.sync();
    const double *hf = hfit.data();
    const float *hthr = (const float *)(hf + C);
    const int32_t *ht = (const int32_t *)(hthr + C);
    for (int c = 0; c < C; c++) {
        const int32_t *b = ht + 3 * (size_t)batch_of[c];
        const int j = c - batch_of[c], S = batch_size[c];
        thr[c] = hthr[c]; f[c] = hf[c]; defined[c] = ht[3 * (size_t)C + c];
        tp[c] = b[j]; fp[c] = b[S + j]; fn[c] = b[2 * S + j];
        pos[c] = hc[c]; neg[c] = hc[C + c]; invalid[c] = hc[2 * C + c];
    }
    return n;
}
