// conformal.cpp — ModelQueries::conformal_fit / conformal_sets: split conformal prediction sets on a built HipGCN, between
// passes (queries.h has the contract, csrc/conformal.hip the formulas, conformal.h the quantile rule).  Off the epoch path.
#include "conformal.h"
#include "queries.h"
#include "gcn.h"
#include "hip_check.h"
#include <cmath>
#include <limits>

void ModelQueries::conformal_check(const char *what, int split, int n, double alpha, int method, float lam, int k_reg, float diffusion) const {
    const std::string w = std::string(what) + ": ";
    require(what, SINGLE_LABEL | CLASS_AGGREGATION | AT_MOST_64 | ONE_RANK);
    if (split < 0 || split > 3 || n < 0) throw GcnHipFailure(-1, w + "invalid argument (split is 0 with a node query, or 1 train, 2 validation, 3 test)");
    if (!(alpha > 0.0 && alpha < 1.0)) throw GcnHipFailure(-1, w + "alpha must be in (0, 1)");
    if (method != CONFORMAL_LAC && method != CONFORMAL_APS) throw GcnHipFailure(-1, w + "the method is 0 (lac) or 1 (aps)");
    if (!(lam >= 0.f) || !std::isfinite(lam)) throw GcnHipFailure(-1, w + "lam must be finite and >= 0");
    if (k_reg < 0) throw GcnHipFailure(-1, w + "k_reg must be >= 0");
    if (!(diffusion >= 0.f && diffusion <= 1.f)) throw GcnHipFailure(-1, w + "diffusion must be in [0, 1]");
}

const float *ModelQueries::conformal_table(const ScoredRows &q, int method, float lam, int k_reg, float diffusion, int *ld_out) {
    const int C = m.params.output_dim, n_local = m.n_local, ld = smooth_row_ld(C);
    const bool diffuse = diffusion > 0.f;
    *ld_out = ld;
    float *S = d_cf_table[0].need((size_t)n_local * ld);
    forward_predict(diffuse ? nullptr : q.subset, true);       // the neighbours' scores are needed: then every row
    GCNHIP_CHECK(gcnhip_conformal_scores(m.env.ctx, d_logp.p, C, n_local, diffuse ? nullptr : q.d_list, diffuse ? n_local : q.n, C, 1.f / temperature_,
                                         method, lam, k_reg, S, ld));
    if (!diffuse) return S;
    float *D = d_cf_table[1].need((size_t)n_local * ld);
    const float inf = std::numeric_limits<float>::infinity();
    GCNHIP_CHECK(gcnhip_graphsum_blend(m.env.ctx, m.graph, S, ld, S, ld, D, ld, C, diffusion, 1.f - diffusion, -inf, inf, nullptr));
    return D;
}

ModelQueries::Conformal ModelQueries::conformal_fit(int split, const int *nodes, int n, double alpha, int method, float lam, int k_reg, float diffusion,
                                                    bool per_class, std::vector<float> *scores) {
    conformal_check("conformal_fit", split, n, alpha, method, lam, k_reg, diffusion);
    if (split && m.split_count[split] < 1) throw GcnHipFailure(-1, "conformal_fit: split " + std::to_string(split) + " has no labelled rows to fit on");
    const int C = m.params.output_dim;
    const ScoredRows q = scored_rows("conformal_fit", split, nodes, n);
    int ld = 0;
    const float *table = conformal_table(q, method, lam, k_reg, diffusion, &ld);
    std::vector<float> h((size_t)q.n);
    std::vector<int32_t> label;
    GCNHIP_CHECK(gcnhip_conformal_true_scores(m.env.ctx, table, ld, q.truth, m.n_local, q.d_list, q.n, C, d_cf_score.need((size_t)q.n)));
    if (q.n) GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, h.data(), d_cf_score.p, h.size() * sizeof(float)));
    if (per_class && q.n) {                                    // the label of every list position: the list itself comes back too
        label.resize((size_t)q.n);
        if (q.d_list) GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, label.data(), q.d_list, label.size() * sizeof(int32_t)));
        const int r0 = m.row_start();
        for (int i = 0; i < q.n; i++) {
            const int r = q.d_list ? label[i] : i;
            label[i] = r >= 0 && r < m.n_local ? m.data->label[r0 + r] : -1;
        }
    }
    m.sync();
    Conformal out;
    out.method = method; out.lam = lam; out.k_reg = k_reg; out.diffusion = diffusion; out.temperature = temperature_;
    out.alpha = alpha; out.per_class = per_class;
    std::string err;
    if (gcn_conformal_quantile(h.data(), q.n, alpha, per_class ? label.data() : nullptr, C, out.thresh, out.n_cal, nullptr, &err) != 0)
        throw GcnHipFailure(-1, "conformal_fit: " + err);
    int64_t scored = 0;
    if (per_class) {
        for (int c = 0; c < C; c++) scored += out.n_cal[c];
    } else {
        scored = out.n_cal[0];
        for (int c = 1; c < C; c++) { out.thresh[c] = out.thresh[0]; out.n_cal[c] = out.n_cal[0]; }
    }
    if (scored < 1) throw GcnHipFailure(-1, "conformal_fit: the rows have no labelled rows to fit on");
    if (scores) scores->swap(h);
    return out;
}

void ModelQueries::conformal_sets(const Conformal &fit, int split, const int *nodes, int n, uint32_t *bits, int32_t *size, int64_t *counts) {
    conformal_check("conformal_sets", split, n, fit.alpha, fit.method, fit.lam, fit.k_reg, fit.diffusion);
    const int C = m.params.output_dim, wpr = (C + 31) / 32, cells = 4 + 3 * C + 1;
    for (int c = 0; c < C; c++)
        if (std::isnan(fit.thresh[c])) throw GcnHipFailure(-1, "conformal_sets: the threshold of class " + std::to_string(c) + " is NaN");
    if (fit.temperature != temperature_)
        throw GcnHipFailure(-1, "conformal_sets: the fit was made at temperature " + std::to_string(fit.temperature) + ", the model is at " +
                                    std::to_string(temperature_) + " (the guarantee holds for the scores the threshold was fitted on: fit again)");
    const ScoredRows q = scored_rows("conformal_sets", split, nodes, n);
    int ld = 0;
    const float *table = conformal_table(q, fit.method, fit.lam, fit.k_reg, fit.diffusion, &ld);
    GCNHIP_CHECK(gcnhip_h2d(m.env.ctx, d_cf_thresh.need(64), fit.thresh, (size_t)C * sizeof(float)));
    uint32_t *d_bits = bits ? d_cf_bits.need((size_t)q.n * wpr) : nullptr;
    int32_t *d_size = size ? d_cf_size.need((size_t)q.n) : nullptr;
    int32_t *d_counts = counts ? d_cf_counts.need((size_t)cells) : nullptr;
    GCNHIP_CHECK(gcnhip_conformal_sets_rows(m.env.ctx, table, ld, m.n_local, q.d_list, q.n, C, d_cf_thresh.p, q.truth, d_bits, d_size, d_counts));
    if (bits && q.n) GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, bits, d_bits, (size_t)q.n * wpr * sizeof(uint32_t)));
    if (size && q.n) GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, size, d_size, (size_t)q.n * sizeof(int32_t)));
    if (counts) {
        std::vector<int32_t> h((size_t)cells);
        GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, h.data(), d_counts, h.size() * sizeof(int32_t)));
        std::copy(h.begin(), h.end(), counts);
    }
    m.sync();
}
