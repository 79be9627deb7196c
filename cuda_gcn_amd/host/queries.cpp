// queries.cpp — ModelQueries: prediction, per-class evaluation, label propagation and Correct & Smooth, temperature scaling,
// node embeddings on a built HipGCN, between passes.  Off the epoch path.
#include "queries.h"
#include "gcn.h"
#include "hip_check.h"
#include <algorithm>
#include <cmath>
#include <numeric>

ModelQueries::ModelQueries(HipGCN &model) : m(model) { arena.bind(m.env.ctx); }

void ModelQueries::require(const char *what, int needs) const {
    const std::string w = std::string(what) + ": ";
    const int C = m.params.output_dim;
    if ((needs & SINGLE_LABEL) && m.opt_.multilabel)
        throw GcnHipFailure(-1, w + "this is a multi-label model (the call works on one softmax per node; predict_multilabel and evaluate take such a model)");
    if ((needs & MULTI_LABEL) && !m.opt_.multilabel) throw GcnHipFailure(-1, w + "this is a single-label model: use predict");
    if ((needs & CLASS_AGGREGATION) && !m.logits_gs) throw GcnHipFailure(-1, w + "this model has no class-width aggregation");
    if ((needs & AT_MOST_64) && C > 64) throw GcnHipFailure(-1, w + "at most 64 classes (the row of a node sits in one wave)");
    if ((needs & AT_MOST_256) && C > 256) throw GcnHipFailure(-1, w + "at most 256 classes on a multi-label model");
    if ((needs & ONE_RANK) && m.world() > 1)
        throw GcnHipFailure(-1, w + "one rank only (the tables and the double sums of this call are not exchanged between ranks)");
}

// dataset node ids -> local rows of this rank (HipGCN::node_id undone); NULL: every local row
void ModelQueries::query_rows(const char *what, const int *nodes, int n, std::vector<int> &rows) {
    const int N = m.params.num_nodes;
    rows.resize(n);
    if (!nodes) {
        for (int i = 0; i < n; i++) rows[i] = i;
        return;
    }
    std::vector<int> pos;
    if (!m.node_order_.empty()) {
        pos.assign(N, -1);
        for (int p = 0; p < N; p++) pos[m.node_order_[p]] = p;
    }
    const int r0 = m.row_start();
    for (int i = 0; i < n; i++) {
        const int id = nodes[i];
        if (id < 0 || id >= N) throw GcnHipFailure(-1, std::string(what) + ": node " + std::to_string(id) + " is not a node of the dataset (0.." + std::to_string(N - 1) + ")");
        const int r = (pos.empty() ? id : pos[id]) - r0;
        if (r < 0 || r >= m.n_local)
            throw GcnHipFailure(-1, std::string(what) + ": node " + std::to_string(id) + " is not a row of rank " + std::to_string(m.env.comm->rank()) + " (each rank predicts its own rows)");
        rows[i] = r;
    }
}

// a registered subset of the adjacency holding these rows: the same query reuses it
const gcnhip_rowset *ModelQueries::query_subset(const std::vector<int> &rows) {
    std::vector<uint32_t> bits(((size_t)m.n_local + 31) / 32 + 1, 0u);
    for (int r : rows) bits[r >> 5] |= 1u << (r & 31);
    if (!pred_rows || bits != pred_bits) {
        if (pred_rows) { GCNHIP_CHECK(gcnhip_graph_remove_rowset(m.env.ctx, m.graph, pred_rows)); pred_rows = nullptr; }
        GCNHIP_CHECK(gcnhip_graph_add_rowset(m.env.ctx, m.graph, bits.data(), &pred_rows));
        pred_bits.swap(bits);
    }
    return pred_rows;
}

// the logit aggregation runs the prediction epilogue instead of its usual launch and stores no logits
void ModelQueries::forward_predict(const gcnhip_rowset *subset, bool keep_logp) {
    const size_t nl = (size_t)m.n_local;
    HipGraphSum::Prediction req;
    req.rows = subset; req.pred = d_pred.need(nl); req.prob = d_prob.need(nl);
    req.ld_logp = m.params.output_dim;
    req.logp = keep_logp ? d_logp.need(nl * req.ld_logp) : nullptr;
    m.forward_hooked(&req, nullptr);
}

// the logit aggregation stores the requested rows into the scratch table instead of variable 6
void ModelQueries::forward_redirect(const gcnhip_rowset *subset) {
    HipGraphSum::Redirect req;
    req.ld = m.variables[6]->ld; req.rows = subset;
    req.data = d_ml_logits.need((size_t)m.n_local * req.ld);
    m.forward_hooked(nullptr, &req);
}

void ModelQueries::predict(const int *nodes, int n, int32_t *pred, float *prob, float *logp) {
    const int C = m.params.output_dim, n_local = m.n_local;
    require("predict", SINGLE_LABEL | CLASS_AGGREGATION | AT_MOST_64);
    if ((n > 0 && (!pred || !prob)) || n < 0) throw GcnHipFailure(-1, "predict: invalid argument");
    if (!nodes) n = n_local;
    std::vector<int> rows;
    query_rows("predict", nodes, n, rows);
    m.sync();                                                  // run()'s epochs in flight, the validation lane's pass
    const gcnhip_rowset *subset = nodes ? query_subset(rows) : nullptr;
    const bool scaled = temperature_ != 1.f;                   // a set temperature: the rows are kept and rescaled behind the forward
    forward_predict(subset, logp || scaled);
    if (n == 0) { m.sync(); return; }
    if (scaled) {
        // in place, so every queried row once: a query may repeat a node
        const int32_t *d_list = nullptr;
        int listed = n_local;
        if (nodes) {
            std::vector<int> once(rows);
            std::sort(once.begin(), once.end());
            once.erase(std::unique(once.begin(), once.end()), once.end());
            listed = (int)once.size();
            d_list = upload_rows(once);
        }
        GCNHIP_CHECK(gcnhip_calib_scale_rows(m.env.ctx, d_logp.p, C, n_local, d_list, listed, C, 1.f / temperature_, d_logp.p, C, d_prob.p));
    }
    const size_t nl = (size_t)n_local;                         // >= 1: some row was asked for
    std::vector<int32_t> hp(nl);
    std::vector<float> hq(nl), hl;
    GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, hp.data(), d_pred.p, nl * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, hq.data(), d_prob.p, nl * sizeof(float)));
    if (logp) {
        hl.resize(nl * C);
        GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, hl.data(), d_logp.p, nl * C * sizeof(float)));
    }
    for (int i = 0; i < n; i++) {
        pred[i] = hp[rows[i]];
        prob[i] = hq[rows[i]];
        if (logp) std::copy(hl.begin() + (size_t)rows[i] * C, hl.begin() + (size_t)(rows[i] + 1) * C, logp + (size_t)i * C);
    }
}

void ModelQueries::predict_multilabel(const int *nodes, int n, uint32_t *bits, float *prob) {
    require("predict_multilabel", MULTI_LABEL | CLASS_AGGREGATION);
    predict_multilabel_rows(nodes, n, nullptr, bits, prob);
}

void ModelQueries::predict_multilabel(const int *nodes, int n, const float *thr, int n_thr, uint32_t *bits, float *prob) {
    require("predict_multilabel", MULTI_LABEL | CLASS_AGGREGATION | ONE_RANK | AT_MOST_256);
    thresholds_check("predict_multilabel", thr, n_thr);
    predict_multilabel_rows(nodes, n, thr, bits, prob);
}

// what a query and an evaluation refuse of the cuts they are given
void ModelQueries::thresholds_check(const char *what, const float *thr, int n_thr) const {
    const int C = m.params.output_dim;
    if (!thr || n_thr != C)
        throw GcnHipFailure(-1, std::string(what) + ": " + std::to_string(thr ? n_thr : 0) + " thresholds for " + std::to_string(C) + " classes");
    for (int c = 0; c < C; c++)
        if (std::isnan(thr[c])) throw GcnHipFailure(-1, std::string(what) + ": the threshold of class " + std::to_string(c) + " is NaN");
}

const float *ModelQueries::upload_cuts(const float *thr) {
    const size_t C = (size_t)m.params.output_dim;
    GCNHIP_CHECK(gcnhip_h2d(m.env.ctx, d_th_cuts.need(C), thr, C * sizeof(float)));
    return d_th_cuts.p;
}

void ModelQueries::predict_multilabel_rows(const int *nodes, int n, const float *thr, uint32_t *bits, float *prob) {
    const int C = m.params.output_dim, wpr = m.ml_wpr;
    if ((n > 0 && !bits) || n < 0) throw GcnHipFailure(-1, "predict_multilabel: invalid argument");
    if (!nodes) n = m.n_local;
    std::vector<int> rows;
    query_rows("predict_multilabel", nodes, n, rows);
    m.sync();
    const gcnhip_rowset *subset = nodes ? query_subset(rows) : nullptr;
    d_ml_bits.need((size_t)n * wpr);
    d_ml_prob.need((size_t)n * C);
    d_ml_rows.need((size_t)n);
    forward_redirect(subset);
    if (n == 0) { m.sync(); return; }
    GCNHIP_CHECK(gcnhip_h2d(m.env.ctx, d_ml_rows.p, rows.data(), (size_t)n * sizeof(int32_t)));
    if (thr)
        GCNHIP_CHECK(gcnhip_bce_predict_rows_thr(m.env.ctx, d_ml_logits.p, m.variables[6]->ld, d_ml_rows.p, n, C, upload_cuts(thr), d_ml_bits.p, wpr,
                                                 prob ? d_ml_prob.p : nullptr, C));
    else
        GCNHIP_CHECK(gcnhip_bce_predict_rows(m.env.ctx, d_ml_logits.p, m.variables[6]->ld, d_ml_rows.p, n, C, d_ml_bits.p, wpr, prob ? d_ml_prob.p : nullptr, C));
    GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, bits, d_ml_bits.p, (size_t)n * wpr * sizeof(uint32_t)));
    if (prob) GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, prob, d_ml_prob.p, (size_t)n * C * sizeof(float)));
}

// a list of local rows on the device
const int32_t *ModelQueries::upload_rows(const std::vector<int> &rows) {
    d_eval_rows.need(rows.size());
    if (!rows.empty()) GCNHIP_CHECK(gcnhip_h2d(m.env.ctx, d_eval_rows.p, rows.data(), rows.size() * sizeof(int32_t)));
    return d_eval_rows.p;
}

// The rows to score: the split's list (already on the device on the fused path), or the query; their subset of the adjacency; and
// on a single-label model the truth they are scored against (a query: the labels themselves).  Synchronises before it touches the device.
ModelQueries::ScoredRows ModelQueries::scored_rows(const char *what, int split, const int *nodes, int n) {
    ScoredRows q{nullptr, n, nullptr, nullptr};
    std::vector<int> rows;
    bool upload = false;
    if (split) {
        if (m.d_split_list[split]) {
            q.d_list = m.d_split_list[split];
            q.n = m.split_local_n[split];
        } else {
            const int r0 = m.row_start();
            for (int r = 0; r < m.n_local; r++)
                if (m.data->split[r0 + r] == split) rows.push_back(r);
            q.n = (int)rows.size();
            upload = true;
        }
    } else {
        if (!nodes) q.n = m.n_local;
        query_rows(what, nodes, q.n, rows);
        upload = nodes != nullptr;                             // NULL: rows 0 .. n_local - 1, no list
    }
    m.sync();                                                  // run()'s epochs in flight, the validation lane's pass
    q.subset = split ? m.split_rows[split] : (nodes ? query_subset(rows) : nullptr);
    if (upload) q.d_list = upload_rows(rows);
    if (!m.opt_.multilabel) {
        q.truth = m.d_truth[split];
        if (!split) {                                          // a query is scored against the labels themselves, uploaded once
            if (!d_label_all) d_label_all = arena.upload(m.data->label.data() + m.row_start(), (size_t)m.n_local);
            q.truth = d_label_all;
        }
    }
    return q;
}

void ModelQueries::evaluate(int split, const int *nodes, int n, int64_t *counts, int64_t *rows_counted, int64_t *unlabelled) {
    require("evaluate", CLASS_AGGREGATION | (m.opt_.multilabel ? AT_MOST_256 : AT_MOST_64));
    evaluate_rows(split, nodes, n, nullptr, counts, rows_counted, unlabelled);
}

void ModelQueries::evaluate(int split, const int *nodes, int n, const float *thr, int n_thr, int64_t *counts, int64_t *rows_counted) {
    require("evaluate", MULTI_LABEL | CLASS_AGGREGATION | ONE_RANK | AT_MOST_256);
    thresholds_check("evaluate", thr, n_thr);
    evaluate_rows(split, nodes, n, thr, counts, rows_counted, nullptr);
}

void ModelQueries::evaluate_rows(int split, const int *nodes, int n, const float *thr, int64_t *counts, int64_t *rows_counted, int64_t *unlabelled) {
    const int C = m.params.output_dim;
    const bool ml = m.opt_.multilabel;
    if (split < 0 || split > 3 || !counts || n < 0) throw GcnHipFailure(-1, "evaluate: invalid argument (split is 0 with a node query, or 1 train, 2 validation, 3 test)");
    const ScoredRows q = scored_rows("evaluate", split, nodes, n);
    n = q.n;
    const int cells = ml ? 3 * C : C * C + 1;                  // all that crosses to the host ... or its two float limbs each, plus the listed rows' (below)
    int32_t *d_counts = d_eval_counts.need(((size_t)std::max(3 * C, C * C + 1) + 1) * 2);
    if (ml) {
        forward_redirect(q.subset);
        if (thr)
            GCNHIP_CHECK(gcnhip_bce_class_counts_rows_thr(m.env.ctx, d_ml_logits.p, m.variables[6]->ld, m.d_ml_truth, m.ml_wpr, q.d_list, n, C, upload_cuts(thr),
                                                          d_counts));
        else
            GCNHIP_CHECK(gcnhip_bce_class_counts_rows(m.env.ctx, d_ml_logits.p, m.variables[6]->ld, m.d_ml_truth, m.ml_wpr, q.d_list, n, C, d_counts));
    } else {
        forward_predict(q.subset, false);
        GCNHIP_CHECK(gcnhip_confusion_rows(m.env.ctx, d_pred.p, q.truth, m.n_local, q.d_list, n, C, d_counts, d_counts + C * C));
    }
    std::vector<int32_t> h(cells);
    GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, h.data(), d_counts, (size_t)cells * sizeof(int32_t)));
    std::vector<int64_t> total(h.begin(), h.end());
    int64_t listed = n;
    if (m.world() > 1) {
        // The counts are additive across ranks, like the four metric floats of an epoch, and go through the same float
        // all-reduce — as two limbs each, so that the sum is exact: a rank's count is below 2^31, so its high limb (count >> 12)
        // is below 2^19 and its low limb below 2^12; up to 32 ranks every partial sum of either stays below 2^24, where f32
        // holds every integer.  (One float per count would round silently from 2^24 rows in a cell.)
        if (m.world() > 32) throw GcnHipFailure(-1, "evaluate: the exact sum of the counts is laid out for at most 32 ranks");
        std::vector<float> limbs(2 * (size_t)(cells + 1));
        for (int i = 0; i <= cells; i++) {
            const int64_t v = i < cells ? (int64_t)h[i] : listed;
            limbs[2 * i] = (float)(v & 4095);
            limbs[2 * i + 1] = (float)(v >> 12);
        }
        float *d_limbs = (float *)d_counts;                    // sized for it above; the counts are on the host already
        GCNHIP_CHECK(gcnhip_h2d(m.env.ctx, d_limbs, limbs.data(), limbs.size() * sizeof(float)));
        m.env.comm->allreduce_sum(d_limbs, limbs.size());
        GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, limbs.data(), d_limbs, limbs.size() * sizeof(float)));
        for (int i = 0; i < cells; i++) total[i] = (int64_t)limbs[2 * i + 1] * 4096 + (int64_t)limbs[2 * i];
        listed = (int64_t)limbs[2 * cells + 1] * 4096 + (int64_t)limbs[2 * cells];
    }
    m.sync();
    std::copy(total.begin(), total.begin() + (ml ? 3 * C : C * C), counts);
    const int64_t no_truth = ml ? 0 : total[C * C];            // single-label: listed rows that are in no cell of the matrix
    if (rows_counted) *rows_counted = listed - no_truth;
    if (unlabelled) *unlabelled = no_truth;
}

// ---- label propagation and Correct & Smooth -----------------------------------------------------------------------------

void ModelQueries::smooth_check(const char *what, int needs, float alpha, int iters) const {
    require(what, needs | ONE_RANK);
    if (!(alpha >= 0.f && alpha <= 1.f)) throw GcnHipFailure(-1, std::string(what) + ": alpha must be in [0, 1]");
    if (iters < 0) throw GcnHipFailure(-1, std::string(what) + ": iters must be >= 0");
}

// label of every local row whose node is in a split of the mask, else -1; on the device too when `host` is NULL
const int32_t *ModelQueries::smooth_truth(const char *what, int splits_mask, std::vector<int32_t> *host) {
    if (splits_mask == 0 || (splits_mask & ~14))
        throw GcnHipFailure(-1, std::string(what) + ": splits are 1 (train), 2 (validation), 3 (test), at least one");
    if (!host)
        for (int s = 1; s <= 3; s++)
            if (splits_mask == (1 << s)) return m.d_truth[s];
    std::vector<int32_t> t((size_t)std::max(m.n_local, 1), -1);
    const int r0 = m.row_start();
    for (int r = 0; r < m.n_local; r++) {
        const int s = m.data->split[r0 + r];
        if (s >= 1 && s <= 3 && ((splits_mask >> s) & 1)) t[r] = m.data->label[r0 + r];
    }
    if (host) { host->swap(t); return nullptr; }
    GCNHIP_CHECK(gcnhip_h2d(m.env.ctx, d_smooth_truth.need(t.size()), t.data(), t.size() * sizeof(int32_t)));
    return d_smooth_truth.p;
}

// `iters` blend launches from `base` (= Y_0, never written), alternating between tables a and b; the last one writes pred
// when asked.  Returns the table that holds Y_iters (base itself when iters == 0).
float *ModelQueries::smooth_iterate(const float *base, float *a, float *b, int ld, int dim, float alpha, int iters, float lo, float hi, int32_t *pred) {
    const float *in = base;
    for (int k = 0; k < iters; k++) {
        float *out = (k & 1) ? b : a;
        GCNHIP_CHECK(gcnhip_graphsum_blend(m.env.ctx, m.graph, in, ld, base, ld, out, ld, dim, alpha, 1.f - alpha, lo, hi, k + 1 == iters ? pred : nullptr));
        in = out;
    }
    return const_cast<float *>(in);
}

// a table's rows to dataset node order; pred_from_rows: also the row argmax (lowest column on a tie), formed on the host
void ModelQueries::smooth_download(const float *table, int ld, int dim, float *out, int32_t *pred_from_rows) {
    if (!m.n_local) return;
    std::vector<float> h((size_t)m.n_local * ld);
    GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, h.data(), table, h.size() * sizeof(float)));
    for (int r = 0; r < m.n_local; r++) {
        const int id = m.node_id(r);
        const float *row = h.data() + (size_t)r * ld;
        if (out) std::copy(row, row + dim, out + (size_t)id * dim);
        if (pred_from_rows) pred_from_rows[id] = (int32_t)(std::max_element(row, row + dim) - row);
    }
}

void ModelQueries::smooth_pred_download(int32_t *pred) {
    if (!m.n_local) return;
    std::vector<int32_t> h((size_t)m.n_local);
    GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, h.data(), d_pred.p, h.size() * sizeof(int32_t)));
    for (int r = 0; r < m.n_local; r++) pred[m.node_id(r)] = h[r];
}

void ModelQueries::propagate(const float *y0, int dim, float alpha, int iters, float lo, float hi, float *out, int32_t *pred) {
    smooth_check("propagate", 0, alpha, iters);
    if (dim < 1 || dim > 64) throw GcnHipFailure(-1, "propagate: y0 has 1 to 64 columns (the row of a node sits in one wave)");
    if (!y0 || !out) throw GcnHipFailure(-1, "propagate: invalid argument");
    m.sync();                                                  // run()'s epochs in flight, the validation lane's pass
    const int ld = smooth_row_ld(dim);
    for (auto &t : d_smooth) t.need((size_t)m.n_local * ld);   // the four tables grow together
    {
        std::vector<float> h((size_t)std::max(m.n_local, 1) * ld, 0.f);
        for (int r = 0; r < m.n_local; r++) {
            const int id = m.node_id(r);
            std::copy(y0 + (size_t)id * dim, y0 + (size_t)(id + 1) * dim, h.begin() + (size_t)r * ld);
        }
        GCNHIP_CHECK(gcnhip_h2d(m.env.ctx, d_smooth[0].p, h.data(), h.size() * sizeof(float)));
    }
    const float *y = smooth_iterate(d_smooth[0].p, d_smooth[1].p, d_smooth[2].p, ld, dim, alpha, iters, lo, hi, pred ? d_pred.need((size_t)m.n_local) : nullptr);
    smooth_download(y, ld, dim, out, pred && iters == 0 ? pred : nullptr);
    if (pred && iters > 0) smooth_pred_download(pred);
    m.sync();
}

void ModelQueries::label_propagation(float alpha, int iters, int splits_mask, int32_t *pred, float *y) {
    const int C = m.params.output_dim;
    smooth_check("label_propagation", SINGLE_LABEL | AT_MOST_64, alpha, iters);
    if (!pred) throw GcnHipFailure(-1, "label_propagation: invalid argument");
    std::vector<int32_t> t;
    smooth_truth("label_propagation", splits_mask, &t);
    // Y_0 in dataset order: the one-hot rows of the known nodes
    std::vector<float> y0((size_t)m.params.num_nodes * C, 0.f), out(y ? 0 : y0.size());
    for (int r = 0; r < m.n_local; r++)
        if (t[r] >= 0 && t[r] < C) y0[(size_t)m.node_id(r) * C + t[r]] = 1.f;
    propagate(y0.data(), C, alpha, iters, 0.f, 1.f, y ? y : out.data(), pred);
}

void ModelQueries::correct_and_smooth(float alpha_correct, int iters_correct, float alpha_smooth, int iters_smooth, int splits_mask, int32_t *pred, float *g) {
    const int C = m.params.output_dim, n_local = m.n_local;
    smooth_check("correct_and_smooth", SINGLE_LABEL | CLASS_AGGREGATION | AT_MOST_64, alpha_correct, iters_correct);
    smooth_check("correct_and_smooth", 0, alpha_smooth, iters_smooth);
    if (!pred) throw GcnHipFailure(-1, "correct_and_smooth: invalid argument");
    m.sync();
    const int32_t *truth = smooth_truth("correct_and_smooth", splits_mask, nullptr);
    const int ld = smooth_row_ld(C);
    for (auto &t : d_smooth) t.need((size_t)m.n_local * ld);   // the four tables grow together
    d_sigma.need(2);
    forward_predict(nullptr, true);                            // P: predict()'s forward, the log-softmax rows kept on the device
    if (temperature_ != 1.f)                                   // the calibrated softmax is what gets corrected and smoothed
        GCNHIP_CHECK(gcnhip_calib_scale_rows(m.env.ctx, d_logp.p, C, n_local, nullptr, n_local, C, 1.f / temperature_, d_logp.p, C, nullptr));
    // correct: spread the residual of the known rows
    GCNHIP_CHECK(gcnhip_cs_error_rows(m.env.ctx, d_logp.p, C, truth, n_local, nullptr, n_local, C, d_smooth[0].p, ld, d_sigma.p));
    const float *eh = smooth_iterate(d_smooth[0].p, d_smooth[1].p, d_smooth[2].p, ld, C, alpha_correct, iters_correct, -1.f, 1.f, nullptr);
    // scale it, add it to P, reset the known rows to their labels; then smooth (E_0, E^ are done with: their tables are free)
    GCNHIP_CHECK(gcnhip_cs_correct_rows(m.env.ctx, d_logp.p, C, eh, ld, truth, n_local, C, d_sigma.p, d_smooth[3].p, ld));
    const float *G = smooth_iterate(d_smooth[3].p, d_smooth[0].p, d_smooth[1].p, ld, C, alpha_smooth, iters_smooth, 0.f, 1.f, d_pred.p);
    if (iters_smooth > 0) smooth_pred_download(pred);
    if (g || iters_smooth == 0) smooth_download(G, ld, C, g, iters_smooth == 0 ? pred : nullptr);
    m.sync();
}

// ---- temperature scaling and calibration error ---------------------------------------------------------------------------

// the kernels take beta = 1.f / T, which they accept up to GCNHIP_BETA_MAX (gcnhip_driver.h derives it): the same limit here,
// on the same f32 quotient, so that no temperature that is accepted is refused later by a launch
static void temperature_check(const char *what, float t) {
    if (!(t > 0.f) || !std::isfinite(t) || !(1.f / t <= GCNHIP_BETA_MAX))
        throw GcnHipFailure(-1, std::string(what) + ": the temperature must be finite and > 0, with 1 / T at most 8e37 (T >= 1.25e-38)");
}

void ModelQueries::calib_check(const char *what, float temperature, int bins) const {
    require(what, SINGLE_LABEL | CLASS_AGGREGATION | AT_MOST_64 | ONE_RANK);
    if (bins < 1 || bins > 64) throw GcnHipFailure(-1, std::string(what) + ": bins must be in 1..64");
    temperature_check(what, temperature);
}

void ModelQueries::set_temperature(float t) {
    temperature_check("set_temperature", t);
    if (t != 1.f) require("set_temperature", SINGLE_LABEL | AT_MOST_64);
    temperature_ = t;
}

// one bins launch on the rows d_logp holds, and its 3 . bins numbers to the host (slot 0 or 1 of the device scratch)
void ModelQueries::calib_bins_download(const ScoredRows &q, float beta, int bins, int slot, int64_t *count, int64_t *correct, double *conf_sum) {
    const int C = m.params.output_dim;
    int32_t *d_cnt = d_calib_counts.need(2 * 2 * 64) + slot * 128, *d_cor = d_cnt + bins;
    double *d_conf = d_calib_sums.p + 4 + slot * 64;
    GCNHIP_CHECK(gcnhip_calib_bins_rows(m.env.ctx, d_logp.p, C, q.truth, m.n_local, q.d_list, q.n, C, beta, bins, d_cnt, d_cor, d_conf));
    std::vector<int32_t> h(2 * (size_t)bins);
    GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, h.data(), d_cnt, h.size() * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, conf_sum, d_conf, (size_t)bins * sizeof(double)));
    std::copy(h.begin(), h.begin() + bins, count);
    std::copy(h.begin() + bins, h.end(), correct);
}

void ModelQueries::calibration(int split, const int *nodes, int n, float temperature, int bins, double *sums, int64_t *count, int64_t *correct, double *conf_sum) {
    calib_check("calibration", temperature, bins);
    if (split < 0 || split > 3 || n < 0 || !sums || !count || !correct || !conf_sum)
        throw GcnHipFailure(-1, "calibration: invalid argument (split is 0 with a node query, or 1 train, 2 validation, 3 test)");
    const int C = m.params.output_dim;
    const ScoredRows q = scored_rows("calibration", split, nodes, n);
    forward_predict(q.subset, true);
    const float beta = 1.f / temperature;
    GCNHIP_CHECK(gcnhip_calib_nll_rows(m.env.ctx, d_logp.p, C, q.truth, m.n_local, q.d_list, q.n, C, beta, d_calib_sums.need(4 + 2 * 64)));
    GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, sums, d_calib_sums.p, 4 * sizeof(double)));
    calib_bins_download(q, beta, bins, 0, count, correct, conf_sum);
    m.sync();
}

ModelQueries::Calibrated ModelQueries::calibrate(int split, int bins, int64_t *count, int64_t *correct, double *conf_sum) {
    calib_check("calibrate", 1.f, bins ? bins : 1);            // bins == 0: no reliability counts
    if (split < 1 || split > 3) throw GcnHipFailure(-1, "calibrate: split is 1 (train), 2 (validation) or 3 (test)");
    if (bins && (!count || !correct || !conf_sum)) throw GcnHipFailure(-1, "calibrate: invalid argument");
    if (m.split_count[split] < 1) throw GcnHipFailure(-1, "calibrate: split " + std::to_string(split) + " has no labelled rows to fit on");
    const int C = m.params.output_dim;
    const ScoredRows q = scored_rows("calibrate", split, nullptr, 0);
    forward_predict(q.subset, true);
    double s[4];
    double *d_sums = d_calib_sums.need(4 + 2 * 64);
    auto nll_at = [&](double beta) {                           // one launch, 32 bytes back
        GCNHIP_CHECK(gcnhip_calib_nll_rows(m.env.ctx, d_logp.p, C, q.truth, m.n_local, q.d_list, q.n, C, (float)beta, d_sums));
        GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, s, d_sums, sizeof s));
    };
    constexpr double LO = 0.01, HI = 100.0;
    double lo = LO, hi = HI, beta = 1.0;
    nll_at(beta);
    if (!(s[3] >= 1.0)) throw GcnHipFailure(-1, "calibrate: split " + std::to_string(split) + " has no labelled rows to fit on");
    Calibrated out;
    out.rows = (int64_t)s[3];
    out.nll_before = s[0] / s[3];
    while (out.steps < 40) {
        const double g = s[1], h = s[2];
        if (g > 0) hi = beta;                                  // convex: the minimum lies where the gradient points away from
        else if (g < 0) lo = beta;
        else break;
        double next = h > 0 ? beta - g / h : 0.0;
        // no minimum seen yet on the side the step goes to (that end is still the outer limit): at least a factor 2, so that a
        // minimum that is not there — the tail of a perfectly classified split, where a Newton step is a constant — is left behind
        if (h > 0 && g < 0 && hi == HI) next = std::max(next, 2 * beta);
        if (h > 0 && g > 0 && lo == LO) next = std::min(next, beta / 2);
        if (!(h > 0) || !(next > lo && next < hi)) next = std::sqrt(lo * hi);
        next = (double)(float)next;                            // the kernels take an f32 beta: iterate on the values they see
        const double delta = std::fabs(next - beta);
        beta = next;
        out.steps++;
        nll_at(beta);
        if (delta <= 1e-6 * beta) break;
    }
    out.temperature = (float)(1.0 / beta);
    out.nll_after = s[0] / s[3];
    // on an end of the bracket — or the gradient vanished in f32 before any minimum was bracketed on that side
    out.at_bound = (hi == HI && (beta >= HI * (1 - 1e-4) || (s[1] == 0 && beta > 1))) || (lo == LO && (beta <= LO * (1 + 1e-4) || (s[1] == 0 && beta < 1)));
    if (bins) {
        calib_bins_download(q, 1.f, bins, 0, count, correct, conf_sum);
        calib_bins_download(q, 1.f / out.temperature, bins, 1, count + bins, correct + bins, conf_sum + bins);
    }
    m.sync();
    return out;
}

// ---- node embeddings ------------------------------------------------------------------------------------------------------

void ModelQueries::embed_check(const char *what, int metric) const {
    require(what, ONE_RANK);
    if (m.params.hidden_dim < 1 || m.params.hidden_dim > 256)
        throw GcnHipFailure(-1, std::string(what) + ": a hidden width of at most 256 (the embedding kernels keep a query tile in LDS)");
    if (metric != METRIC_DOT && metric != METRIC_COSINE) throw GcnHipFailure(-1, std::string(what) + ": the metric is 0 (dot) or 1 (cosine)");
}

std::vector<int> ModelQueries::embed_query(const char *what, const int *nodes, int &n) {
    std::vector<int> all, rows;
    if (!nodes) {                                              // every node, in dataset id order
        all.resize((size_t)m.params.num_nodes);
        std::iota(all.begin(), all.end(), 0);
        nodes = all.data();
        n = (int)all.size();
    }
    query_rows(what, nodes, n, rows);
    return rows;
}

ModelQueries::EmbedTable ModelQueries::embed_forward(bool norms) {
    if (!m.forward_hidden_only()) forward_redirect(nullptr);
    const HipVariable &h1 = *m.variables[3];
    EmbedTable t{h1.data, h1.ld, m.n_local, m.params.hidden_dim, nullptr};
    if (norms) {
        GCNHIP_CHECK(gcnhip_embed_inv_norms(m.env.ctx, t.data, t.ld, t.rows, t.dim, d_emb_inv.need((size_t)t.rows)));
        t.inv_norm = d_emb_inv.p;
    }
    return t;
}

void ModelQueries::embed(const int *nodes, int n, float *out, bool normalize) {
    embed_check("embed", METRIC_DOT);
    if (n < 0 || (!out && (n > 0 || !nodes))) throw GcnHipFailure(-1, "embed: invalid argument");
    const std::vector<int> rows = embed_query("embed", nodes, n);
    m.sync();                                                  // run()'s epochs in flight, the validation lane's pass
    const EmbedTable t = embed_forward(normalize);
    if (n == 0) { m.sync(); return; }
    int32_t *d_rows = d_emb_rows.need((size_t)n);
    float *d_out = d_emb_out.need((size_t)n * t.dim);
    GCNHIP_CHECK(gcnhip_h2d(m.env.ctx, d_rows, rows.data(), (size_t)n * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_embed_rows(m.env.ctx, t.data, t.ld, t.rows, t.dim, t.inv_norm, d_rows, n, d_out, t.dim));
    GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, out, d_out, (size_t)n * t.dim * sizeof(float)));
}

void ModelQueries::similar(const int *nodes, int n, int k, int metric, bool exclude_self, int32_t *out_id, float *out_score) {
    embed_check("similar", metric);
    if (k < 1 || k > 64) throw GcnHipFailure(-1, "similar: k must be in 1..64 (a list is one entry per lane)");
    if (n < 0 || ((!out_id || !out_score) && (n > 0 || !nodes))) throw GcnHipFailure(-1, "similar: invalid argument");
    const std::vector<int> rows = embed_query("similar", nodes, n);
    m.sync();
    if (m.n_local < 1) {                                       // no candidate at all: every slot is the empty one
        std::fill(out_id, out_id + (size_t)n * k, -1);
        std::fill(out_score, out_score + (size_t)n * k, -INFINITY);
        return;
    }
    if (!d_node_ids) {                                         // the dataset id of every local row: the order never changes
        std::vector<int32_t> ids((size_t)m.n_local);
        for (int r = 0; r < m.n_local; r++) ids[r] = m.node_id(r);
        d_node_ids = arena.upload(ids.data(), ids.size());
    }
    const EmbedTable t = embed_forward(metric == METRIC_COSINE);
    if (n == 0) { m.sync(); return; }
    size_t full = 0, least = 0;
    if (gcnhip_topk_plan(t.rows, n, k, 0, nullptr, nullptr, &full, &least) != 0) throw GcnHipFailure(-1, std::string("similar: ") + gcnhip_last_error());
    const size_t bytes = std::max(std::min(full, EMBED_SCRATCH_CAP), least);
    int32_t *d_rows = d_emb_rows.need((size_t)n);
    int32_t *d_ids = d_emb_ids.need((size_t)n * k);
    float *d_scores = d_emb_out.need((size_t)n * k);
    GCNHIP_CHECK(gcnhip_h2d(m.env.ctx, d_rows, rows.data(), (size_t)n * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_topk_rows(m.env.ctx, t.data, t.ld, t.rows, t.dim, t.inv_norm, d_node_ids, d_rows, n, k, exclude_self ? 1 : 0, 0,
                                  d_emb_scratch.need(bytes), bytes, 3, d_ids, d_scores));
    GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, out_id, d_ids, (size_t)n * k * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, out_score, d_scores, (size_t)n * k * sizeof(float)));
}

void ModelQueries::score_pairs(const int *src, const int *dst, int n_pairs, int metric, float *out) {
    embed_check("score_pairs", metric);
    if (n_pairs < 0 || (n_pairs > 0 && (!src || !dst || !out))) throw GcnHipFailure(-1, "score_pairs: invalid argument");
    std::vector<int> rows, rows_dst;
    if (n_pairs) {
        query_rows("score_pairs", src, n_pairs, rows);
        query_rows("score_pairs", dst, n_pairs, rows_dst);
        rows.insert(rows.end(), rows_dst.begin(), rows_dst.end());
    }
    m.sync();
    const EmbedTable t = embed_forward(metric == METRIC_COSINE);
    if (n_pairs == 0) { m.sync(); return; }
    int32_t *d_rows = d_emb_rows.need(2 * (size_t)n_pairs);    // src, then dst
    float *d_out = d_emb_out.need((size_t)n_pairs);
    GCNHIP_CHECK(gcnhip_h2d(m.env.ctx, d_rows, rows.data(), rows.size() * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_pair_scores(m.env.ctx, t.data, t.ld, t.rows, t.dim, t.inv_norm, d_rows, d_rows + n_pairs, n_pairs, d_out));
    GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, out, d_out, (size_t)n_pairs * sizeof(float)));
}

// ---- explaining a logit ---------------------------------------------------------------------------------------------------

void ModelQueries::explain_check(const char *what, bool default_classes) const {
    require(what, ONE_RANK);
    const std::string w = std::string(what) + ": ";
    if (m.params.hidden_dim < 1 || m.params.hidden_dim > 256)
        throw GcnHipFailure(-1, w + "a hidden width of at most 256 (thread k of a workgroup owns hidden unit k)");
    if (m.flags & HIPGCN_BF16_TABLES) throw GcnHipFailure(-1, w + "not with bf16 tables (the gates are read from the f32 hidden matrix a forward stores)");
    // the logits of the default classes, and the hidden layer of a model without the aggregate-first form, come from a hooked forward
    if (default_classes || m.eval_modules.empty()) require(what, CLASS_AGGREGATION);
}

const std::vector<int> &ModelQueries::explain_indptr() {
    if (xp_indptr.empty()) {
        const int *d_indptr = nullptr;
        int n_rows = 0;
        GCNHIP_CHECK(gcnhip_graph_arrays(m.graph, &d_indptr, nullptr, nullptr, &n_rows, nullptr));
        xp_indptr.assign((size_t)n_rows + 1, 0);
        GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, xp_indptr.data(), d_indptr, xp_indptr.size() * sizeof(int)));
    }
    return xp_indptr;
}

int64_t ModelQueries::explain_size(const int *nodes, int n) {
    explain_check("explain", false);
    if (n < 0) throw GcnHipFailure(-1, "explain: invalid argument");
    const std::vector<int> rows = embed_query("explain", nodes, n);
    m.sync();
    const std::vector<int> &ip = explain_indptr();
    int64_t total = 0;
    for (int r : rows) total += ip[r + 1] - ip[r];
    return total;
}

ModelQueries::EmbedTable ModelQueries::explain_forward(const char *what, const std::vector<int> &rows, const int32_t *d_rows, const int *classes,
                                                       std::vector<int32_t> &cls) {
    const int C = m.params.output_dim, n = (int)rows.size();
    cls.resize(rows.size());
    if (classes) {
        for (int i = 0; i < n; i++) {
            if (classes[i] < 0 || classes[i] >= C)
                throw GcnHipFailure(-1, std::string(what) + ": class " + std::to_string(classes[i]) + " is not a class of the model (0.." + std::to_string(C - 1) + ")");
            cls[i] = classes[i];
        }
        return embed_forward(false);
    }
    // one evaluation forward with its logits in scratch; where its fused launch kept the hidden layer in registers, the layer's
    // own product stores it (same weights, same input: the forward's hidden layer)
    forward_redirect(nullptr);
    if (!m.eval_modules.empty() && static_cast<HipSparseMatmul *>(m.eval_modules[0])->hidden_not_stored) m.forward_hidden_only();
    const HipVariable &h1 = *m.variables[3];
    const EmbedTable t{h1.data, h1.ld, m.n_local, m.params.hidden_dim, nullptr};
    if (n == 0) return t;
    // the queried rows of the logits (d_rows: the caller's upload of `rows`), gathered on the device; the argmax (lowest class
    // on a tie) on the host
    const size_t batch = std::max<size_t>(1, ((size_t)16 << 20) / ((size_t)C * sizeof(float)));
    std::vector<float> z;
    for (size_t q0 = 0; q0 < (size_t)n; q0 += batch) {
        const size_t nb = std::min(batch, (size_t)n - q0);
        z.resize(nb * C);
        float *d_z = d_xp_z.need(nb * C);
        const int ld_z = m.variables[6]->ld;
        for (int c0 = 0; c0 < C; c0 += 256) {                   // the row gather takes at most 256 columns at a time
            const int cw = std::min(256, C - c0);
            GCNHIP_CHECK(gcnhip_embed_rows(m.env.ctx, d_ml_logits.p + c0, ld_z, m.n_local, cw, nullptr, d_rows + q0, (int)nb, d_z + c0, C));
        }
        GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, z.data(), d_z, z.size() * sizeof(float)));
        for (size_t i = 0; i < nb; i++) {
            const float *row = z.data() + i * C;
            cls[q0 + i] = (int32_t)(std::max_element(row, row + C) - row);
        }
    }
    return t;
}

void ModelQueries::explain_features(const EmbedTable &t, const int32_t *d_rows, const int32_t *d_cls, int n, size_t cap_bytes, float *host_out, double *d_acc,
                                    int32_t *d_count) {
    const int F = m.params.input_dim, C = m.params.output_dim;
    const HipVariable &w1 = *m.variables[2], &w2 = *m.variables[5];
    const int scaling = m.factored_ ? 1 : 0;
    if (!cap_bytes) cap_bytes = EMBED_SCRATCH_CAP;
    const size_t batch = std::max<size_t>(1, std::min(cap_bytes, EMBED_SCRATCH_CAP) / ((size_t)F * sizeof(float)));
    for (size_t q0 = 0; q0 < (size_t)n; q0 += batch) {
        const int nb = (int)std::min(batch, (size_t)n - q0);
        float *d_feat = d_xp_feat.need((size_t)nb * F);
        if (m.feat_agg)
            GCNHIP_CHECK(gcnhip_explain_features_agg(m.env.ctx, m.graph, d_rows + q0, d_cls + q0, nb, t.data, t.ld, t.dim, w2.data, w2.ld, C, w1.data, w1.ld, F,
                                                     gcnhip_feat_values(m.feat_agg), F, scaling, d_feat, F));
        else
            GCNHIP_CHECK(gcnhip_explain_features_walk(m.env.ctx, m.graph, m.feat, d_rows + q0, d_cls + q0, nb, t.data, t.ld, t.dim, w2.data, w2.ld, C, w1.data,
                                                      w1.ld, scaling, d_feat, F));
        if (d_acc) GCNHIP_CHECK(gcnhip_explain_abs_colsum(m.env.ctx, d_feat, F, d_cls + q0, nb, F, C, d_acc, d_count));
        if (host_out) GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, host_out + q0 * F, d_feat, (size_t)nb * F * sizeof(float)));
    }
}

void ModelQueries::explain(const int *nodes, const int *classes, int n, size_t feat_scratch_bytes, int32_t *out_class, float *logit, float *hidden, float *feat,
                           int64_t *nbr_ptr, int32_t *nbr_ids, float *nbr_values) {
    explain_check("explain", classes == nullptr);
    if (n < 0 || ((n > 0 || !nodes) && (!out_class || !logit || !hidden || !nbr_ptr || !nbr_ids || !nbr_values))) throw GcnHipFailure(-1, "explain: invalid argument");
    const std::vector<int> rows = embed_query("explain", nodes, n);
    const int h = m.params.hidden_dim, C = m.params.output_dim;
    if (classes)                                               // before any launch
        for (int i = 0; i < n; i++)
            if (classes[i] < 0 || classes[i] >= C)
                throw GcnHipFailure(-1, "explain: class " + std::to_string(classes[i]) + " is not a class of the model (0.." + std::to_string(C - 1) + ")");
    m.sync();                                                  // run()'s epochs in flight, the validation lane's pass
    const std::vector<int> &ip = explain_indptr();
    std::vector<int32_t> ptr((size_t)n + 1, 0), cls;
    int64_t total = 0;
    for (int i = 0; i < n; i++) {
        if (nbr_ptr) nbr_ptr[i] = total;
        ptr[i] = (int32_t)total;
        total += ip[rows[i] + 1] - ip[rows[i]];
        if (total > INT32_MAX) throw GcnHipFailure(-1, "explain: more than 2^31 - 1 neighbour entries in one query: ask for fewer nodes at a time");
    }
    if (nbr_ptr) nbr_ptr[n] = total;
    int32_t *d_rows = d_xp_rows.need((size_t)n), *d_cls = d_xp_cls.need((size_t)n), *d_ptr = d_xp_ptr.need((size_t)n);
    if (n) GCNHIP_CHECK(gcnhip_h2d(m.env.ctx, d_rows, rows.data(), (size_t)n * sizeof(int32_t)));
    const EmbedTable t = explain_forward("explain", rows, d_rows, classes, cls);
    if (n == 0) { m.sync(); return; }
    const HipVariable &w2 = *m.variables[5];
    int32_t *d_nrow = d_xp_nbr_row.need((size_t)total);
    float *d_nval = d_xp_nbr_val.need((size_t)total), *d_logit = d_xp_logit.need((size_t)n), *d_hidden = d_xp_hidden.need((size_t)n * h);
    GCNHIP_CHECK(gcnhip_h2d(m.env.ctx, d_cls, cls.data(), (size_t)n * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_h2d(m.env.ctx, d_ptr, ptr.data(), (size_t)n * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_explain_hops(m.env.ctx, m.graph, d_rows, d_cls, n, t.data, t.ld, t.dim, w2.data, w2.ld, C, m.factored_ ? 1 : 0, d_logit, d_hidden, h, d_ptr,
                                     d_nrow, d_nval, total));
    std::copy(cls.begin(), cls.end(), out_class);
    GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, logit, d_logit, (size_t)n * sizeof(float)));
    GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, hidden, d_hidden, (size_t)n * h * sizeof(float)));
    if (total) {
        GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, nbr_ids, d_nrow, (size_t)total * sizeof(int32_t)));
        GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, nbr_values, d_nval, (size_t)total * sizeof(float)));
        for (int64_t e = 0; e < total; e++) nbr_ids[e] = m.node_id(nbr_ids[e]);
    }
    if (feat) explain_features(t, d_rows, d_cls, n, feat_scratch_bytes, feat, nullptr, nullptr);
    m.sync();
}

void ModelQueries::feature_importance(int split, const int *nodes, int n, size_t feat_scratch_bytes, double *mean_abs, int64_t *count) {
    explain_check("feature_importance", true);
    if (m.params.output_dim > 256)
        throw GcnHipFailure(-1, "feature_importance: at most 256 classes (a thread keeps its column's sum of every class in LDS), this model has " +
                                    std::to_string(m.params.output_dim));
    if (split < 0 || split > 3 || n < 0 || !mean_abs || !count)
        throw GcnHipFailure(-1, "feature_importance: invalid argument (split is 0 with a node query, or 1 train, 2 validation, 3 test)");
    const int F = m.params.input_dim, C = m.params.output_dim;
    std::vector<int> rows;
    if (split) {                                               // the split's nodes in id order
        std::vector<int> ids;
        for (int id = 0; id < m.params.num_nodes; id++) ids.push_back(id);
        std::vector<int> all;
        query_rows("feature_importance", ids.data(), (int)ids.size(), all);
        const int r0 = m.row_start();
        for (int r : all)
            if (m.data->split[r0 + r] == split) rows.push_back(r);
        if (rows.empty()) throw GcnHipFailure(-1, "feature_importance: split " + std::to_string(split) + " has no rows");
    } else {
        rows = embed_query("feature_importance", nodes, n);
    }
    n = (int)rows.size();
    m.sync();
    std::vector<int32_t> cls;
    int32_t *d_rows = d_xp_rows.need((size_t)n);
    if (n) GCNHIP_CHECK(gcnhip_h2d(m.env.ctx, d_rows, rows.data(), (size_t)n * sizeof(int32_t)));
    const EmbedTable t = explain_forward("feature_importance", rows, d_rows, nullptr, cls);
    double *d_acc = d_xp_acc.need((size_t)C * F);
    int32_t *d_cnt = d_xp_count.need((size_t)C);
    GCNHIP_CHECK(gcnhip_memset_async(m.env.ctx, d_acc, 0, (size_t)C * F * sizeof(double)));
    GCNHIP_CHECK(gcnhip_memset_async(m.env.ctx, d_cnt, 0, (size_t)C * sizeof(int32_t)));
    if (n) {
        int32_t *d_cls = d_xp_cls.need((size_t)n);
        GCNHIP_CHECK(gcnhip_h2d(m.env.ctx, d_cls, cls.data(), (size_t)n * sizeof(int32_t)));
        explain_features(t, d_rows, d_cls, n, feat_scratch_bytes, nullptr, d_acc, d_cnt);
    }
    std::vector<int32_t> hc((size_t)C);
    GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, mean_abs, d_acc, (size_t)C * F * sizeof(double)));
    GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, hc.data(), d_cnt, (size_t)C * sizeof(int32_t)));
    for (int c = 0; c < C; c++) {
        count[c] = hc[c];
        if (hc[c])
            for (int f = 0; f < F; f++) mean_abs[(size_t)c * F + f] /= (double)hc[c];
    }
    m.sync();
}
