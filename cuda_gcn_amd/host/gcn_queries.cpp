// gcn_queries.cpp — what a caller asks of a built HipGCN between passes: variables and weights, prediction, per-class
// evaluation, the weights file.
#include "gcn.h"
#include "weights.h"
#include "hip_check.h"
#include <algorithm>
#include <cmath>

void HipGCN::row_scale(std::vector<float> &dinv) {
    dinv.assign((size_t)n_local, 1.f);
    const float *d = nullptr;
    GCNHIP_CHECK(gcnhip_graph_scales(graph, &d, nullptr, nullptr, nullptr));
    if (n_local) GCNHIP_CHECK(gcnhip_d2h(env.ctx, dinv.data(), d, dinv.size() * sizeof(float)));
}

void HipGCN::get_var(int k, bool grad, std::vector<float> &out, int *rows, int *cols) {
    if (k < 1 || k > 6) throw GcnHipFailure(-1, "get_var: k must be 1..6");
    HipVariable *v = variables[k].get();
    if (k == 3 && !grad && h1_from_fused_eval && !eval_modules.empty()) {
        // the last forward on this stream was an evaluation whose hidden matrix stayed in registers: run it as its own launch
        static_cast<HipSparseMatmul *>(eval_modules[0])->forward_stored();
        h1_from_fused_eval = false;
        sync();
    }
    out.resize((size_t)v->rows * v->cols);
    v->download(out.data(), grad);
    if (rows) *rows = v->rows;
    if (cols) *cols = v->cols;
}

void HipGCN::set_weights(const float *w1, const float *w2) {
    variables[2]->upload(w1);
    variables[5]->upload(w2);
    GCNHIP_CHECK(gcnhip_sumsq(env.ctx, variables[2]->data, (int64_t)variables[2]->elems(), optimizer->d_sumsq));
    sync();
}

// ---- prediction and the weights file (beyond the reference) ------------------------------------------------------------

// dataset node ids -> local rows of this rank (node_order() undone); NULL: every local row
void HipGCN::query_rows(const char *what, const int *nodes, int n, std::vector<int> &rows) {
    const int N = params.num_nodes;
    rows.resize(n);
    if (!nodes) {
        for (int i = 0; i < n; i++) rows[i] = i;
        return;
    }
    std::vector<int> pos;
    if (!node_order_.empty()) {
        pos.assign(N, -1);
        for (int p = 0; p < N; p++) pos[node_order_[p]] = p;
    }
    const int r0 = row_start();
    for (int i = 0; i < n; i++) {
        const int id = nodes[i];
        if (id < 0 || id >= N) throw GcnHipFailure(-1, std::string(what) + ": node " + std::to_string(id) + " is not a node of the dataset (0.." + std::to_string(N - 1) + ")");
        const int r = (pos.empty() ? id : pos[id]) - r0;
        if (r < 0 || r >= n_local)
            throw GcnHipFailure(-1, std::string(what) + ": node " + std::to_string(id) + " is not a row of rank " + std::to_string(env.comm->rank()) + " (each rank predicts its own rows)");
        rows[i] = r;
    }
}

// a registered subset of `graph` holding these rows: the same query reuses it
const gcnhip_rowset *HipGCN::query_subset(const std::vector<int> &rows) {
    std::vector<uint32_t> bits(((size_t)n_local + 31) / 32 + 1, 0u);
    for (int r : rows) bits[r >> 5] |= 1u << (r & 31);
    if (!pred_rows || bits != pred_bits) {
        if (pred_rows) { GCNHIP_CHECK(gcnhip_graph_remove_rowset(env.ctx, graph, pred_rows)); pred_rows = nullptr; }
        GCNHIP_CHECK(gcnhip_graph_add_rowset(env.ctx, graph, bits.data(), &pred_rows));
        pred_bits.swap(bits);
    }
    return pred_rows;
}

// An evaluation forward (eval_async's module list without the loss) on the main stream with one hook set on the logit
// aggregation: the prediction epilogue, or the logits redirected to a scratch table.  Training state stays as it was.
void HipGCN::forward_hooked(const HipGraphSum::Prediction *prediction, const HipGraphSum::Redirect *redirect) {
    refresh_input();
    const std::vector<Module *> &list = eval_modules.empty() ? modules : eval_modules;
    struct Unhook {                                            // also when a forward throws
        HipGraphSum *gs;
        ~Unhook() { gs->predict = nullptr; gs->redirect = nullptr; }
    } unhook{logits_gs};
    logits_gs->predict = prediction;
    logits_gs->redirect = redirect;
    for (size_t i = 0; i + 1 < list.size(); i++) list[i]->forward(false);           // the last module is the loss
    // variable 3: a fused evaluation keeps H1 in registers (what it held stays); otherwise the forward stored it
    if (eval_modules.empty() || !static_cast<HipSparseMatmul *>(eval_modules[0])->hidden_not_stored) h1_from_fused_eval = false;
}

// scratch logits of the multi-label prediction and evaluation [local rows x ld of Z], zeroed once
float *HipGCN::ml_logits_scratch() {
    if (!d_ml_logits) d_ml_logits = arena.alloc_zeroed<float>((size_t)std::max(n_local, 1) * variables[6]->ld);
    return d_ml_logits;
}

// predicted class and its probability per local row (predict, evaluate), on first use
void HipGCN::pred_scratch() {
    if (d_pred) return;
    const size_t nl = (size_t)std::max(n_local, 1);
    d_pred = arena.alloc<int32_t>(nl);
    d_prob = arena.alloc<float>(nl);
}

void HipGCN::predict(const int *nodes, int n, int32_t *pred, float *prob, float *logp) {
    const int C = params.output_dim;
    if (opt_.multilabel) throw GcnHipFailure(-1, "predict: this is a multi-label model: use predict_multilabel");
    if (!logits_gs) throw GcnHipFailure(-1, "predict: this model has no class-width aggregation");
    if (C > 64) throw GcnHipFailure(-1, "predict: at most 64 classes (the logit row of a node sits in one wave)");
    if ((n > 0 && (!pred || !prob)) || n < 0) throw GcnHipFailure(-1, "predict: invalid argument");
    if (!nodes) n = n_local;
    std::vector<int> rows;
    query_rows("predict", nodes, n, rows);
    sync();                                                    // run()'s epochs in flight, the validation lane's pass
    const gcnhip_rowset *subset = nodes ? query_subset(rows) : nullptr;
    const size_t nl = (size_t)std::max(n_local, 1);
    pred_scratch();
    const bool scaled = temperature_ != 1.f;                   // a set temperature: the rows are kept and rescaled behind the forward
    if ((logp || scaled) && !d_logp) d_logp = arena.alloc<float>(nl * C);
    // the logit aggregation runs the prediction epilogue instead of its usual launch and stores no logits
    HipGraphSum::Prediction req;
    req.rows = subset; req.pred = d_pred; req.prob = d_prob; req.logp = logp || scaled ? d_logp : nullptr; req.ld_logp = C;
    forward_hooked(&req, nullptr);
    if (n == 0) { sync(); return; }
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
        GCNHIP_CHECK(gcnhip_calib_scale_rows(env.ctx, d_logp, C, n_local, d_list, listed, C, 1.f / temperature_, d_logp, C, d_prob));
    }
    std::vector<int32_t> hp(nl);
    std::vector<float> hq(nl), hl;
    GCNHIP_CHECK(gcnhip_d2h(env.ctx, hp.data(), d_pred, nl * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_d2h(env.ctx, hq.data(), d_prob, nl * sizeof(float)));
    if (logp) {
        hl.resize(nl * C);
        GCNHIP_CHECK(gcnhip_d2h(env.ctx, hl.data(), d_logp, nl * C * sizeof(float)));
    }
    for (int i = 0; i < n; i++) {
        pred[i] = hp[rows[i]];
        prob[i] = hq[rows[i]];
        if (logp) std::copy(hl.begin() + (size_t)rows[i] * C, hl.begin() + (size_t)(rows[i] + 1) * C, logp + (size_t)i * C);
    }
}

void HipGCN::predict_multilabel(const int *nodes, int n, uint32_t *bits, float *prob) {
    const int C = params.output_dim;
    if (!opt_.multilabel) throw GcnHipFailure(-1, "predict_multilabel: this is a single-label model: use predict");
    if (!logits_gs) throw GcnHipFailure(-1, "predict_multilabel: this model has no class-width aggregation");
    if ((n > 0 && !bits) || n < 0) throw GcnHipFailure(-1, "predict_multilabel: invalid argument");
    if (!nodes) n = n_local;
    std::vector<int> rows;
    query_rows("predict_multilabel", nodes, n, rows);
    sync();
    const gcnhip_rowset *subset = nodes ? query_subset(rows) : nullptr;
    HipVariable *Z = variables[6].get();
    const size_t nq = (size_t)std::max(n, 1);
    ml_logits_scratch();
    if (nq > ml_query_cap) {
        ml_query_cap = 0;                                      // (a regrow that throws leaves NULL behind: nothing is sized until all three exist)
        arena.regrow(d_ml_bits, nq * ml_wpr);
        arena.regrow(d_ml_prob, nq * C);
        arena.regrow(d_ml_rows, nq);
        ml_query_cap = nq;
    }
    // the logit aggregation stores the requested rows into the scratch table instead of variable 6
    HipGraphSum::Redirect req;
    req.data = d_ml_logits; req.ld = Z->ld; req.rows = subset;
    forward_hooked(nullptr, &req);
    if (n == 0) { sync(); return; }
    GCNHIP_CHECK(gcnhip_h2d(env.ctx, d_ml_rows, rows.data(), (size_t)n * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_bce_predict_rows(env.ctx, d_ml_logits, Z->ld, d_ml_rows, n, C, d_ml_bits, ml_wpr, prob ? d_ml_prob : nullptr, C));
    GCNHIP_CHECK(gcnhip_d2h(env.ctx, bits, d_ml_bits, (size_t)n * ml_wpr * sizeof(uint32_t)));
    if (prob) GCNHIP_CHECK(gcnhip_d2h(env.ctx, prob, d_ml_prob, (size_t)n * C * sizeof(float)));
}

// a list of local rows on the device (evaluate's scratch, grown when needed)
const int32_t *HipGCN::upload_rows(const std::vector<int> &rows) {
    const size_t n = std::max(rows.size(), (size_t)1);
    if (n > eval_rows_cap) {
        eval_rows_cap = 0;
        arena.regrow(d_eval_rows, n);
        eval_rows_cap = n;
    }
    if (!rows.empty()) GCNHIP_CHECK(gcnhip_h2d(env.ctx, d_eval_rows, rows.data(), rows.size() * sizeof(int32_t)));
    return d_eval_rows;
}

// The rows to score: the split's list (already on the device on the fused path), or the query; their subset of `graph`; and on
// a single-label model the truth they are scored against (a query: the labels themselves).  Synchronises before it touches the device.
HipGCN::ScoredRows HipGCN::scored_rows(const char *what, int split, const int *nodes, int n) {
    ScoredRows q{nullptr, n, nullptr, nullptr};
    std::vector<int> rows;
    bool upload = false;
    if (split) {
        if (d_split_list[split]) {
            q.d_list = d_split_list[split];
            q.n = split_local_n[split];
        } else {
            const int r0 = row_start();
            for (int r = 0; r < n_local; r++)
                if (data->split[r0 + r] == split) rows.push_back(r);
            q.n = (int)rows.size();
            upload = true;
        }
    } else {
        if (!nodes) q.n = n_local;
        query_rows(what, nodes, q.n, rows);
        upload = nodes != nullptr;                             // NULL: rows 0 .. n_local - 1, no list
    }
    sync();                                                    // run()'s epochs in flight, the validation lane's pass
    q.subset = split ? split_rows[split] : (nodes ? query_subset(rows) : nullptr);
    if (upload) q.d_list = upload_rows(rows);
    if (!opt_.multilabel) {
        q.truth = d_truth[split];
        if (!split) {                                          // a query is scored against the labels themselves
            if (!d_label_all) {
                std::vector<int32_t> lab(data->label.begin() + row_start(), data->label.begin() + row_start() + n_local);
                if (lab.empty()) lab.assign(1, -1);
                d_label_all = arena.upload(lab.data(), lab.size());
            }
            q.truth = d_label_all;
        }
    }
    return q;
}

void HipGCN::evaluate(int split, const int *nodes, int n, int64_t *counts, int64_t *rows_counted, int64_t *unlabelled) {
    const int C = params.output_dim;
    const bool ml = opt_.multilabel;
    if (!logits_gs) throw GcnHipFailure(-1, "evaluate: this model has no class-width aggregation");
    if (!ml && C > 64) throw GcnHipFailure(-1, "evaluate: at most 64 classes on a single-label model (the logit row of a node sits in one wave)");
    if (ml && C > 256) throw GcnHipFailure(-1, "evaluate: at most 256 classes on a multi-label model");
    if (split < 0 || split > 3 || !counts || n < 0) throw GcnHipFailure(-1, "evaluate: invalid argument (split is 0 with a node query, or 1 train, 2 validation, 3 test)");
    const ScoredRows q = scored_rows("evaluate", split, nodes, n);
    const int32_t *d_list = q.d_list;
    const gcnhip_rowset *subset = q.subset;
    n = q.n;
    const int m = ml ? 3 * C : C * C + 1;                      // all that crosses to the host
    if (!d_eval_counts)                                        // ... or its two float limbs each, plus the listed rows' (below)
        d_eval_counts = arena.alloc<int32_t>(((size_t)std::max(3 * C, C * C + 1) + 1) * 2);
    if (ml) {
        HipVariable *Z = variables[6].get();
        HipGraphSum::Redirect req;
        req.data = ml_logits_scratch(); req.ld = Z->ld; req.rows = subset;
        forward_hooked(nullptr, &req);
        GCNHIP_CHECK(gcnhip_bce_class_counts_rows(env.ctx, d_ml_logits, Z->ld, d_ml_truth, ml_wpr, d_list, n, C, d_eval_counts));
    } else {
        pred_scratch();
        const int32_t *truth = q.truth;
        HipGraphSum::Prediction req;
        req.rows = subset; req.pred = d_pred; req.prob = d_prob;
        forward_hooked(&req, nullptr);
        GCNHIP_CHECK(gcnhip_confusion_rows(env.ctx, d_pred, truth, n_local, d_list, n, C, d_eval_counts, d_eval_counts + C * C));
    }
    std::vector<int32_t> h(m);
    GCNHIP_CHECK(gcnhip_d2h(env.ctx, h.data(), d_eval_counts, (size_t)m * sizeof(int32_t)));
    std::vector<int64_t> total(h.begin(), h.end());
    int64_t listed = n;
    if (world() > 1) {
        // The counts are additive across ranks, like the four metric floats of an epoch, and go through the same float
        // all-reduce — as two limbs each, so that the sum is exact: a rank's count is below 2^31, so its high limb (count >> 12)
        // is below 2^19 and its low limb below 2^12; up to 32 ranks every partial sum of either stays below 2^24, where f32
        // holds every integer.  (One float per count would round silently from 2^24 rows in a cell.)
        if (world() > 32) throw GcnHipFailure(-1, "evaluate: the exact sum of the counts is laid out for at most 32 ranks");
        std::vector<float> limbs(2 * (size_t)(m + 1));
        for (int i = 0; i <= m; i++) {
            const int64_t v = i < m ? (int64_t)h[i] : listed;
            limbs[2 * i] = (float)(v & 4095);
            limbs[2 * i + 1] = (float)(v >> 12);
        }
        float *d_limbs = (float *)d_eval_counts;               // sized for it above; the counts are on the host already
        GCNHIP_CHECK(gcnhip_h2d(env.ctx, d_limbs, limbs.data(), limbs.size() * sizeof(float)));
        env.comm->allreduce_sum(d_limbs, limbs.size());
        GCNHIP_CHECK(gcnhip_d2h(env.ctx, limbs.data(), d_limbs, limbs.size() * sizeof(float)));
        for (int i = 0; i < m; i++) total[i] = (int64_t)limbs[2 * i + 1] * 4096 + (int64_t)limbs[2 * i];
        listed = (int64_t)limbs[2 * m + 1] * 4096 + (int64_t)limbs[2 * m];
    }
    sync();
    std::copy(total.begin(), total.begin() + (ml ? 3 * C : C * C), counts);
    const int64_t no_truth = ml ? 0 : total[C * C];            // single-label: listed rows that are in no cell of the matrix
    if (rows_counted) *rows_counted = listed - no_truth;
    if (unlabelled) *unlabelled = no_truth;
}

// ---- label propagation and Correct & Smooth (beyond the reference) ------------------------------------------------------

void HipGCN::smooth_check(const char *what, float alpha, int iters) const {
    if (world() > 1)
        throw GcnHipFailure(-1, std::string(what) + ": one rank only (with several, every iteration would need a table exchange)");
    if (!(alpha >= 0.f && alpha <= 1.f)) throw GcnHipFailure(-1, std::string(what) + ": alpha must be in [0, 1]");
    if (iters < 0) throw GcnHipFailure(-1, std::string(what) + ": iters must be >= 0");
}

// the four tables, wide enough for rows of ld floats (zeroed: no launch reads their padding, a download may)
void HipGCN::smooth_tables(int ld) {
    if (ld <= smooth_ld) return;
    smooth_ld = 0;
    for (float *&t : d_smooth) {
        arena.release(t);
        t = nullptr;
        t = arena.alloc_zeroed<float>((size_t)std::max(n_local, 1) * ld);
    }
    smooth_ld = ld;
}

// label of every local row whose node is in a split of the mask, else -1; on the device too when `host` is NULL
const int32_t *HipGCN::smooth_truth(const char *what, int splits_mask, std::vector<int32_t> *host) {
    if (splits_mask == 0 || (splits_mask & ~14))
        throw GcnHipFailure(-1, std::string(what) + ": splits are 1 (train), 2 (validation), 3 (test), at least one");
    if (!host)
        for (int s = 1; s <= 3; s++)
            if (splits_mask == (1 << s)) return d_truth[s];
    std::vector<int32_t> t((size_t)std::max(n_local, 1), -1);
    const int r0 = row_start();
    for (int r = 0; r < n_local; r++) {
        const int s = data->split[r0 + r];
        if (s >= 1 && s <= 3 && ((splits_mask >> s) & 1)) t[r] = data->label[r0 + r];
    }
    if (host) { host->swap(t); return nullptr; }
    if (!d_smooth_truth) d_smooth_truth = arena.alloc<int32_t>(t.size());
    GCNHIP_CHECK(gcnhip_h2d(env.ctx, d_smooth_truth, t.data(), t.size() * sizeof(int32_t)));
    return d_smooth_truth;
}

// `iters` blend launches from `base` (= Y_0, never written), alternating between tables a and b; the last one writes pred
// when asked.  Returns the table that holds Y_iters (base itself when iters == 0).
float *HipGCN::smooth_iterate(const float *base, float *a, float *b, int ld, int dim, float alpha, int iters, float lo, float hi, int32_t *pred) {
    const float *in = base;
    for (int k = 0; k < iters; k++) {
        float *out = (k & 1) ? b : a;
        GCNHIP_CHECK(gcnhip_graphsum_blend(env.ctx, graph, in, ld, base, ld, out, ld, dim, alpha, 1.f - alpha, lo, hi, k + 1 == iters ? pred : nullptr));
        in = out;
    }
    return const_cast<float *>(in);
}

// a table's rows to dataset node order; pred_from_rows: also the row argmax (lowest column on a tie), formed on the host
void HipGCN::smooth_download(const float *table, int ld, int dim, float *out, int32_t *pred_from_rows) {
    if (!n_local) return;
    std::vector<float> h((size_t)n_local * ld);
    GCNHIP_CHECK(gcnhip_d2h(env.ctx, h.data(), table, h.size() * sizeof(float)));
    const int r0 = row_start();
    for (int r = 0; r < n_local; r++) {
        const int id = node_order_.empty() ? r0 + r : node_order_[r0 + r];
        const float *row = h.data() + (size_t)r * ld;
        if (out) std::copy(row, row + dim, out + (size_t)id * dim);
        if (pred_from_rows) pred_from_rows[id] = (int32_t)(std::max_element(row, row + dim) - row);
    }
}

void HipGCN::smooth_pred_download(int32_t *pred) {
    if (!n_local) return;
    std::vector<int32_t> h((size_t)n_local);
    GCNHIP_CHECK(gcnhip_d2h(env.ctx, h.data(), d_pred, h.size() * sizeof(int32_t)));
    const int r0 = row_start();
    for (int r = 0; r < n_local; r++) pred[node_order_.empty() ? r0 + r : node_order_[r0 + r]] = h[r];
}

void HipGCN::propagate(const float *y0, int dim, float alpha, int iters, float lo, float hi, float *out, int32_t *pred) {
    smooth_check("propagate", alpha, iters);
    if (dim < 1 || dim > 64) throw GcnHipFailure(-1, "propagate: y0 has 1 to 64 columns (the row of a node sits in one wave)");
    if (!y0 || !out) throw GcnHipFailure(-1, "propagate: invalid argument");
    sync();                                                    // run()'s epochs in flight, the validation lane's pass
    const int ld = smooth_row_ld(dim);
    smooth_tables(ld);
    pred_scratch();
    {
        std::vector<float> h((size_t)std::max(n_local, 1) * ld, 0.f);
        const int r0 = row_start();
        for (int r = 0; r < n_local; r++) {
            const int id = node_order_.empty() ? r0 + r : node_order_[r0 + r];
            std::copy(y0 + (size_t)id * dim, y0 + (size_t)(id + 1) * dim, h.begin() + (size_t)r * ld);
        }
        GCNHIP_CHECK(gcnhip_h2d(env.ctx, d_smooth[0], h.data(), h.size() * sizeof(float)));
    }
    const float *y = smooth_iterate(d_smooth[0], d_smooth[1], d_smooth[2], ld, dim, alpha, iters, lo, hi, pred ? d_pred : nullptr);
    smooth_download(y, ld, dim, out, pred && iters == 0 ? pred : nullptr);
    if (pred && iters > 0) smooth_pred_download(pred);
    sync();
}

void HipGCN::label_propagation(float alpha, int iters, int splits_mask, int32_t *pred, float *y) {
    const int C = params.output_dim;
    smooth_check("label_propagation", alpha, iters);
    if (opt_.multilabel) throw GcnHipFailure(-1, "label_propagation: this is a multi-label model (the scheme spreads one label per node)");
    if (C > 64) throw GcnHipFailure(-1, "label_propagation: at most 64 classes (the row of a node sits in one wave)");
    if (!pred) throw GcnHipFailure(-1, "label_propagation: invalid argument");
    std::vector<int32_t> t;
    smooth_truth("label_propagation", splits_mask, &t);
    // Y_0 in dataset order: the one-hot rows of the known nodes
    std::vector<float> y0((size_t)params.num_nodes * C, 0.f), out(y ? 0 : y0.size());
    const int r0 = row_start();
    for (int r = 0; r < n_local; r++)
        if (t[r] >= 0 && t[r] < C) y0[(size_t)(node_order_.empty() ? r0 + r : node_order_[r0 + r]) * C + t[r]] = 1.f;
    propagate(y0.data(), C, alpha, iters, 0.f, 1.f, y ? y : out.data(), pred);
}

void HipGCN::correct_and_smooth(float alpha_correct, int iters_correct, float alpha_smooth, int iters_smooth, int splits_mask, int32_t *pred, float *g) {
    const int C = params.output_dim;
    smooth_check("correct_and_smooth", alpha_correct, iters_correct);
    smooth_check("correct_and_smooth", alpha_smooth, iters_smooth);
    if (opt_.multilabel) throw GcnHipFailure(-1, "correct_and_smooth: this is a multi-label model (the scheme corrects a softmax)");
    if (!logits_gs) throw GcnHipFailure(-1, "correct_and_smooth: this model has no class-width aggregation");
    if (C > 64) throw GcnHipFailure(-1, "correct_and_smooth: at most 64 classes (the row of a node sits in one wave)");
    if (!pred) throw GcnHipFailure(-1, "correct_and_smooth: invalid argument");
    sync();
    const int32_t *truth = smooth_truth("correct_and_smooth", splits_mask, nullptr);
    const int ld = smooth_row_ld(C);
    const size_t nl = (size_t)std::max(n_local, 1);
    smooth_tables(ld);
    pred_scratch();
    if (!d_logp) d_logp = arena.alloc<float>(nl * C);
    if (!d_sigma) d_sigma = arena.alloc<float>(2);
    // P: predict()'s forward, the log-softmax rows kept on the device
    HipGraphSum::Prediction req;
    req.rows = nullptr; req.pred = d_pred; req.prob = d_prob; req.logp = d_logp; req.ld_logp = C;
    forward_hooked(&req, nullptr);
    if (temperature_ != 1.f)                                   // the calibrated softmax is what gets corrected and smoothed
        GCNHIP_CHECK(gcnhip_calib_scale_rows(env.ctx, d_logp, C, n_local, nullptr, n_local, C, 1.f / temperature_, d_logp, C, nullptr));
    // correct: spread the residual of the known rows
    GCNHIP_CHECK(gcnhip_cs_error_rows(env.ctx, d_logp, C, truth, n_local, nullptr, n_local, C, d_smooth[0], ld, d_sigma));
    const float *eh = smooth_iterate(d_smooth[0], d_smooth[1], d_smooth[2], ld, C, alpha_correct, iters_correct, -1.f, 1.f, nullptr);
    // scale it, add it to P, reset the known rows to their labels; then smooth (E_0, E^ are done with: their tables are free)
    GCNHIP_CHECK(gcnhip_cs_correct_rows(env.ctx, d_logp, C, eh, ld, truth, n_local, C, d_sigma, d_smooth[3], ld));
    const float *G = smooth_iterate(d_smooth[3], d_smooth[0], d_smooth[1], ld, C, alpha_smooth, iters_smooth, 0.f, 1.f, d_pred);
    if (iters_smooth > 0) smooth_pred_download(pred);
    if (g || iters_smooth == 0) smooth_download(G, ld, C, g, iters_smooth == 0 ? pred : nullptr);
    sync();
}

// ---- temperature scaling and calibration error (beyond the reference) ---------------------------------------------------

void HipGCN::calib_check(const char *what, float temperature, int bins) const {
    const std::string w(what);
    if (opt_.multilabel) throw GcnHipFailure(-1, w + ": this is a multi-label model (a temperature scales one softmax per node)");
    if (!logits_gs) throw GcnHipFailure(-1, w + ": this model has no class-width aggregation");
    if (params.output_dim > 64) throw GcnHipFailure(-1, w + ": at most 64 classes (the row of a node sits in one wave)");
    if (world() > 1) throw GcnHipFailure(-1, w + ": one rank only (the double sums would need an exact all-reduce that the float transport does not give)");
    if (bins < 1 || bins > 64) throw GcnHipFailure(-1, w + ": bins must be in 1..64");
    if (!(temperature > 0.f) || !std::isfinite(temperature)) throw GcnHipFailure(-1, w + ": the temperature must be finite and > 0");
}

void HipGCN::set_temperature(float t) {
    if (!(t > 0.f) || !std::isfinite(t)) throw GcnHipFailure(-1, "set_temperature: the temperature must be finite and > 0");
    if (t != 1.f && opt_.multilabel) throw GcnHipFailure(-1, "set_temperature: this is a multi-label model (a temperature scales one softmax per node)");
    if (t != 1.f && params.output_dim > 64) throw GcnHipFailure(-1, "set_temperature: at most 64 classes (the row of a node sits in one wave)");
    temperature_ = t;
}

void HipGCN::forward_logp(const gcnhip_rowset *subset) {
    const int C = params.output_dim;
    pred_scratch();
    if (!d_logp) d_logp = arena.alloc<float>((size_t)std::max(n_local, 1) * C);
    if (!d_calib_sums) {
        d_calib_sums = arena.alloc<double>(4 + 2 * 64);
        d_calib_counts = arena.alloc<int32_t>(2 * 2 * 64);
    }
    HipGraphSum::Prediction req;
    req.rows = subset; req.pred = d_pred; req.prob = d_prob; req.logp = d_logp; req.ld_logp = C;
    forward_hooked(&req, nullptr);
}

// one bins launch on the rows d_logp holds, and its 3 . bins numbers to the host (slot 0 or 1 of the device scratch)
void HipGCN::calib_bins_download(const ScoredRows &q, float beta, int bins, int slot, int64_t *count, int64_t *correct, double *conf_sum) {
    const int C = params.output_dim;
    int32_t *d_cnt = d_calib_counts + slot * 128, *d_cor = d_cnt + bins;
    double *d_conf = d_calib_sums + 4 + slot * 64;
    GCNHIP_CHECK(gcnhip_calib_bins_rows(env.ctx, d_logp, C, q.truth, n_local, q.d_list, q.n, C, beta, bins, d_cnt, d_cor, d_conf));
    std::vector<int32_t> h(2 * (size_t)bins);
    GCNHIP_CHECK(gcnhip_d2h(env.ctx, h.data(), d_cnt, h.size() * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_d2h(env.ctx, conf_sum, d_conf, (size_t)bins * sizeof(double)));
    std::copy(h.begin(), h.begin() + bins, count);
    std::copy(h.begin() + bins, h.end(), correct);
}

void HipGCN::calibration(int split, const int *nodes, int n, float temperature, int bins, double *sums, int64_t *count, int64_t *correct, double *conf_sum) {
    calib_check("calibration", temperature, bins);
    if (split < 0 || split > 3 || n < 0 || !sums || !count || !correct || !conf_sum)
        throw GcnHipFailure(-1, "calibration: invalid argument (split is 0 with a node query, or 1 train, 2 validation, 3 test)");
    const int C = params.output_dim;
    const ScoredRows q = scored_rows("calibration", split, nodes, n);
    forward_logp(q.subset);
    const float beta = 1.f / temperature;
    GCNHIP_CHECK(gcnhip_calib_nll_rows(env.ctx, d_logp, C, q.truth, n_local, q.d_list, q.n, C, beta, d_calib_sums));
    GCNHIP_CHECK(gcnhip_d2h(env.ctx, sums, d_calib_sums, 4 * sizeof(double)));
    calib_bins_download(q, beta, bins, 0, count, correct, conf_sum);
    sync();
}

HipGCN::Calibrated HipGCN::calibrate(int split, int bins, int64_t *count, int64_t *correct, double *conf_sum) {
    calib_check("calibrate", 1.f, bins ? bins : 1);            // bins == 0: no reliability counts
    if (split < 1 || split > 3) throw GcnHipFailure(-1, "calibrate: split is 1 (train), 2 (validation) or 3 (test)");
    if (bins && (!count || !correct || !conf_sum)) throw GcnHipFailure(-1, "calibrate: invalid argument");
    if (split_count[split] < 1) throw GcnHipFailure(-1, "calibrate: split " + std::to_string(split) + " has no labelled rows to fit on");
    const int C = params.output_dim;
    const ScoredRows q = scored_rows("calibrate", split, nullptr, 0);
    forward_logp(q.subset);
    double s[4];
    auto nll_at = [&](double beta) {                           // one launch, 32 bytes back
        GCNHIP_CHECK(gcnhip_calib_nll_rows(env.ctx, d_logp, C, q.truth, n_local, q.d_list, q.n, C, (float)beta, d_calib_sums));
        GCNHIP_CHECK(gcnhip_d2h(env.ctx, s, d_calib_sums, sizeof s));
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
    sync();
    return out;
}

void HipGCN::save_weights(const char *path) {
    std::vector<float> w1, w2;
    get_var(2, false, w1, nullptr, nullptr);
    get_var(5, false, w2, nullptr, nullptr);
    std::string err;
    if (gcn_weights_write(path, params.input_dim, params.hidden_dim, params.output_dim, w1.data(), w2.data(), &err) != 0) throw GcnHipFailure(-1, err);
}

void HipGCN::load_weights(const char *path) {
    int F = params.input_dim, h = params.hidden_dim, C = params.output_dim;
    std::vector<float> w1((size_t)F * h), w2((size_t)h * C);
    std::string err;
    if (gcn_weights_read(path, &F, &h, &C, w1.data(), w2.data(), &err) != 0) throw GcnHipFailure(-1, err);
    set_weights(w1.data(), w2.data());
}
