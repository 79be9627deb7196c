// ranking.cpp — per-class ROC-AUC and average precision: ModelQueries::ranking on a built HipGCN, between passes (queries.h has
// the contract, csrc/ranking.hip the kernels and the formulas), and the host-only derivation of ranking.h.  Off the epoch path.
#include "ranking.h"
#include "queries.h"
#include "gcn.h"
#include "hip_check.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

int gcn_ranking_report(int C, const int64_t *u2, const double *ap_sum, const int64_t *pos, const int64_t *neg, RankingReport *out, std::string *err) {
    auto fail = [&](const std::string &why) {
        if (err) *err = "ranking_report: " + why;
        return -1;
    };
    if (!out) return fail("no output");
    if (C < 1) return fail("the number of classes must be at least 1");
    if (!u2 || !ap_sum || !pos || !neg) return fail("u2, ap_sum, pos and neg go together");
    RankingReport r;
    r.auc.assign(C, 0.0); r.ap.assign(C, 0.0); r.auc_defined.assign(C, 0); r.ap_defined.assign(C, 0);
    double sum_auc = 0, sum_ap = 0, w_auc = 0, w_ap = 0, wsum_auc = 0, wsum_ap = 0;
    int n_ap = 0;
    for (int c = 0; c < C; c++) {
        const std::string cls = " for class " + std::to_string(c);
        if (pos[c] < 0 || neg[c] < 0) return fail("negative count" + cls);
        if (pos[c] > ((int64_t)1 << 31) || neg[c] > ((int64_t)1 << 31)) return fail("a count above 2^31" + cls);
        const int64_t pairs2 = 2 * pos[c] * neg[c];
        if (u2[c] < 0 || u2[c] > pairs2) return fail("u2 outside [0, 2 P N]" + cls);
        if (!(ap_sum[c] >= 0.0) || ap_sum[c] > (double)pos[c]) return fail("ap_sum outside [0, P]" + cls);
        if (pos[c] > 0 && neg[c] > 0) {
            r.auc_defined[c] = 1;
            r.auc[c] = (double)u2[c] / (double)pairs2;
            sum_auc += r.auc[c];
            w_auc += (double)pos[c] * r.auc[c];
            wsum_auc += (double)pos[c];
            r.classes_defined++;
        }
        if (pos[c] > 0) {
            r.ap_defined[c] = 1;
            r.ap[c] = ap_sum[c] / (double)pos[c];
            sum_ap += r.ap[c];
            w_ap += (double)pos[c] * r.ap[c];
            wsum_ap += (double)pos[c];
            n_ap++;
        }
    }
    r.macro_auc = r.classes_defined ? sum_auc / r.classes_defined : 0.0;
    r.macro_ap = n_ap ? sum_ap / n_ap : 0.0;
    r.weighted_auc = wsum_auc > 0 ? w_auc / wsum_auc : 0.0;
    r.weighted_ap = wsum_ap > 0 ? w_ap / wsum_ap : 0.0;
    *out = std::move(r);
    return 0;
}

int gcn_ranking_report_write(const char *path, int C, const RankingReport &rep, const int64_t *pos, const int64_t *neg, std::string *err) {
    FILE *f = fopen(path, "w");
    bool ok = f != nullptr;
    for (int c = 0; ok && c < C; c++) {
        char a[40] = "undefined", p[40] = "undefined";
        if (rep.auc_defined[c]) snprintf(a, sizeof a, "%.9f", rep.auc[c]);
        if (rep.ap_defined[c]) snprintf(p, sizeof p, "%.9f", rep.ap[c]);
        ok = fprintf(f, "class %d pos %lld neg %lld auc %s ap %s\n", c, (long long)pos[c], (long long)neg[c], a, p) > 0;
    }
    if (ok)
        ok = fprintf(f, "macro_auc %.9f macro_ap %.9f weighted_auc %.9f weighted_ap %.9f classes %d\n", rep.macro_auc, rep.macro_ap, rep.weighted_auc,
                     rep.weighted_ap, rep.classes_defined) > 0;
    if (f && fclose(f) != 0) ok = false;
    if (!ok && err) *err = std::string("could not write the ranking report to ") + path;
    return ok ? 0 : -1;
}

// Classes in batches: the two key tables and their sort scratch — four columns of `stride` keys per class — fit the cap.
// A class's column is sorted and searched by itself, so no result depends on the batching.
const int32_t *ModelQueries::sorted_class_batches(const ScoredRows &q, const float *table, int ld, size_t scratch_bytes, const BatchStats &stats) {
    static_assert(GCNHIP_THRESHOLD_SCAN_BLOCKS <= GCNHIP_RANK_STATS_BLOCKS, "one work block serves both statistics");
    const int C = m.params.output_dim, n = q.n;
    const bool ml = m.opt_.multilabel;
    const size_t stride = (size_t)std::max(n, 1);
    const size_t cap = scratch_bytes ? scratch_bytes : RANKING_SCRATCH_DEFAULT;
    const int batch = (int)std::min<size_t>((size_t)C, std::max<size_t>(1, cap / (4 * stride * sizeof(uint32_t))));
    uint32_t *keys = d_rk_keys.need(4 * (size_t)batch * stride);
    uint32_t *sort_scratch = keys + 2 * (size_t)batch * stride;
    int32_t *d_counts = d_rk_counts.need(3 * (size_t)C + 1);   // pos | neg | invalid | unlabelled
    double *d_work = d_rk_work.need(2 * (size_t)batch * GCNHIP_RANK_STATS_BLOCKS);
    for (int c0 = 0; c0 < C; c0 += batch) {
        const int c1 = std::min(C, c0 + batch), S = c1 - c0;
        uint32_t *pos_keys = keys, *neg_keys = keys + (size_t)S * stride;     // back to back: 2 S segments for one sort call
        GCNHIP_CHECK(gcnhip_rank_keys(m.env.ctx, table, ld, m.n_local, q.d_list, n, c0, c1, C, ml ? nullptr : q.truth, ml ? m.d_ml_truth : nullptr, m.ml_wpr,
                                      pos_keys, neg_keys, (int64_t)stride, d_counts + c0, d_counts + C + c0, d_counts + 2 * C + c0,
                                      c0 == 0 ? d_counts + 3 * C : nullptr));
        GCNHIP_CHECK(gcnhip_sort_segments_u32(m.env.ctx, keys, sort_scratch, n, 2 * S, (int64_t)stride));
        stats(c0, S, pos_keys, neg_keys, (int64_t)stride, d_counts + c0, d_counts + C + c0, d_work);
    }
    return d_counts;
}

int64_t ModelQueries::ranking(int split, const int *nodes, int n, size_t scratch_bytes, int64_t *u2, double *ap_sum, int64_t *pos, int64_t *neg,
                              int64_t *invalid, int64_t *unlabelled, std::vector<float> *scores) {
    const int C = m.params.output_dim, n_local = m.n_local;
    const bool ml = m.opt_.multilabel;
    require("ranking", CLASS_AGGREGATION | ONE_RANK | (ml ? AT_MOST_256 : AT_MOST_64));
    if (split < 0 || split > 3 || n < 0 || !u2 || !ap_sum || !pos || !neg || !invalid)
        throw GcnHipFailure(-1, "ranking: invalid argument (split is 0 with a node query, or 1 train, 2 validation, 3 test)");
    if ((!split && nodes ? n : n_local) > RANKING_ROWS_MAX) throw GcnHipFailure(-1, "ranking: at most 2^24 listed rows");
    const ScoredRows q = scored_rows("ranking", split, nodes, n);
    n = q.n;
    // one forward; the score table: the log-softmax rows at the model's temperature, or the logits of a multi-label model
    const float *table;
    int ld;
    if (ml) {
        forward_redirect(q.subset);
        table = d_ml_logits.p;
        ld = m.variables[6]->ld;
    } else {
        forward_predict(q.subset, true);
        table = d_logp.p;
        ld = C;
        if (temperature_ != 1.f && n > 0) {
            // in place, so every queried row once, as predict() does it: a split lists its rows once, a query may repeat a node
            const int32_t *d_once = q.d_list;
            int listed = n;
            if (!split && nodes) {
                std::vector<int> once;
                query_rows("ranking", nodes, n, once);
                std::sort(once.begin(), once.end());
                once.erase(std::unique(once.begin(), once.end()), once.end());
                listed = (int)once.size();
                int32_t *d = d_rk_once.need(once.size());
                GCNHIP_CHECK(gcnhip_h2d(m.env.ctx, d, once.data(), once.size() * sizeof(int32_t)));
                d_once = d;
            }
            GCNHIP_CHECK(gcnhip_calib_scale_rows(m.env.ctx, d_logp.p, C, n_local, d_once, listed, C, 1.f / temperature_, d_logp.p, C, d_prob.p));
        }
    }
    double *d_ap = d_rk_sums.need(2 * (size_t)C);              // ap_sum [C] | u2 [C] (int64)
    int64_t *d_u2 = (int64_t *)(d_ap + C);
    const int32_t *d_counts = sorted_class_batches(q, table, ld, scratch_bytes, [&](int c0, int S, const uint32_t *pos_keys, const uint32_t *neg_keys,
                                                                                    int64_t stride, const int32_t *d_pos, const int32_t *d_neg, void *d_work) {
        GCNHIP_CHECK(gcnhip_rank_stats(m.env.ctx, pos_keys, neg_keys, stride, n, S, d_pos, d_neg, d_work, d_u2 + c0, d_ap + c0));
    });
    std::vector<int32_t> hc(3 * (size_t)C + 1);
    std::vector<double> hs(2 * (size_t)C);
    GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, hc.data(), d_counts, hc.size() * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, hs.data(), d_ap, hs.size() * sizeof(double)));
    if (scores) {
        std::vector<float> h((size_t)std::max(n, 1) * ld);
        if (n > 0 && q.d_list) {
            float *d = d_rk_scores.need((size_t)n * ld);
            GCNHIP_CHECK(gcnhip_gather_rows(m.env.ctx, table, ld, q.d_list, n, d));
            GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, h.data(), d, (size_t)n * ld * sizeof(float)));
        } else if (n > 0) {
            GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, h.data(), table, (size_t)n * ld * sizeof(float)));
        }
        scores->resize((size_t)n * C);
        for (int i = 0; i < n; i++) std::copy(h.begin() + (size_t)i * ld, h.begin() + (size_t)i * ld + C, scores->begin() + (size_t)i * C);
    }
    m.sync();
    for (int c = 0; c < C; c++) {
        pos[c] = hc[c]; neg[c] = hc[C + c]; invalid[c] = hc[2 * C + c];
        ap_sum[c] = hs[c];
        memcpy(&u2[c], &hs[C + c], sizeof(int64_t));
    }
    if (unlabelled) *unlabelled = hc[3 * C];
    return n;
}
