// mc_dropout.cpp — ModelQueries::mc_dropout: per-node uncertainty from S stochastic forwards (queries.h has the contract,
// csrc/mcdropout.hip the definition and the two kernels).  Off the epoch path: the forward is composed here from the library's
// entry points, the way predict_new composes its own, and touches no training module.
#include "queries.h"
#include "gcn.h"
#include "hip_check.h"
#include <algorithm>
#include <cmath>

int64_t ModelQueries::mc_dropout_rows(int split, const int *nodes, int n, int samples, const float *p, uint64_t first_sample) {
    const char *what = "mc_dropout";
    const std::string w = std::string(what) + ": ";
    require(what, SINGLE_LABEL | AT_MOST_64 | ONE_RANK);
    if (m.flags & HIPGCN_BF16_TABLES) throw GcnHipFailure(-1, w + "not with bf16 tables (the stochastic forward aggregates the f32 rows a training forward stores)");
    const int H = m.params.hidden_dim;
    if (H < 1 || H > 256) throw GcnHipFailure(-1, w + "a hidden width of at most 256");
    if (samples < 1 || samples > MC_SAMPLES_MAX)
        throw GcnHipFailure(-1, w + "samples must be in 1.." + std::to_string(MC_SAMPLES_MAX) + ", got " + std::to_string(samples));
    const float rate = p ? *p : m.params.dropout;
    if (!(rate >= 0.f && rate < 1.f)) throw GcnHipFailure(-1, w + "the dropout rate p must be in [0, 1), got " + std::to_string(rate));
    if (first_sample + (uint64_t)samples > ((uint64_t)1 << 32) || first_sample > ((uint64_t)1 << 32))
        throw GcnHipFailure(-1, w + "first_sample + samples is above 2^32 (a sample's index is the 32-bit epoch word of its masks)");
    if (split < 0 || split > 3) throw GcnHipFailure(-1, w + "invalid argument (split is 0 with a node query, or 1 train, 2 validation, 3 test)");
    if (n < 0) throw GcnHipFailure(-1, w + "invalid argument");
    if (split) {
        const int r0 = m.row_start();
        int64_t k = 0;
        for (int r = 0; r < m.n_local; r++) k += m.data->split[r0 + r] == split;
        return k;
    }
    if (!nodes) return m.n_local;
    std::vector<int> rows;
    query_rows(what, nodes, n, rows);
    return n;
}

ModelQueries::McDropout ModelQueries::mc_dropout(int split, const int *nodes, int n, int samples, const float *p, const uint64_t *seed, uint64_t first_sample,
                                                 int32_t *pred, float *confidence, float *entropy, float *expected_entropy, float *mutual_information,
                                                 float *variation_ratio, float *mean_prob, int32_t *votes, float *samples_logp) {
    const char *what = "mc_dropout";
    McDropout res;
    res.rows = mc_dropout_rows(split, nodes, n, samples, p, first_sample);       // every refusal, before any launch
    res.p = p ? *p : m.params.dropout;
    res.seed = seed ? *seed : (m.env.seed ^ KEY_MC_DROPOUT);
    res.samples = samples;
    res.first_sample = first_sample;
    const int N = m.n_local, Hd = m.params.hidden_dim, C = m.params.output_dim, S = samples;
    const ScoredRows q = scored_rows(what, split, nodes, n);   // synchronises: run()'s epochs in flight, the validation lane's pass
    n = q.n;
    if (n == 0) return res;
    gcnhip_ctx *ctx = m.env.ctx;
    const HipVariable &T = *m.variables[1], &W1 = *m.variables[2], &H1 = *m.variables[3], &P = *m.variables[4], &W2 = *m.variables[5];
    const size_t nl = (size_t)N, nn = (size_t)n;
    float *d_t = d_mc_t.need(nl * T.ld), *d_h = d_mc_h.need(nl * H1.ld), *d_p = d_mc_p.need(nl * P.ld);
    int32_t *d_pr = d_pred.need(nl);
    float *d_pb = d_prob.need(nl), *d_lp = d_logp.need(nl * C);
    double *d_acc = d_mc_acc.need(nn * (C + 1));
    int32_t *d_vt = d_mc_votes.need(nn * C);
    // the epoch word of sample s: its index
    std::vector<uint32_t> words((size_t)S);
    for (int s = 0; s < S; s++) words[s] = (uint32_t)(first_sample + (uint64_t)s);
    uint32_t *d_words = d_mc_epoch.need((size_t)S);
    GCNHIP_CHECK(gcnhip_h2d(ctx, d_words, words.data(), words.size() * sizeof(uint32_t)));
    // a set temperature rescales the rows in place, so every queried row once: a query may repeat a node
    const bool scaled = temperature_ != 1.f;
    const int32_t *d_once = q.d_list;
    int listed_once = n;
    if (scaled && !split && nodes) {
        std::vector<int> once;
        query_rows(what, nodes, n, once);
        std::sort(once.begin(), once.end());
        once.erase(std::unique(once.begin(), once.end()), once.end());
        listed_once = (int)once.size();
        int32_t *d = d_mc_once.need(once.size());
        GCNHIP_CHECK(gcnhip_h2d(ctx, d, once.data(), once.size() * sizeof(int32_t)));
        d_once = d;
    }
    float *d_sl = samples_logp && q.d_list ? d_mc_samples.need((size_t)S * nn * C) : nullptr;
    // the training forward's own coefficient form (gcn_build.cpp): factored — the feature values carry dinv, the hidden
    // aggregation leaves dinv . H (scaling 2), the logits are the true ones (scaling 1); HIPGCN_EDGE_COEF — per-edge coefficients
    const int scaling_hidden = m.factored_ ? 2 : 0, scaling_logits = m.factored_ ? 1 : 0;
    for (int s = 0; s < S; s++) {
        const uint32_t *d_word = d_words + s;
        GCNHIP_CHECK(gcnhip_spmm_fwd(ctx, m.feat, gcnhip_feat_values(m.feat), W1.data, W1.ld, d_t, T.ld, Hd, res.p, res.seed ^ KEY_INPUT_DROPOUT, d_word, 0,
                                     nullptr));
        gcnhip_gs_opts o = {};
        o.scaling = scaling_hidden;
        o.relu_dropout = 1; o.training = 1; o.p = res.p;
        o.seed = res.seed ^ KEY_HIDDEN_DROPOUT; o.d_epoch = d_word; o.elem_offset = 0;
        GCNHIP_CHECK(gcnhip_graphsum_ex(ctx, m.graph, &o, d_t, T.ld, d_h, H1.ld, Hd));
        GCNHIP_CHECK(gcnhip_matmul_fwd(ctx, d_h, H1.ld, W2.data, W2.ld, d_p, P.ld, N, Hd, C));
        GCNHIP_CHECK(gcnhip_graphsum_predict(ctx, m.graph, q.subset, d_p, nullptr, P.ld, nullptr, 0, C, scaling_logits, d_pr, d_pb, d_lp, C));
        if (scaled) GCNHIP_CHECK(gcnhip_calib_scale_rows(ctx, d_lp, C, N, d_once, listed_once, C, 1.f / temperature_, d_lp, C, nullptr));
        GCNHIP_CHECK(gcnhip_mc_accumulate_rows(ctx, d_lp, C, N, q.d_list, n, C, s == 0 ? 1 : 0, d_acc, d_vt));
        if (samples_logp) {
            float *dst = samples_logp + (size_t)s * nn * C;
            if (d_sl) GCNHIP_CHECK(gcnhip_gather_rows(ctx, d_lp, C, q.d_list, n, d_sl + (size_t)s * nn * C));
            else GCNHIP_CHECK(gcnhip_d2h(ctx, dst, d_lp, nn * C * sizeof(float)));        // no list: rows 0 .. n - 1 as they lie
        }
    }
    // {confidence | entropy | expected entropy | mutual information | variation ratio} [5 x n], then mean_prob [n x C]
    float *d_out = d_mc_out.need(nn * (5 + (size_t)C));
    int32_t *d_best = d_mc_pred.need(nn);
    float *d_mp = d_out + 5 * nn;
    GCNHIP_CHECK(gcnhip_mc_finalize_rows(ctx, d_acc, d_vt, n, C, S, mean_prob ? d_mp : nullptr, C, d_best, d_out, d_out + nn, d_out + 2 * nn, d_out + 3 * nn,
                                         d_out + 4 * nn));
    if (pred) GCNHIP_CHECK(gcnhip_d2h(ctx, pred, d_best, nn * sizeof(int32_t)));
    float *const host[5] = {confidence, entropy, expected_entropy, mutual_information, variation_ratio};
    for (int k = 0; k < 5; k++)
        if (host[k]) GCNHIP_CHECK(gcnhip_d2h(ctx, host[k], d_out + (size_t)k * nn, nn * sizeof(float)));
    if (mean_prob) GCNHIP_CHECK(gcnhip_d2h(ctx, mean_prob, d_mp, nn * C * sizeof(float)));
    if (votes) GCNHIP_CHECK(gcnhip_d2h(ctx, votes, d_vt, nn * C * sizeof(int32_t)));
    if (d_sl) GCNHIP_CHECK(gcnhip_d2h(ctx, samples_logp, d_sl, (size_t)S * nn * C * sizeof(float)));
    m.sync();
    return res;
}
