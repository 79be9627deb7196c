// tsne_query.cpp — ModelQueries::tsne: the exact t-SNE map of the hidden layer of a trained model (or of a caller's table), where
// it lies (queries.h has the contract, include/gcnhip_driver.h the definitions, csrc/tsne.hip the kernels).  Off the epoch path:
// the hidden layer comes from embed_forward and no training module is touched.
#include "queries.h"
#include "gcn.h"
#include "hip_check.h"
#include <algorithm>
#include <cmath>

int64_t ModelQueries::tsne_rows(int k, int split, const int *nodes, int n, const float *data, int data_dim, int iters, std::vector<int> *rows) {
    const char *what = "tsne";
    const std::string w = std::string(what) + ": ";
    require(what, ONE_RANK);
    if (m.flags & HIPGCN_BF16_TABLES) throw GcnHipFailure(-1, w + "not with bf16 tables (the kernels read the f32 rows of the hidden layer)");
    if (k != 2 && k != 3) throw GcnHipFailure(-1, w + "k must be 2 or 3, got " + std::to_string(k));
    if (iters < 1) throw GcnHipFailure(-1, w + "iters must be at least 1, got " + std::to_string(iters));
    if (n < 0) throw GcnHipFailure(-1, w + "invalid argument");
    if (data) {
        if (split != 0 || nodes) throw GcnHipFailure(-1, w + "with data the rows are the data's: no split and no node query");
        if (data_dim < 1 || data_dim > 256) throw GcnHipFailure(-1, w + "data of a width in 1..256, got " + std::to_string(data_dim));
        return n;
    }
    if (m.params.hidden_dim < 1 || m.params.hidden_dim > 256)
        throw GcnHipFailure(-1, w + "a hidden width of at most 256 (the gradient keeps a tile of rows in registers)");
    if (split < 0 || split > 3) throw GcnHipFailure(-1, w + "invalid argument (split is 0 with a node query, or 1 train, 2 validation, 3 test)");
    int listed = n;
    std::vector<int> list = kmeans_list(what, split, nodes, listed);   // a node id outside the graph is refused here
    if (rows) *rows = std::move(list);
    return listed;
}

ModelQueries::Tsne ModelQueries::tsne(int k, int split, const int *nodes, int n, const float *data, int data_dim, double perplexity, int iters,
                                      double exaggeration, int exaggeration_iters, double learning_rate, bool normalize, const double *init, int kl_every,
                                      size_t scratch_bytes, float *coords, double *beta, double *history) {
    Tsne res;
    std::vector<int> rows;
    res.rows = tsne_rows(k, split, nodes, n, data, data_dim, iters, &rows);      // every refusal that needs no GPU; the list is made once
    n = (int)res.rows;
    if (n < 1 || !init) throw GcnHipFailure(-1, "tsne: invalid argument (no rows, or no start)");
    if (kl_every < 1) kl_every = iters;
    m.sync();                                                  // run()'s epochs in flight, the validation lane's pass
    gcnhip_ctx *ctx = m.env.ctx;
    const size_t nn = (size_t)n, nk = nn * (size_t)k;
    EmbedTable t;
    const int32_t *d_rows = nullptr;
    if (data) {
        float *d = d_ts_data.need(nn * (size_t)data_dim);
        GCNHIP_CHECK(gcnhip_h2d(ctx, d, data, nn * (size_t)data_dim * sizeof(float)));
        t = EmbedTable{d, data_dim, n, data_dim, nullptr};
    } else {
        t = embed_forward(normalize);
        int32_t *r = d_ts_rows.need(nn);
        GCNHIP_CHECK(gcnhip_h2d(ctx, r, rows.data(), nn * sizeof(int32_t)));
        d_rows = r;
    }
    size_t pack_bytes = 0, full = 0, least = 0;
    if (gcnhip_tsne_plan(n, t.dim, &pack_bytes, &full, &least) != 0) throw GcnHipFailure(-1, std::string("tsne: ") + gcnhip_last_error());
    const size_t bytes = std::max(std::min(full, scratch_bytes ? scratch_bytes : TSNE_SCRATCH_DEFAULT), least);
    unsigned char *d_pack = d_ts_pack.need(pack_bytes), *d_scr = d_ts_scratch.need(bytes);
    int32_t *d_count = d_ts_count.need(2);
    const int n_hist = iters / kl_every + 1;
    double *d_state = d_ts_f64.need(3 * nk + 9 * nn + 2 * nn + 3 * (size_t)n_hist), *d_sums = d_state + 3 * nk, *d_beta = d_sums + 9 * nn,
           *d_invz = d_beta + nn, *d_hist = d_invz + nn;
    float *d_y = d_ts_f32.need(nk + nn), *d_m = d_y + nk;

    GCNHIP_CHECK(gcnhip_tsne_pack(ctx, t.data, t.ld, t.rows, t.dim, t.inv_norm, d_rows, n, d_pack, pack_bytes, d_count));
    int32_t points = 0;
    GCNHIP_CHECK(gcnhip_d2h(ctx, &points, d_count, sizeof(int32_t)));
    m.sync();
    res.points = points;
    if (!(perplexity >= 1.0) || !(perplexity < (double)points - 1.0))
        throw GcnHipFailure(-1, "tsne: perplexity must be in [1, points - 1) = [1, " + std::to_string(points - 1) + "), got " + std::to_string(perplexity));
    if (!(learning_rate > 0.0)) learning_rate = std::max((double)points / exaggeration / 4.0, 50.0);
    res.learning_rate = learning_rate;
    GCNHIP_CHECK(gcnhip_tsne_bandwidths(ctx, d_pack, n, t.dim, points, perplexity, d_beta, d_m, d_invz, d_count + 1, d_scr, bytes));

    std::vector<double> state(3 * nk, 0.0);                    // {y | update = 0 | gain = 1}
    std::vector<float> y32(nk);
    for (size_t e = 0; e < nk; e++) {
        state[e] = init[e];
        state[2 * nk + e] = 1.0;
        y32[e] = (float)init[e];
    }
    GCNHIP_CHECK(gcnhip_h2d(ctx, d_state, state.data(), state.size() * sizeof(double)));
    GCNHIP_CHECK(gcnhip_h2d(ctx, d_y, y32.data(), nk * sizeof(float)));
    int slot = 0;
    for (int it = 0; it < iters; it++) {                       // nothing below waits for the device
        const bool early = it < exaggeration_iters, record = (it + 1) % kl_every == 0 || it == iters - 1;
        GCNHIP_CHECK(gcnhip_tsne_gradient(ctx, d_pack, n, t.dim, d_y, k, record ? 1 : 0, d_sums, d_scr, bytes));
        GCNHIP_CHECK(gcnhip_tsne_update(ctx, d_pack, n, t.dim, k, d_sums, early ? exaggeration : 1.0, early ? 0.5 : 0.8, learning_rate, 1, d_state, d_y,
                                        nullptr, record ? d_hist + 3 * (size_t)slot : nullptr));
        if (record && history) history[3 * (size_t)slot] = (double)it;
        if (record) slot++;
    }
    std::vector<double> hist(3 * (size_t)slot);
    GCNHIP_CHECK(gcnhip_d2h(ctx, hist.data(), d_hist, hist.size() * sizeof(double)));
    int32_t unconv = 0;
    GCNHIP_CHECK(gcnhip_d2h(ctx, &unconv, d_count + 1, sizeof(int32_t)));
    if (coords) GCNHIP_CHECK(gcnhip_d2h(ctx, coords, d_y, nk * sizeof(float)));
    if (beta) GCNHIP_CHECK(gcnhip_d2h(ctx, beta, d_beta, nn * sizeof(double)));
    m.sync();
    res.unconverged = unconv;
    res.history_rows = slot;
    res.kl = hist[3 * (size_t)(slot - 1)];
    if (history)
        for (int s = 0; s < slot; s++) {                       // (iteration, KL, gradient norm)
            history[3 * (size_t)s + 1] = hist[3 * (size_t)s];
            history[3 * (size_t)s + 2] = hist[3 * (size_t)s + 1];
        }
    return res;
}
