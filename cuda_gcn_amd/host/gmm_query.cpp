// gmm_query.cpp — ModelQueries::gmm / gmm_score: a Gaussian mixture of the hidden layer of a trained model (or of a caller's table) by
// expectation maximisation, where it lies (queries.h has the contract, include/gcnhip_driver.h the definitions, csrc/gmm.hip the
// kernels, gmm.h the information criteria).  Off the epoch path: the hidden layer comes from embed_forward, the loop is composed here
// from the library's entry points, and no training module is touched.
#include "queries.h"
#include "gcn.h"
#include "hip_check.h"
#include <algorithm>
#include <cmath>
#include <numeric>

int64_t ModelQueries::gmm_rows(const char *what, int k, int split, const int *nodes, int n, const float *data, int data_dim, std::vector<int> *rows) {
    const std::string w = std::string(what) + ": ";
    require(what, ONE_RANK);
    if (m.flags & HIPGCN_BF16_TABLES) throw GcnHipFailure(-1, w + "not with bf16 tables (the kernels read the f32 rows of the hidden layer)");
    if (k < 1 || k > 256) throw GcnHipFailure(-1, w + "k must be in 1..256, got " + std::to_string(k));
    if (n < 0) throw GcnHipFailure(-1, w + "invalid argument");
    int listed = n;
    if (data) {
        if (split != 0 || nodes) throw GcnHipFailure(-1, w + "with data the rows are the data's: no split and no node query");
        if (data_dim < 1 || data_dim > 256) throw GcnHipFailure(-1, w + "data of a width in 1..256, got " + std::to_string(data_dim));
        if (rows) { rows->resize((size_t)n); std::iota(rows->begin(), rows->end(), 0); }
    } else {
        if (m.params.hidden_dim < 1 || m.params.hidden_dim > 256)
            throw GcnHipFailure(-1, w + "a hidden width of at most 256 (the E-step keeps a row's operand in registers)");
        if (split < 0 || split > 3) throw GcnHipFailure(-1, w + "invalid argument (split is 0 with a node query, or 1 train, 2 validation, 3 test)");
        std::vector<int> list = kmeans_list(what, split, nodes, listed);   // a node id outside the graph is refused here
        if (rows) *rows = std::move(list);
    }
    return listed;
}

int64_t ModelQueries::gmm_check(int k, int split, const int *nodes, int n, const float *data, int data_dim, int iters, double tol, double reg_covar,
                                int init, const int *init_pos, const float *init_means, std::vector<int> *rows) {
    const char *what = "gmm";
    const std::string w = std::string(what) + ": ";
    const int64_t listed = gmm_rows(what, k, split, nodes, n, data, data_dim, rows);
    if (k > listed) throw GcnHipFailure(-1, w + "k = " + std::to_string(k) + " is above the " + std::to_string(listed) + " rows listed");
    if (iters < 1) throw GcnHipFailure(-1, w + "iters must be at least 1, got " + std::to_string(iters));
    if (!(tol >= 0.0) || !std::isfinite(tol)) throw GcnHipFailure(-1, w + "tol must be finite and at least 0, got " + std::to_string(tol));
    if (!(reg_covar > 0.0) || !std::isfinite(reg_covar)) throw GcnHipFailure(-1, w + "reg_covar must be finite and above 0, got " + std::to_string(reg_covar));
    if (init != GMM_INIT_KMEANS && init != GMM_INIT_POSITIONS && init != GMM_INIT_MEANS)
        throw GcnHipFailure(-1, w + "init is 0 (k-means), 1 (k list positions) or 2 (k means)");
    if (init == GMM_INIT_KMEANS && data) throw GcnHipFailure(-1, w + "with data, init is k list positions or k means (k-means runs on the model's rows)");
    if ((init == GMM_INIT_POSITIONS && !init_pos) || (init == GMM_INIT_MEANS && !init_means))
        throw GcnHipFailure(-1, w + "invalid argument (the initial positions or means are missing)");
    const int dim = data ? data_dim : m.params.hidden_dim;
    if (init == GMM_INIT_POSITIONS)
        for (int c = 0; c < k; c++)
            if (init_pos[c] < 0 || init_pos[c] >= listed)
                throw GcnHipFailure(-1, w + "initial position " + std::to_string(init_pos[c]) + " is outside the list (0.." + std::to_string(listed - 1) + ")");
    if (init == GMM_INIT_MEANS)
        for (size_t e = 0; e < (size_t)k * dim; e++)
            if (!std::isfinite(init_means[e])) throw GcnHipFailure(-1, w + "an initial mean is not finite");
    return listed;
}

// the table of a query and its list on the device: the caller's rows (uploaded) or the hidden layer
ModelQueries::EmbedTable ModelQueries::gmm_table(const std::vector<int> &rows, const float *data, int data_dim, bool normalize, int32_t *d_rows) {
    gcnhip_ctx *ctx = m.env.ctx;
    const size_t nn = rows.size();
    EmbedTable t;
    if (data) {
        float *d = d_gm_data.need(nn * (size_t)data_dim);
        GCNHIP_CHECK(gcnhip_h2d(ctx, d, data, nn * (size_t)data_dim * sizeof(float)));
        t = EmbedTable{d, data_dim, (int)nn, data_dim, nullptr};
    } else {
        t = embed_forward(normalize);
    }
    if (nn) GCNHIP_CHECK(gcnhip_h2d(ctx, d_rows, rows.data(), nn * sizeof(int32_t)));
    return t;
}

// {shift [ldc] | mu | var | prec | mprec [k x ldc] | weights | cst [k4] | lse | max_resp [n]}
struct GmmBlock {
    int ldc, k4;
    float *shift, *mu, *var, *prec, *mprec, *weights, *cst, *lse, *max_resp;
    static size_t floats(int k, int dim, size_t n) { return (size_t)((dim + 3) / 4 * 4) * (1 + 4 * (size_t)k) + 2 * (size_t)((k + 3) / 4 * 4) + 2 * n; }
    GmmBlock(float *p, int k, int dim, size_t n) : ldc((dim + 3) / 4 * 4), k4((k + 3) / 4 * 4) {
        const size_t kl = (size_t)k * ldc;
        shift = p; mu = shift + ldc; var = mu + kl; prec = var + kl; mprec = prec + kl; weights = mprec + kl; cst = weights + k4; lse = cst + k4;
        max_resp = lse + n;
    }
};

ModelQueries::Gmm ModelQueries::gmm(int k, int split, const int *nodes, int n, const float *data, int data_dim, int iters, double tol, bool spherical,
                                    double reg_covar, bool normalize, int init, const int *init_pos, const float *init_means, const uint64_t *seed,
                                    size_t scratch_bytes, float *weights, float *means, float *variances, int32_t *assign, float *max_resp,
                                    float *log_likelihood, float *resp, double *sizes, float *shift, double *history, int64_t *contingency,
                                    int64_t capacity) {
    const char *what = "gmm";
    Gmm res;
    std::vector<int> rows;
    res.rows = gmm_check(k, split, nodes, n, data, data_dim, iters, tol, reg_covar, init, init_pos, init_means, &rows);   // every refusal, before any launch
    if (capacity >= 0 && res.rows > capacity)
        throw GcnHipFailure(-1, "gmm: the query lists " + std::to_string(res.rows) + " rows, the outputs have room for " + std::to_string(capacity));
    res.k = k;
    res.seed = seed ? *seed : m.env.seed;
    const int C = m.params.output_dim;
    if (contingency && (data || m.opt_.multilabel || C > 64))
        throw GcnHipFailure(-1, std::string(what) + ": the component x class table needs the nodes of a single-label model with at most 64 classes");
    const int n_in = n;
    n = (int)rows.size();
    const size_t nn = (size_t)n;
    gcnhip_ctx *ctx = m.env.ctx;
    std::vector<int32_t> first((size_t)n);
    std::vector<float> centres;
    if (init == GMM_INIT_KMEANS) {                             // the existing clustering, its assignment as the first responsibilities
        centres.resize((size_t)k * m.params.hidden_dim);
        kmeans(k, split, nodes, n_in, 100, normalize, KMEANS_INIT_PLUSPLUS, nullptr, nullptr, seed, 0, first.data(), nullptr, centres.data(), nullptr,
               nullptr, nullptr, nullptr);
    }
    m.sync();                                                  // run()'s epochs in flight, the validation lane's pass
    int32_t *d_rows = d_gm_int.need(2 * nn), *d_assign = d_rows + nn;
    const EmbedTable t = gmm_table(rows, data, data_dim, normalize, d_rows);
    const int dim = t.dim, W = 1 + 2 * dim;
    GmmBlock B(d_gm_f32.need(GmmBlock::floats(k, dim, nn)), k, dim, nn);
    double *d_sums = d_gm_f64.need((size_t)k * W + (size_t)iters + 1 + (size_t)dim), *d_lsum = d_sums + (size_t)k * W, *d_mean = d_lsum + iters + 1;

    // the shift: the f32-rounded float64 mean of the listed rows
    size_t pca_least = 0, e_bytes = 0, m_full = 0, m_least = 0;
    if (gcnhip_pca_plan(n, dim, nullptr, &pca_least) != 0 || gcnhip_gmm_plan(n, k, dim, &e_bytes, &m_full, &m_least) != 0)
        throw GcnHipFailure(-1, std::string(what) + ": " + gcnhip_last_error());
    GCNHIP_CHECK(gcnhip_pca_mean(ctx, t.data, t.ld, t.rows, dim, t.inv_norm, d_rows, n, d_mean, d_pca_count.need(1), d_pca_scratch.need(pca_least), pca_least));
    std::vector<double> mean64((size_t)dim);
    GCNHIP_CHECK(gcnhip_d2h(ctx, mean64.data(), d_mean, (size_t)dim * sizeof(double)));
    std::vector<float> sh((size_t)B.ldc, 0.f);
    for (int j = 0; j < dim; j++) sh[j] = (float)mean64[j];
    GCNHIP_CHECK(gcnhip_h2d(ctx, B.shift, sh.data(), sh.size() * sizeof(float)));

    // the scratch: {the E-step's partials | lj | the M-step's partials}, lj whole when the cap allows it, else per batch of parts
    const size_t cap = scratch_bytes ? scratch_bytes : GMM_SCRATCH_DEFAULT, lj_full = nn * k * sizeof(float);
    const bool whole = lj_full + m_least <= cap;
    const size_t part_lj = (size_t)1024 * k * sizeof(float);
    const int batch_parts = whole ? 0 : (int)std::max<size_t>(cap / (part_lj + m_least), 1);
    const size_t lj_bytes = ((whole ? lj_full : batch_parts * part_lj) + 255) / 256 * 256;   // rounded UP: the partials lie past lj's last entry
    const size_t m_bytes = whole ? std::max(std::min(m_full, cap - lj_full), m_least) : (size_t)batch_parts * m_least;
    unsigned char *d_scr = d_gm_scratch.need(e_bytes + lj_bytes + m_bytes);
    float *d_lj = (float *)(d_scr + e_bytes);
    unsigned char *d_mscr = d_scr + e_bytes + lj_bytes;

    // the first responsibilities: a hard assignment — the clustering's, or to the nearest of the given means
    if (init != GMM_INIT_KMEANS) {
        float *d_centres = d_km_centers.need((size_t)k * dim), *d_cn = d_km_cn.need((size_t)k);
        if (init == GMM_INIT_POSITIONS) {
            std::vector<int32_t> at((size_t)k);
            for (int c = 0; c < k; c++) at[c] = rows[init_pos[c]];
            int32_t *d_pos = d_km_pos.need((size_t)k);
            GCNHIP_CHECK(gcnhip_h2d(ctx, d_pos, at.data(), at.size() * sizeof(int32_t)));
            GCNHIP_CHECK(gcnhip_embed_rows(ctx, t.data, t.ld, t.rows, dim, t.inv_norm, d_pos, k, d_centres, dim));
        } else {
            GCNHIP_CHECK(gcnhip_h2d(ctx, d_centres, init_means, (size_t)k * dim * sizeof(float)));
        }
        size_t km_least = 0;
        if (gcnhip_kmeans_plan(0, k, dim, nullptr, &km_least, nullptr) != 0) throw GcnHipFailure(-1, std::string(what) + ": " + gcnhip_last_error());
        GCNHIP_CHECK(gcnhip_kmeans_update(ctx, t.data, t.ld, t.rows, dim, t.inv_norm, d_rows, 0, nullptr, nullptr, k, d_centres, dim, d_km_sizes.need((size_t)k),
                                          d_cn, nullptr, d_km_scratch.need(km_least), km_least));
        GCNHIP_CHECK(gcnhip_kmeans_assign(ctx, t.data, t.ld, t.rows, dim, t.inv_norm, d_rows, n, d_centres, dim, d_cn, k, nullptr, d_assign, d_km_dist.need(nn),
                                          d_km_flag.need(2)));
        centres.resize((size_t)k * dim);
        GCNHIP_CHECK(gcnhip_d2h(ctx, centres.data(), d_centres, centres.size() * sizeof(float)));
    } else {
        GCNHIP_CHECK(gcnhip_h2d(ctx, d_assign, first.data(), nn * sizeof(int32_t)));
    }
    // what a component the first M-step does not fit keeps: its centre, unit variances, no weight
    std::vector<float> par((size_t)k * B.ldc, 0.f), ones((size_t)k * B.ldc, 1.f), zeros((size_t)B.k4, 0.f);
    for (int c = 0; c < k; c++)
        for (int j = 0; j < dim; j++) par[(size_t)c * B.ldc + j] = centres[(size_t)c * dim + j] - sh[j];
    GCNHIP_CHECK(gcnhip_h2d(ctx, B.mu, par.data(), par.size() * sizeof(float)));
    GCNHIP_CHECK(gcnhip_h2d(ctx, B.var, ones.data(), ones.size() * sizeof(float)));
    GCNHIP_CHECK(gcnhip_h2d(ctx, B.weights, zeros.data(), zeros.size() * sizeof(float)));
    GCNHIP_CHECK(gcnhip_gmm_finalize(ctx, nullptr, n, k, dim, spherical, reg_covar, B.mu, B.var, B.weights, B.prec, B.mprec, B.ldc, B.cst));
    GCNHIP_CHECK(gcnhip_gmm_mstep(ctx, t.data, t.ld, t.rows, dim, t.inv_norm, d_rows, n, B.shift, nullptr, nullptr, d_assign, k, 0, n, d_sums, d_mscr, m_bytes));
    GCNHIP_CHECK(gcnhip_gmm_finalize(ctx, d_sums, n, k, dim, spherical, reg_covar, B.mu, B.var, B.weights, B.prec, B.mprec, B.ldc, B.cst));

    double prev = -INFINITY;
    for (int it = 0; it < iters; it++) {
        GCNHIP_CHECK(gcnhip_gmm_estep(ctx, t.data, t.ld, t.rows, dim, t.inv_norm, d_rows, n, B.shift, B.prec, B.mprec, B.ldc, B.cst, k, B.lse, d_assign,
                                      B.max_resp, whole ? d_lj : nullptr, d_lsum + it, d_scr, e_bytes));
        if (whole) {
            GCNHIP_CHECK(gcnhip_gmm_mstep(ctx, t.data, t.ld, t.rows, dim, t.inv_norm, d_rows, n, B.shift, d_lj, B.lse, nullptr, k, 0, n, d_sums, d_mscr, m_bytes));
        } else {
            for (int p0 = 0; p0 < n; p0 += batch_parts * 1024) {   // the E-step again, a batch of parts at a time: the same bits
                const int p1 = (int)std::min<int64_t>(n, (int64_t)p0 + (int64_t)batch_parts * 1024);
                GCNHIP_CHECK(gcnhip_gmm_estep(ctx, t.data, t.ld, t.rows, dim, t.inv_norm, d_rows + p0, p1 - p0, B.shift, B.prec, B.mprec, B.ldc, B.cst, k,
                                              B.lse + p0, d_assign + p0, B.max_resp + p0, d_lj, nullptr, nullptr, 0));
                GCNHIP_CHECK(gcnhip_gmm_mstep(ctx, t.data, t.ld, t.rows, dim, t.inv_norm, d_rows, n, B.shift, d_lj, B.lse, nullptr, k, p0, p1, d_sums, d_mscr,
                                              m_bytes));
            }
        }
        GCNHIP_CHECK(gcnhip_gmm_finalize(ctx, d_sums, n, k, dim, spherical, reg_covar, B.mu, B.var, B.weights, B.prec, B.mprec, B.ldc, B.cst));
        double sum = 0;
        GCNHIP_CHECK(gcnhip_d2h(ctx, &sum, d_lsum + it, sizeof(double)));      // the eight bytes of an iteration
        const double lb = sum / (double)n;
        if (history) { history[2 * it] = (double)(it + 1); history[2 * it + 1] = lb; }
        res.iters_run = it + 1;
        res.lower_bound = lb;
        const bool done = std::fabs(lb - prev) < tol;
        prev = lb;
        if (done) { res.converged = true; break; }
    }
    // the fit as it is handed back: the shift added once.  The last E-step runs on exactly these numbers, as gmm_score() will.
    std::vector<float> mu((size_t)k * B.ldc), var((size_t)k * B.ldc), wt((size_t)B.k4);
    GCNHIP_CHECK(gcnhip_d2h(ctx, mu.data(), B.mu, mu.size() * sizeof(float)));
    GCNHIP_CHECK(gcnhip_d2h(ctx, var.data(), B.var, var.size() * sizeof(float)));
    GCNHIP_CHECK(gcnhip_d2h(ctx, wt.data(), B.weights, wt.size() * sizeof(float)));
    std::vector<float> mean_out((size_t)k * dim), var_out((size_t)k * dim);
    for (int c = 0; c < k; c++)
        for (int j = 0; j < dim; j++) {
            mean_out[(size_t)c * dim + j] = mu[(size_t)c * B.ldc + j] + sh[j];
            var_out[(size_t)c * dim + j] = var[(size_t)c * B.ldc + j];
        }
    if (sizes) {
        std::vector<double> sums((size_t)k * W);
        GCNHIP_CHECK(gcnhip_d2h(ctx, sums.data(), d_sums, sums.size() * sizeof(double)));
        for (int c = 0; c < k; c++) sizes[c] = sums[(size_t)c * W];
    }
    gmm_estep_fit(t, d_rows, n, k, wt.data(), mean_out.data(), var_out.data(), sh.data(), B.lse, d_assign, B.max_resp, log_likelihood, assign, max_resp, resp);
    if (weights) std::copy(wt.begin(), wt.begin() + k, weights);
    if (means) std::copy(mean_out.begin(), mean_out.end(), means);
    if (variances) std::copy(var_out.begin(), var_out.end(), variances);
    if (shift) std::copy(sh.begin(), sh.begin() + dim, shift);
    if (contingency) {
        if (!d_label_all) d_label_all = arena.upload(m.data->label.data() + m.row_start(), (size_t)m.n_local);
        int32_t *d_counts = d_km_counts.need((size_t)k * C + 1);
        GCNHIP_CHECK(gcnhip_contingency_rows(ctx, d_assign, d_label_all, m.n_local, d_rows, n, k, C, d_counts, d_counts + (size_t)k * C));
        std::vector<int32_t> cnt((size_t)k * C + 1);
        GCNHIP_CHECK(gcnhip_d2h(ctx, cnt.data(), d_counts, cnt.size() * sizeof(int32_t)));
        for (size_t e = 0; e < (size_t)k * C; e++) contingency[e] = cnt[e];
        res.skipped = cnt[(size_t)k * C];
    }
    m.sync();
    return res;
}

// One E-step of the uploaded list under a fit as it is handed back (weights [k], means / variances [k x dim], shift [dim]): the
// operands from mu' = means - shift (f32), then the launch and the copies.  d_lse / d_assign / d_max_resp: device [n].
void ModelQueries::gmm_estep_fit(const EmbedTable &t, const int32_t *d_rows, int n, int k, const float *weights, const float *means, const float *variances,
                                 const float *shift, float *d_lse, int32_t *d_assign, float *d_max_resp, float *log_likelihood, int32_t *assign,
                                 float *max_resp, float *resp) {
    gcnhip_ctx *ctx = m.env.ctx;
    const int dim = t.dim;
    const size_t nn = (size_t)n;
    GmmBlock P(d_gm_fit.need(GmmBlock::floats(k, dim, 0)), k, dim, 0);
    std::vector<float> mu((size_t)k * P.ldc, 0.f), var((size_t)k * P.ldc, 1.f), wt((size_t)P.k4, 0.f), sh((size_t)P.ldc, 0.f);
    std::copy(shift, shift + dim, sh.begin());
    std::copy(weights, weights + k, wt.begin());
    for (int c = 0; c < k; c++)
        for (int j = 0; j < dim; j++) {
            mu[(size_t)c * P.ldc + j] = means[(size_t)c * dim + j] - shift[j];
            var[(size_t)c * P.ldc + j] = variances[(size_t)c * dim + j];
        }
    GCNHIP_CHECK(gcnhip_h2d(ctx, P.shift, sh.data(), sh.size() * sizeof(float)));
    GCNHIP_CHECK(gcnhip_h2d(ctx, P.mu, mu.data(), mu.size() * sizeof(float)));
    GCNHIP_CHECK(gcnhip_h2d(ctx, P.var, var.data(), var.size() * sizeof(float)));
    GCNHIP_CHECK(gcnhip_h2d(ctx, P.weights, wt.data(), wt.size() * sizeof(float)));
    GCNHIP_CHECK(gcnhip_gmm_finalize(ctx, nullptr, n, k, dim, 0, 1.0, P.mu, P.var, P.weights, P.prec, P.mprec, P.ldc, P.cst));
    float *d_lj = resp ? d_gm_resp.need(nn * k) : nullptr;
    GCNHIP_CHECK(gcnhip_gmm_estep(ctx, t.data, t.ld, t.rows, dim, t.inv_norm, d_rows, n, P.shift, P.prec, P.mprec, P.ldc, P.cst, k, d_lse, d_assign, d_max_resp,
                                  d_lj, nullptr, nullptr, 0));
    std::vector<float> lse(nn);
    GCNHIP_CHECK(gcnhip_d2h(ctx, lse.data(), d_lse, nn * sizeof(float)));
    if (log_likelihood) std::copy(lse.begin(), lse.end(), log_likelihood);
    if (assign) GCNHIP_CHECK(gcnhip_d2h(ctx, assign, d_assign, nn * sizeof(int32_t)));
    if (max_resp) GCNHIP_CHECK(gcnhip_d2h(ctx, max_resp, d_max_resp, nn * sizeof(float)));
    if (resp) {                                                // r = exp(lj - lse), the log joint brought over once
        GCNHIP_CHECK(gcnhip_d2h(ctx, resp, d_lj, nn * k * sizeof(float)));
        for (size_t i = 0; i < nn; i++)
            for (int c = 0; c < k; c++) resp[i * k + c] = std::exp(resp[i * k + c] - lse[i]);
    }
}

int64_t ModelQueries::gmm_score(int k, int width, const float *weights, const float *means, const float *variances, const float *shift, int split,
                                const int *nodes, int n, const float *data, int data_dim, bool normalize, float *log_likelihood, int32_t *assign,
                                float *max_resp, float *resp, int64_t capacity) {
    const char *what = "gmm_score";
    const std::string w = std::string(what) + ": ";
    std::vector<int> rows;
    const int64_t listed = gmm_rows(what, k, split, nodes, n, data, data_dim, &rows);
    if (capacity >= 0 && listed > capacity)
        throw GcnHipFailure(-1, w + "the query lists " + std::to_string(listed) + " rows, the outputs have room for " + std::to_string(capacity));
    const int dim = data ? data_dim : m.params.hidden_dim;
    if (width != dim) throw GcnHipFailure(-1, w + "the fit is of width " + std::to_string(width) + ", the rows of width " + std::to_string(dim));
    if (!weights || !means || !variances || !shift) throw GcnHipFailure(-1, w + "invalid argument (the fit's weights, means, variances and shift)");
    for (int c = 0; c < k; c++)
        if (!(weights[c] >= 0.f) || !std::isfinite(weights[c])) throw GcnHipFailure(-1, w + "the fit is not finite (weights)");
    for (size_t e = 0; e < (size_t)k * dim; e++)
        if (!std::isfinite(means[e]) || !(variances[e] > 0.f) || !std::isfinite(variances[e]))
            throw GcnHipFailure(-1, w + "the fit is not finite (means, or variances that are not above 0)");
    for (int j = 0; j < dim; j++)
        if (!std::isfinite(shift[j])) throw GcnHipFailure(-1, w + "the fit is not finite (shift)");
    n = (int)rows.size();
    m.sync();
    const size_t nn = (size_t)n;
    int32_t *d_rows = d_gm_int.need(2 * nn), *d_assign = d_rows + nn;
    const EmbedTable t = gmm_table(rows, data, data_dim, normalize, d_rows);
    if (n > 0) {
        float *d_out = d_gm_f32.need(2 * nn);
        gmm_estep_fit(t, d_rows, n, k, weights, means, variances, shift, d_out, d_assign, d_out + nn, log_likelihood, assign, max_resp, resp);
    }
    m.sync();
    return n;
}
