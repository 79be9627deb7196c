// pca_query.cpp — ModelQueries::pca_fit / pca_project: principal components of the hidden layer of a trained model, where it lies
// (queries.h has the contract, csrc/pca.hip the definitions and the kernels, pca.h the eigenproblem and what is derived from it).
// Off the epoch path: the hidden layer comes from embed_forward and no training module is touched.
#include "queries.h"
#include "gcn.h"
#include "hip_check.h"
#include "pca.h"
#include <algorithm>
#include <cmath>

int64_t ModelQueries::pca_rows(int k, int split, const int *nodes, int n, std::vector<int> *rows) {
    const char *what = "pca";
    const std::string w = std::string(what) + ": ";
    require(what, ONE_RANK);
    if (m.flags & HIPGCN_BF16_TABLES) throw GcnHipFailure(-1, w + "not with bf16 tables (the kernels read the f32 rows of the hidden layer)");
    if (m.params.hidden_dim < 1 || m.params.hidden_dim > 256)
        throw GcnHipFailure(-1, w + "a hidden width of at most 256 (the scatter kernel keeps a workgroup's tiles in registers)");
    if (split < 0 || split > 3) throw GcnHipFailure(-1, w + "invalid argument (split is 0 with a node query, or 1 train, 2 validation, 3 test)");
    if (n < 0) throw GcnHipFailure(-1, w + "invalid argument");
    if (k < 1 || k > m.params.hidden_dim) throw GcnHipFailure(-1, w + "k must be in 1.." + std::to_string(m.params.hidden_dim) + ", got " + std::to_string(k));
    int listed = n;
    std::vector<int> list = kmeans_list(what, split, nodes, listed);   // a node id outside the graph is refused here
    if (listed < 2) throw GcnHipFailure(-1, w + "at least 2 rows, the query lists " + std::to_string(listed));
    if (rows) *rows = std::move(list);
    return listed;
}

ModelQueries::Pca ModelQueries::pca_fit(int k, int split, const int *nodes, int n, bool normalize, bool center, bool whiten, size_t scratch_bytes,
                                        double *mean, double *scatter, double *eigenvalues, double *components, double *explained,
                                        double *scale, float *coords) {
    Pca res;
    std::vector<int> rows;
    res.rows = pca_rows(k, split, nodes, n, &rows);            // every refusal, before any launch; the list is made once
    res.k = k;
    n = (int)rows.size();
    m.sync();                                                  // run()'s epochs in flight, the validation lane's pass
    const EmbedTable t = embed_forward(normalize);
    gcnhip_ctx *ctx = m.env.ctx;
    const size_t nn = (size_t)n, h = (size_t)t.dim;
    size_t full = 0, least = 0;
    if (gcnhip_pca_plan(n, t.dim, &full, &least) != 0) throw GcnHipFailure(-1, std::string("pca: ") + gcnhip_last_error());
    const size_t bytes = scratch_bytes ? std::max(std::min(full, scratch_bytes), least) : full;
    unsigned char *d_scr = d_pca_scratch.need(bytes);
    int32_t *d_rows = d_pca_rows.need(nn), *d_count = d_pca_count.need(1);
    double *d_mean = d_pca_stats.need(h + h * h), *d_scatter = d_mean + h;
    GCNHIP_CHECK(gcnhip_h2d(ctx, d_rows, rows.data(), nn * sizeof(int32_t)));
    // the count the mean call also writes is not read back: every listed id was checked, so it is res.rows
    if (center) GCNHIP_CHECK(gcnhip_pca_mean(ctx, t.data, t.ld, t.rows, t.dim, t.inv_norm, d_rows, n, d_mean, d_count, d_scr, bytes));
    GCNHIP_CHECK(gcnhip_pca_scatter(ctx, t.data, t.ld, t.rows, t.dim, t.inv_norm, d_rows, n, center ? d_mean : nullptr, d_scatter, d_scr, bytes));
    std::vector<double> stats(h + h * h, 0.0);                 // h + h . h doubles: all the fit brings to the host
    if (center) GCNHIP_CHECK(gcnhip_d2h(ctx, stats.data(), d_mean, (h + h * h) * sizeof(double)));
    else GCNHIP_CHECK(gcnhip_d2h(ctx, stats.data() + h, d_scatter, h * h * sizeof(double)));
    PcaFit fit;
    std::string why;
    if (gcn_pca_from_scatter(stats.data() + h, stats.data(), res.rows, t.dim, k, whiten, &fit, &why) != 0) throw GcnHipFailure(-1, "pca: " + why);
    res.rank = fit.rank;
    if (mean) std::copy(stats.begin(), stats.begin() + h, mean);
    if (scatter) std::copy(stats.begin() + h, stats.end(), scatter);
    if (eigenvalues) std::copy(fit.eigenvalues.begin(), fit.eigenvalues.end(), eigenvalues);
    if (components)
        for (size_t j = 0; j < h; j++)
            for (size_t a = 0; a < h; a++) components[j * h + a] = fit.components[a * h + j];
    if (explained) {
        std::copy(fit.explained_variance.begin(), fit.explained_variance.end(), explained);
        std::copy(fit.explained_variance_ratio.begin(), fit.explained_variance_ratio.end(), explained + h);
        std::copy(fit.singular_values.begin(), fit.singular_values.end(), explained + 2 * h);
    }
    if (scale && whiten) std::copy(fit.scale.begin(), fit.scale.end(), scale);
    if (coords) {
        std::vector<double> basis(h * (size_t)k + (size_t)k, 0.0);
        for (size_t a = 0; a < h; a++)
            for (int j = 0; j < k; j++) basis[a * k + j] = fit.components[a * h + j];
        if (whiten) std::copy(fit.scale.begin(), fit.scale.end(), basis.begin() + h * k);
        double *d_basis = d_pca_basis.need(basis.size());
        float *d_out = d_pca_out.need(nn * k);
        GCNHIP_CHECK(gcnhip_h2d(ctx, d_basis, basis.data(), basis.size() * sizeof(double)));
        GCNHIP_CHECK(gcnhip_pca_project(ctx, t.data, t.ld, t.rows, t.dim, t.inv_norm, d_rows, n, center ? d_mean : nullptr, d_basis, k, k,
                                        whiten ? d_basis + h * k : nullptr, d_out, k));
        GCNHIP_CHECK(gcnhip_d2h(ctx, coords, d_out, nn * k * sizeof(float)));
    }
    m.sync();
    return res;
}

int64_t ModelQueries::pca_project(int width, int k, const double *mean, const double *components, const double *scale, bool normalize, const int *nodes,
                                  int n, float *out) {
    const char *what = "pca_transform";
    const std::string w = std::string(what) + ": ";
    require(what, ONE_RANK);
    if (m.flags & HIPGCN_BF16_TABLES) throw GcnHipFailure(-1, w + "not with bf16 tables (the kernels read the f32 rows of the hidden layer)");
    if (width != m.params.hidden_dim || width > 256)
        throw GcnHipFailure(-1, w + "the fit is of width " + std::to_string(width) + ", the hidden layer of width " + std::to_string(m.params.hidden_dim));
    if (k < 1 || k > width || !components || n < 0) throw GcnHipFailure(-1, w + "invalid argument (k components of 1..hidden, a node query)");
    const size_t h = (size_t)width;
    for (size_t e = 0; e < (size_t)k * h; e++)
        if (!std::isfinite(components[e])) throw GcnHipFailure(-1, w + "the fit is not finite (components)");
    for (size_t a = 0; mean && a < h; a++)
        if (!std::isfinite(mean[a])) throw GcnHipFailure(-1, w + "the fit is not finite (mean)");
    for (int j = 0; scale && j < k; j++)
        if (!std::isfinite(scale[j])) throw GcnHipFailure(-1, w + "the fit is not finite (scale)");
    const std::vector<int> rows = embed_query(what, nodes, n);  // a node id outside the graph is refused here
    if (n > 0 && !out) throw GcnHipFailure(-1, w + "invalid argument");
    m.sync();
    const EmbedTable t = embed_forward(normalize);
    if (n == 0) { m.sync(); return 0; }
    gcnhip_ctx *ctx = m.env.ctx;
    const size_t nn = (size_t)n;
    std::vector<double> block(h + h * k + (size_t)k, 0.0);     // {mean | basis [h x k] | scale}
    if (mean) std::copy(mean, mean + h, block.begin());
    for (size_t a = 0; a < h; a++)
        for (int j = 0; j < k; j++) block[h + a * k + j] = components[(size_t)j * h + a];
    if (scale) std::copy(scale, scale + k, block.begin() + h + h * k);
    double *d_block = d_pca_basis.need(block.size());
    int32_t *d_rows = d_pca_rows.need(nn);
    float *d_out = d_pca_out.need(nn * k);
    GCNHIP_CHECK(gcnhip_h2d(ctx, d_block, block.data(), block.size() * sizeof(double)));
    GCNHIP_CHECK(gcnhip_h2d(ctx, d_rows, rows.data(), nn * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_pca_project(ctx, t.data, t.ld, t.rows, t.dim, t.inv_norm, d_rows, n, mean ? d_block : nullptr, d_block + h, k, k,
                                    scale ? d_block + h + h * k : nullptr, d_out, k));
    GCNHIP_CHECK(gcnhip_d2h(ctx, out, d_out, nn * k * sizeof(float)));
    m.sync();
    return n;
}
