// mmd_query.cpp — ModelQueries::mmd: the kernel two-sample sums of two groups of rows of the hidden layer of a trained model (or of a
// caller's table), where they lie (queries.h has the contract, include/gcnhip_driver.h the definitions, csrc/mmd.hip the kernels,
// mmd.h the statistics).  Off the epoch path: the hidden layer comes from embed_forward, the walk is composed here from the library's
// entry points, and no training module is touched.
#include "queries.h"
#include "gcn.h"
#include "hip_check.h"
#include <algorithm>
#include <cmath>
#include <numeric>

// every refusal, before any launch; the rows of the list (group A's m_a positions first)
int64_t ModelQueries::mmd_check(const int *nodes, int n, int m_a, const float *data, int data_dim, const double *gamma, int n_gamma,
                                const uint8_t *perm_bits, int permutations, std::vector<int> *rows) {
    const char *what = "mmd";
    const std::string w = std::string(what) + ": ";
    require(what, ONE_RANK);
    if (m.flags & HIPGCN_BF16_TABLES) throw GcnHipFailure(-1, w + "not with bf16 tables (the kernels read the f32 rows of the hidden layer)");
    if (n < 0 || m_a < 0 || n_gamma < 0 || (n_gamma > 0 && !gamma)) throw GcnHipFailure(-1, w + "invalid argument");
    if (permutations < 0) throw GcnHipFailure(-1, w + "permutations must be at least 0, got " + std::to_string(permutations));
    if (permutations > 0 && !perm_bits) throw GcnHipFailure(-1, w + "invalid argument (the permutations' bits are missing)");
    if (n_gamma > MMD_MAX_GAMMAS) throw GcnHipFailure(-1, w + "at most 4 values of gamma, got " + std::to_string(n_gamma));
    for (int g = 0; g < n_gamma; g++)
        if (!(gamma[g] > 0.0) || !std::isfinite(gamma[g]) || !((float)gamma[g] > 0.f) || !std::isfinite((float)gamma[g]))
            throw GcnHipFailure(-1, w + "gamma must be finite and above 0 (in f32 too), got " + std::to_string(gamma[g]));
    if (m_a < 1 || m_a >= n) throw GcnHipFailure(-1, w + "an empty group (" + std::to_string(m_a) + " and " + std::to_string(n - m_a) + " rows)");
    std::vector<int> list;
    if (data) {
        if (nodes) throw GcnHipFailure(-1, w + "with data the rows are the data's: no node query");
        if (data_dim < 1 || data_dim > 256) throw GcnHipFailure(-1, w + "data of a width in 1..256, got " + std::to_string(data_dim));
        list.resize((size_t)n);
        std::iota(list.begin(), list.end(), 0);
    } else {
        if (m.params.hidden_dim < 1 || m.params.hidden_dim > 256)
            throw GcnHipFailure(-1, w + "a hidden width of at most 256 (the walk keeps a row's operand in registers)");
        if (!nodes) throw GcnHipFailure(-1, w + "invalid argument (the nodes of the two groups are missing)");
        int listed = n;
        list = kmeans_list(what, 0, nodes, listed);             // a node id outside the graph is refused here
        std::vector<char> in_a((size_t)m.n_local, 0);
        for (int i = 0; i < m_a; i++) in_a[list[i]] = 1;
        for (int i = m_a; i < n; i++)
            if (in_a[list[i]]) throw GcnHipFailure(-1, w + "the groups overlap: node " + std::to_string(nodes[i]) + " is in both");
    }
    if (rows) *rows = std::move(list);
    return n;
}

ModelQueries::Mmd ModelQueries::mmd(const int *nodes, int n, int m_a, const float *data, int data_dim, bool normalize, const double *gamma, int n_gamma,
                                    const uint8_t *perm_bits, int permutations, bool want_witness, size_t scratch_bytes, double *sums, float *witness,
                                    double *gamma_used) {
    const char *what = "mmd";
    Mmd res;
    std::vector<int> rows;
    res.rows = mmd_check(nodes, n, m_a, data, data_dim, gamma, n_gamma, perm_bits, permutations, &rows);
    gcnhip_ctx *ctx = m.env.ctx;
    const size_t nn = (size_t)n;
    m.sync();                                                  // run()'s epochs in flight, the validation lane's pass
    int32_t *d_rows = d_mmd_int.need(nn + 2), *d_counts = d_rows + nn;
    EmbedTable t;
    if (data) {
        float *d = d_mmd_data.need(nn * (size_t)data_dim);
        GCNHIP_CHECK(gcnhip_h2d(ctx, d, data, nn * (size_t)data_dim * sizeof(float)));
        t = EmbedTable{d, data_dim, n, data_dim, nullptr};
    } else {
        t = embed_forward(normalize);
    }
    GCNHIP_CHECK(gcnhip_h2d(ctx, d_rows, rows.data(), nn * sizeof(int32_t)));
    const int dim = t.dim, cols = 1 + permutations;
    const auto fail = [&]() { return GcnHipFailure(-1, std::string(what) + ": " + gcnhip_last_error()); };

    // the shift: the f32-rounded float64 mean of the listed rows; the default gamma: 1 / the mean of d2 over the pairs of distinct rows
    // = (n - 1) / (2 trace(scatter)), the scatter about that mean in float64
    size_t pca_full = 0, pca_least = 0;
    if (gcnhip_pca_plan(n, dim, &pca_full, &pca_least) != 0) throw fail();
    double *d_mean = d_mmd_f64.need((size_t)dim + (size_t)dim * dim + 3 * 256), *d_scatter = d_mean + dim, *d_sums = d_scatter + (size_t)dim * dim;
    unsigned char *d_pscr = d_pca_scratch.need(pca_least);
    GCNHIP_CHECK(gcnhip_pca_mean(ctx, t.data, t.ld, t.rows, dim, t.inv_norm, d_rows, n, d_mean, d_pca_count.need(1), d_pscr, pca_least));
    std::vector<double> mean64((size_t)dim);
    GCNHIP_CHECK(gcnhip_d2h(ctx, mean64.data(), d_mean, (size_t)dim * sizeof(double)));
    std::vector<float> sh((size_t)dim);
    for (int j = 0; j < dim; j++) sh[j] = (float)mean64[j];
    float *d_shift = d_mmd_f32.need((size_t)dim + nn), *d_wit = d_shift + dim;
    GCNHIP_CHECK(gcnhip_h2d(ctx, d_shift, sh.data(), sh.size() * sizeof(float)));
    std::vector<double> gammas(gamma, gamma + n_gamma);
    if (gammas.empty()) {
        GCNHIP_CHECK(gcnhip_pca_scatter(ctx, t.data, t.ld, t.rows, dim, t.inv_norm, d_rows, n, d_mean, d_scatter, d_pscr, pca_least));
        std::vector<double> sc((size_t)dim * dim);
        GCNHIP_CHECK(gcnhip_d2h(ctx, sc.data(), d_scatter, sc.size() * sizeof(double)));
        double trace = 0;
        for (int j = 0; j < dim; j++) trace += sc[(size_t)j * dim + j];
        const double g = (double)(n - 1) / (2.0 * trace);
        if (!(g > 0.0) || !std::isfinite(g) || !std::isfinite((float)g))
            throw GcnHipFailure(-1, std::string(what) + ": the rows do not differ, so there is no default gamma (1 / the mean squared distance): give one");
        gammas.push_back(g);
    }
    res.n_gamma = (int)gammas.size();

    // per gamma and per chunk of at most 254 permutations: S = {ones | group A | the chunk's groups}, the walk, the fold
    uint8_t *d_bits = d_mmd_bits.need(nn * 32);
    std::vector<uint8_t> bits;
    std::vector<double> part(3 * 256);
    const int pb = (permutations + 7) / 8;
    for (size_t g = 0; g < gammas.size(); g++) {
        const float gf = (float)gammas[g];
        if (gamma_used) gamma_used[g] = (double)gf;
        for (int p0 = 0; p0 == 0 || p0 < permutations; p0 += MMD_CHUNK) {
            const int chunk = std::min(MMD_CHUNK, permutations - p0), Bp = (2 + chunk + 15) / 16 * 16, bw = Bp / 8;
            const bool wit = want_witness && p0 == 0;
            bits.assign(nn * bw, 0);
            for (size_t i = 0; i < nn; i++) {
                uint8_t *row = bits.data() + i * bw;
                row[0] = (uint8_t)(1 | ((int)i < m_a ? 2 : 0));
                for (int p = 0; p < chunk; p++)
                    if ((perm_bits[i * pb + ((p0 + p) >> 3)] >> ((p0 + p) & 7)) & 1) row[(2 + p) >> 3] |= (uint8_t)(1 << ((2 + p) & 7));
            }
            GCNHIP_CHECK(gcnhip_h2d(ctx, d_bits, bits.data(), bits.size()));
            size_t full = 0, least = 0;
            if (gcnhip_mmd_plan(n, dim, Bp, wit, &full, &least) != 0) throw fail();
            const size_t bytes = std::max(std::min(full, scratch_bytes ? scratch_bytes : MMD_SCRATCH_DEFAULT), least);
            unsigned char *d_scr = d_mmd_scratch.need(bytes);
            GCNHIP_CHECK(gcnhip_mmd_walk(ctx, t.data, t.ld, t.rows, dim, t.inv_norm, d_rows, n, d_shift, gf, d_bits, Bp, wit, d_scr, bytes));
            GCNHIP_CHECK(gcnhip_mmd_fold(ctx, n, dim, Bp, wit, d_scr, bytes, d_sums, d_counts, wit ? d_wit : nullptr));
            GCNHIP_CHECK(gcnhip_d2h(ctx, part.data(), d_sums, 3 * (size_t)Bp * sizeof(double)));
            int32_t counts[2] = {0, 0};
            GCNHIP_CHECK(gcnhip_d2h(ctx, counts, d_counts, sizeof counts));
            res.m = counts[1];
            res.rest = counts[0] - counts[1];
            if (sums)                                          // [gamma][AA | AB | BB][observed, the permutations]
                for (int qv = 0; qv < 3; qv++) {
                    double *dst = sums + (g * 3 + qv) * (size_t)cols;
                    if (p0 == 0) dst[0] = part[(size_t)qv * Bp + 1];
                    for (int p = 0; p < chunk; p++) dst[1 + p0 + p] = part[(size_t)qv * Bp + 2 + p];
                }
            if (wit && witness) GCNHIP_CHECK(gcnhip_d2h(ctx, witness + g * nn, d_wit, nn * sizeof(float)));
        }
    }
    m.sync();
    return res;
}
