// dbscan_query.cpp — ModelQueries::dbscan / neighbor_counts: the density clusters and the noise of the hidden layer of a trained
// model (or of a caller's table), where it lies (queries.h has the contract, include/gcnhip_driver.h the definitions,
// csrc/dbscan.hip the kernels).  Off the epoch path: the hidden layer comes from embed_forward and no training module is touched.
#include "queries.h"
#include "gcn.h"
#include "hip_check.h"
#include <algorithm>
#include <cmath>

int64_t ModelQueries::dbscan_rows(const char *what, int split, const int *nodes, int n, const float *data, int data_dim, const double *eps, int n_eps,
                                  int min_samples, std::vector<int> *rows) {
    const std::string w = std::string(what) + ": ";
    require(what, ONE_RANK);
    if (m.flags & HIPGCN_BF16_TABLES) throw GcnHipFailure(-1, w + "not with bf16 tables (the kernels read the f32 rows of the hidden layer)");
    if (n_eps < 1 || n_eps > 8 || !eps) throw GcnHipFailure(-1, w + "between 1 and 8 radii, got " + std::to_string(n_eps));
    for (int e = 0; e < n_eps; e++)
        if (!(eps[e] > 0.0) || !std::isfinite(eps[e]) || !std::isfinite((float)(eps[e] * eps[e])))
            throw GcnHipFailure(-1, w + "eps must be finite and above 0, got " + std::to_string(eps[e]));
    if (min_samples < 1) throw GcnHipFailure(-1, w + "min_samples must be at least 1, got " + std::to_string(min_samples));
    if (n < 0) throw GcnHipFailure(-1, w + "invalid argument");
    if (data) {
        if (split != 0 || nodes) throw GcnHipFailure(-1, w + "with data the rows are the data's: no split and no node query");
        if (data_dim < 1 || data_dim > 256) throw GcnHipFailure(-1, w + "data of a width in 1..256, got " + std::to_string(data_dim));
        return n;
    }
    if (m.params.hidden_dim < 1 || m.params.hidden_dim > 256)
        throw GcnHipFailure(-1, w + "a hidden width of at most 256 (the walk keeps a tile of rows in registers)");
    if (split < 0 || split > 3) throw GcnHipFailure(-1, w + "invalid argument (split is 0 with a node query, or 1 train, 2 validation, 3 test)");
    int listed = n;
    std::vector<int> list = kmeans_list(what, split, nodes, listed);   // a node id outside the graph is refused here
    if (rows) *rows = std::move(list);
    return listed;
}

ModelQueries::Dbscan ModelQueries::dbscan_run(const char *what, const double *eps, int n_eps, int min_samples, int split, const int *nodes, int n,
                                              const float *data, int data_dim, bool normalize, int32_t *labels, uint8_t *core, int32_t *count,
                                              int32_t *sizes, int64_t *contingency) {
    Dbscan res;
    std::vector<int> rows;
    res.rows = dbscan_rows(what, split, nodes, n, data, data_dim, eps, n_eps, std::max(min_samples, 1), &rows);   // every refusal that needs no GPU
    n = (int)res.rows;
    if (n < 1) throw GcnHipFailure(-1, std::string(what) + ": invalid argument (no rows)");
    m.sync();                                                  // run()'s epochs in flight, the validation lane's pass
    gcnhip_ctx *ctx = m.env.ctx;
    const size_t nn = (size_t)n;
    // {rows | count [E x n] | labels | sizes [n] | totals [5] | points | flags [DBSCAN_BATCH]}
    int32_t *d_int = d_db_int.need(nn * (size_t)(3 + n_eps) + 6 + DBSCAN_BATCH), *d_count = d_int + nn, *d_labels = d_count + nn * (size_t)n_eps,
            *d_sizes = d_labels + nn, *d_totals = d_sizes + nn, *d_points = d_totals + 5, *d_flags = d_points + 1;
    EmbedTable t;
    const int32_t *d_rows = nullptr;
    if (data) {
        float *d = d_db_data.need(nn * (size_t)data_dim);
        GCNHIP_CHECK(gcnhip_h2d(ctx, d, data, nn * (size_t)data_dim * sizeof(float)));
        t = EmbedTable{d, data_dim, n, data_dim, nullptr};
    } else {
        t = embed_forward(normalize);
        GCNHIP_CHECK(gcnhip_h2d(ctx, d_int, rows.data(), nn * sizeof(int32_t)));
        d_rows = d_int;
    }
    size_t pack_bytes = 0, state_bytes = 0;
    if (gcnhip_dbscan_plan(n, t.dim, &pack_bytes, &state_bytes) != 0) throw GcnHipFailure(-1, std::string(what) + ": " + gcnhip_last_error());
    unsigned char *d_pack = d_db_pack.need(pack_bytes), *d_state = d_db_state.need(state_bytes), *d_core = d_db_core.need(nn);

    GCNHIP_CHECK(gcnhip_tsne_pack(ctx, t.data, t.ld, t.rows, t.dim, t.inv_norm, d_rows, n, d_pack, pack_bytes, d_points));
    GCNHIP_CHECK(gcnhip_dbscan_counts(ctx, d_pack, n, t.dim, eps, n_eps, d_count));
    int32_t points = 0;
    GCNHIP_CHECK(gcnhip_d2h(ctx, &points, d_points, sizeof(int32_t)));
    if (count) GCNHIP_CHECK(gcnhip_d2h(ctx, count, d_count, nn * (size_t)n_eps * sizeof(int32_t)));
    if (min_samples < 1) {
        m.sync();
        res.points = points;
        return res;
    }
    GCNHIP_CHECK(gcnhip_dbscan_cores(ctx, d_pack, n, t.dim, d_count, min_samples, d_state, state_bytes));
    for (bool settled = false; !settled;) {                    // every round but the last lowers a root: it ends
        for (int r = 0; r < DBSCAN_BATCH; r++) GCNHIP_CHECK(gcnhip_dbscan_link(ctx, d_pack, n, t.dim, eps[0], d_state, state_bytes, d_flags + r));
        int32_t flags[DBSCAN_BATCH];
        GCNHIP_CHECK(gcnhip_d2h(ctx, flags, d_flags, sizeof flags));
        m.sync();
        for (int r = 0; r < DBSCAN_BATCH && !settled; r++) {   // a round after the settled one changes nothing
            res.rounds++;
            settled = flags[r] == 0;
        }
    }
    GCNHIP_CHECK(gcnhip_dbscan_labels(ctx, d_pack, n, t.dim, d_state, state_bytes, d_labels, d_core, d_sizes, d_totals));
    int32_t totals[5] = {};
    GCNHIP_CHECK(gcnhip_d2h(ctx, totals, d_totals, sizeof totals));
    if (labels) GCNHIP_CHECK(gcnhip_d2h(ctx, labels, d_labels, nn * sizeof(int32_t)));
    if (core) GCNHIP_CHECK(gcnhip_d2h(ctx, core, d_core, nn));
    if (sizes) GCNHIP_CHECK(gcnhip_d2h(ctx, sizes, d_sizes, nn * sizeof(int32_t)));
    m.sync();
    res.points = totals[0]; res.core = totals[1]; res.border = totals[2]; res.noise = totals[3]; res.clusters = totals[4];
    if (contingency && !data && res.clusters >= 1 && res.clusters <= 256) {
        const int C = m.params.output_dim, k = (int)res.clusters;
        if (!d_label_all) d_label_all = arena.upload(m.data->label.data() + m.row_start(), (size_t)m.n_local);
        int32_t *d_cont = d_db_cont.need((size_t)k * C + 1);   // {counts [k x C] | skipped}
        GCNHIP_CHECK(gcnhip_contingency_rows(ctx, d_labels, d_label_all, m.n_local, d_rows, n, k, C, d_cont, d_cont + (size_t)k * C));
        std::vector<int32_t> cnt((size_t)k * C + 1);
        GCNHIP_CHECK(gcnhip_d2h(ctx, cnt.data(), d_cont, cnt.size() * sizeof(int32_t)));
        m.sync();
        for (size_t e = 0; e < (size_t)k * C; e++) contingency[e] = cnt[e];
        res.contingency_rows = k;
        res.skipped = cnt[(size_t)k * C];
    }
    return res;
}

ModelQueries::Dbscan ModelQueries::dbscan(double eps, int min_samples, int split, const int *nodes, int n, const float *data, int data_dim,
                                          bool normalize, int32_t *labels, uint8_t *core, int32_t *count, int32_t *sizes, int64_t *contingency) {
    if (min_samples < 1) throw GcnHipFailure(-1, "dbscan: min_samples must be at least 1, got " + std::to_string(min_samples));
    return dbscan_run("dbscan", &eps, 1, min_samples, split, nodes, n, data, data_dim, normalize, labels, core, count, sizes, contingency);
}

ModelQueries::Dbscan ModelQueries::neighbor_counts(const double *eps, int n_eps, int split, const int *nodes, int n, const float *data, int data_dim,
                                                   bool normalize, int32_t *count) {
    return dbscan_run("neighbor_counts", eps, n_eps, 0, split, nodes, n, data, data_dim, normalize, nullptr, nullptr, count, nullptr, nullptr);
}
