// kmeans.cpp — ModelQueries::kmeans: Lloyd's k-means on the hidden layer of a trained model, where it lies (queries.h has the
// contract, csrc/kmeans.hip the definitions and the kernels).  Off the epoch path: the hidden layer comes from embed_forward, the
// loop is composed here from the library's entry points, and no training module is touched.
#include "queries.h"
#include "gcn.h"
#include "hip_check.h"
#include <algorithm>
#include <cmath>

// the rows a query lists: a split in ascending dataset id, or the node query (NULL: every node in id order)
std::vector<int> ModelQueries::kmeans_list(const char *what, int split, const int *nodes, int &n) {
    if (!split) return embed_query(what, nodes, n);
    std::vector<std::pair<int, int>> by_id;
    const int r0 = m.row_start();
    for (int r = 0; r < m.n_local; r++)
        if (m.data->split[r0 + r] == split) by_id.emplace_back(m.node_id(r), r);
    std::sort(by_id.begin(), by_id.end());
    std::vector<int> rows(by_id.size());
    for (size_t i = 0; i < by_id.size(); i++) rows[i] = by_id[i].second;
    n = (int)rows.size();
    return rows;
}

int64_t ModelQueries::kmeans_rows(int k, int split, const int *nodes, int n, int iters, int init, const int *init_pos, const float *init_centers) {
    const char *what = "kmeans";
    const std::string w = std::string(what) + ": ";
    require(what, ONE_RANK);
    if (m.flags & HIPGCN_BF16_TABLES) throw GcnHipFailure(-1, w + "not with bf16 tables (the kernels read the f32 rows of the hidden layer)");
    if (m.params.hidden_dim < 1 || m.params.hidden_dim > 256)
        throw GcnHipFailure(-1, w + "a hidden width of at most 256 (the assignment keeps a tile of rows and one of centres in LDS)");
    if (split < 0 || split > 3) throw GcnHipFailure(-1, w + "invalid argument (split is 0 with a node query, or 1 train, 2 validation, 3 test)");
    if (n < 0) throw GcnHipFailure(-1, w + "invalid argument");
    if (k < 1 || k > 256) throw GcnHipFailure(-1, w + "k must be in 1..256, got " + std::to_string(k));
    if (iters < 1) throw GcnHipFailure(-1, w + "iters must be at least 1, got " + std::to_string(iters));
    if (init != KMEANS_INIT_PLUSPLUS && init != KMEANS_INIT_POSITIONS && init != KMEANS_INIT_CENTERS)
        throw GcnHipFailure(-1, w + "init is 0 (k-means++), 1 (k list positions) or 2 (k centres)");
    if ((init == KMEANS_INIT_POSITIONS && !init_pos) || (init == KMEANS_INIT_CENTERS && !init_centers))
        throw GcnHipFailure(-1, w + "invalid argument (the initial positions or centres are missing)");
    int listed = n;
    kmeans_list(what, split, nodes, listed);                   // a node id outside the graph is refused here
    if (k > listed) throw GcnHipFailure(-1, w + "k = " + std::to_string(k) + " is above the " + std::to_string(listed) + " rows listed");
    if (init == KMEANS_INIT_POSITIONS)
        for (int c = 0; c < k; c++)
            if (init_pos[c] < 0 || init_pos[c] >= listed)
                throw GcnHipFailure(-1, w + "initial position " + std::to_string(init_pos[c]) + " is outside the list (0.." + std::to_string(listed - 1) + ")");
    if (init == KMEANS_INIT_CENTERS)
        for (size_t e = 0; e < (size_t)k * m.params.hidden_dim; e++)
            if (!std::isfinite(init_centers[e])) throw GcnHipFailure(-1, w + "an initial centre is not finite");
    return listed;
}

ModelQueries::KMeans ModelQueries::kmeans(int k, int split, const int *nodes, int n, int iters, bool normalize, int init, const int *init_pos,
                                          const float *init_centers, const uint64_t *seed, size_t scratch_bytes, int32_t *assign, float *dist2,
                                          float *centers, int32_t *sizes, int32_t *seed_pos, double *history, int64_t *contingency) {
    const char *what = "kmeans";
    KMeans res;
    res.rows = kmeans_rows(k, split, nodes, n, iters, init, init_pos, init_centers);       // every refusal, before any launch
    res.k = k;
    res.seed = seed ? *seed : m.env.seed;
    const int C = m.params.output_dim;
    if (contingency && (m.opt_.multilabel || C > 64))
        throw GcnHipFailure(-1, std::string(what) + ": the cluster x class table needs a single-label model with at most 64 classes");
    const std::vector<int> rows = kmeans_list(what, split, nodes, n);
    m.sync();                                                  // run()'s epochs in flight, the validation lane's pass
    const EmbedTable t = embed_forward(normalize);
    gcnhip_ctx *ctx = m.env.ctx;
    const size_t nn = (size_t)n;
    size_t full = 0, least = 0, seeding = 0;
    if (gcnhip_kmeans_plan(n, k, t.dim, &full, &least, &seeding) != 0) throw GcnHipFailure(-1, std::string("kmeans: ") + gcnhip_last_error());
    const size_t upd_bytes = scratch_bytes ? std::max(std::min(full, scratch_bytes), least) : full;
    unsigned char *d_scr = d_km_scratch.need(std::max(upd_bytes, seeding));
    int32_t *d_rows = d_km_rows.need(nn);
    int32_t *d_assign = d_km_assign.need(2 * nn);
    float *d_dist = d_km_dist.need(nn);
    float *d_centers = d_km_centers.need((size_t)k * t.dim), *d_cn = d_km_cn.need((size_t)k);
    int32_t *d_sizes = d_km_sizes.need((size_t)k), *d_pos = d_km_pos.need((size_t)k), *d_flag = d_km_flag.need(2);
    double *d_inertia = d_km_inertia.need((size_t)iters);
    GCNHIP_CHECK(gcnhip_h2d(ctx, d_rows, rows.data(), nn * sizeof(int32_t)));

    if (init == KMEANS_INIT_PLUSPLUS) {
        GCNHIP_CHECK(gcnhip_kmeans_seed(ctx, t.data, t.ld, t.rows, t.dim, t.inv_norm, d_rows, n, k, res.seed ^ KEY_KMEANS, d_centers, t.dim, d_pos, d_scr, seeding));
        if (seed_pos) GCNHIP_CHECK(gcnhip_d2h(ctx, seed_pos, d_pos, (size_t)k * sizeof(int32_t)));
    } else if (init == KMEANS_INIT_POSITIONS) {
        std::vector<int32_t> at((size_t)k);
        for (int c = 0; c < k; c++) at[c] = rows[init_pos[c]];
        GCNHIP_CHECK(gcnhip_h2d(ctx, d_pos, at.data(), at.size() * sizeof(int32_t)));
        GCNHIP_CHECK(gcnhip_embed_rows(ctx, t.data, t.ld, t.rows, t.dim, t.inv_norm, d_pos, k, d_centers, t.dim));
    } else {
        GCNHIP_CHECK(gcnhip_h2d(ctx, d_centers, init_centers, (size_t)k * t.dim * sizeof(float)));
    }
    // the norms of the initial centres: an update over no rows keeps every row and writes cn
    GCNHIP_CHECK(gcnhip_kmeans_update(ctx, t.data, t.ld, t.rows, t.dim, t.inv_norm, d_rows, 0, nullptr, nullptr, k, d_centers, t.dim, d_sizes, d_cn, nullptr,
                                      d_scr, upd_bytes));
    std::vector<int32_t> moved_at;
    int32_t *cur = d_assign, *prev = nullptr;
    for (int it = 0; it < iters; it++) {
        GCNHIP_CHECK(gcnhip_kmeans_assign(ctx, t.data, t.ld, t.rows, t.dim, t.inv_norm, d_rows, n, d_centers, t.dim, d_cn, k, prev, cur, d_dist, d_flag));
        GCNHIP_CHECK(gcnhip_kmeans_update(ctx, t.data, t.ld, t.rows, t.dim, t.inv_norm, d_rows, n, cur, d_dist, k, d_centers, t.dim, d_sizes, d_cn,
                                          d_inertia + it, d_scr, upd_bytes));
        int32_t moved = 0;
        GCNHIP_CHECK(gcnhip_d2h(ctx, &moved, d_flag, sizeof(int32_t)));       // the four bytes of an iteration
        moved_at.push_back(moved);
        res.iters_run = it + 1;
        prev = cur;
        cur = cur == d_assign ? d_assign + nn : d_assign;
        if (moved == 0) { res.converged = true; break; }
    }
    std::vector<double> inertia((size_t)res.iters_run);
    GCNHIP_CHECK(gcnhip_d2h(ctx, inertia.data(), d_inertia, inertia.size() * sizeof(double)));
    res.inertia = inertia.back();
    if (history)
        for (int it = 0; it < res.iters_run; it++) { history[2 * it] = (double)moved_at[it]; history[2 * it + 1] = inertia[it]; }
    if (assign) GCNHIP_CHECK(gcnhip_d2h(ctx, assign, prev, nn * sizeof(int32_t)));
    if (dist2) GCNHIP_CHECK(gcnhip_d2h(ctx, dist2, d_dist, nn * sizeof(float)));
    if (centers) GCNHIP_CHECK(gcnhip_d2h(ctx, centers, d_centers, (size_t)k * t.dim * sizeof(float)));
    if (sizes) GCNHIP_CHECK(gcnhip_d2h(ctx, sizes, d_sizes, (size_t)k * sizeof(int32_t)));
    if (contingency) {
        if (!d_label_all) d_label_all = arena.upload(m.data->label.data() + m.row_start(), (size_t)m.n_local);
        int32_t *d_counts = d_km_counts.need((size_t)k * C);
        GCNHIP_CHECK(gcnhip_contingency_rows(ctx, prev, d_label_all, m.n_local, d_rows, n, k, C, d_counts, d_flag + 1));
        std::vector<int32_t> cnt((size_t)k * C);
        int32_t skipped = 0;
        GCNHIP_CHECK(gcnhip_d2h(ctx, cnt.data(), d_counts, cnt.size() * sizeof(int32_t)));
        GCNHIP_CHECK(gcnhip_d2h(ctx, &skipped, d_flag + 1, sizeof(int32_t)));
        for (size_t e = 0; e < cnt.size(); e++) contingency[e] = cnt[e];
        res.skipped = skipped;
    }
    m.sync();
    return res;
}
