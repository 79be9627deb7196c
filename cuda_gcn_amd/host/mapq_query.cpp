// mapq_query.cpp — ModelQueries::knn / map_quality: the exact nearest neighbours of the hidden layer of a trained model (or of a
// caller's table), and whether a map of it keeps them (queries.h has the contract, include/gcnhip_driver.h the definitions,
// csrc/mapq.hip the kernels).  Off the epoch path: the hidden layer comes from embed_forward and no training module is touched.
#include "queries.h"
#include "gcn.h"
#include "hip_check.h"

int gcn_map_quality_metrics(const int64_t *sums, int64_t points, int k, double *out, std::string *err) {
    const auto fail = [&](const std::string &why) {
        if (err) *err = "map_quality_metrics: " + why;
        return -1;
    };
    if (!sums || !out) return fail("invalid argument");
    if (k < 1 || k > 32) return fail("k must be in 1..32, got " + std::to_string(k));
    if (points < 2 * (int64_t)k + 1) return fail("k must be below half the points: " + std::to_string(points) + " points at k = " + std::to_string(k));
    const double m = (double)points, kk = (double)k, worst = m * kk * (2.0 * m - 3.0 * kk - 1.0) / 2.0;   // > 0: 2 m - 3 k - 1 >= k + 1
    if (sums[0] < 0 || sums[1] < 0 || sums[2] < 0 || (double)sums[0] > worst || (double)sums[1] > worst || sums[2] > points * k)
        return fail("sums outside their range");
    out[0] = 1.0 - (double)sums[0] / worst;
    out[1] = 1.0 - (double)sums[1] / worst;
    out[2] = (double)sums[2] / (m * kk);
    return 0;
}

int64_t ModelQueries::mapq_rows(const char *what, int k, int split, const int *nodes, int n, const float *data, int data_dim, std::vector<int> *rows) {
    const double one = 1.0;
    const int64_t listed = dbscan_rows(what, split, nodes, n, data, data_dim, &one, 1, 1, rows);   // the rows and every refusal DBSCAN has for them
    const std::string w = std::string(what) + ": ";
    if (k < 1 || k > 32) throw GcnHipFailure(-1, w + "k must be in 1..32, got " + std::to_string(k));
    if (listed < 2 * (int64_t)k + 1)
        throw GcnHipFailure(-1, w + "at least 2 k + 1 = " + std::to_string(2 * k + 1) + " rows (k below half the points), got " + std::to_string(listed));
    return listed;
}

void ModelQueries::mapq_points(const char *what, int k, int64_t points) const {
    if (points < 2 * (int64_t)k + 1)
        throw GcnHipFailure(-1, std::string(what) + ": at least 2 k + 1 = " + std::to_string(2 * k + 1) + " points (k below half of them), got " +
                                    std::to_string(points));
}

// the pack of the listed rows of the hidden layer, or of the caller's n x data_dim table; returns the width packed
int ModelQueries::mapq_pack(const std::vector<int> &rows, int n, int k, const float *data, int data_dim, bool normalize, Scratch<unsigned char> &pack,
                            int32_t *d_rows, int32_t *d_points) {
    gcnhip_ctx *ctx = m.env.ctx;
    EmbedTable t;
    const int32_t *list = nullptr;
    if (data) {
        float *d = d_mq_data.need((size_t)n * (size_t)data_dim);
        GCNHIP_CHECK(gcnhip_h2d(ctx, d, data, (size_t)n * (size_t)data_dim * sizeof(float)));
        t = EmbedTable{d, data_dim, n, data_dim, nullptr};
    } else {
        t = embed_forward(normalize);
        GCNHIP_CHECK(gcnhip_h2d(ctx, d_rows, rows.data(), (size_t)n * sizeof(int32_t)));
        list = d_rows;
    }
    size_t pack_bytes = 0;
    if (gcnhip_mapq_plan(n, t.dim, k, &pack_bytes, nullptr) != 0) throw GcnHipFailure(-1, std::string("map quality: ") + gcnhip_last_error());
    GCNHIP_CHECK(gcnhip_tsne_pack(ctx, t.data, t.ld, t.rows, t.dim, t.inv_norm, list, n, pack.need(pack_bytes), pack_bytes, d_points));
    return t.dim;
}

ModelQueries::Knn ModelQueries::knn(int k, int split, const int *nodes, int n, const float *data, int data_dim, bool normalize, int32_t *ids,
                                    int32_t *pos, float *d2) {
    Knn res;
    std::vector<int> rows;
    res.rows = mapq_rows("knn", k, split, nodes, n, data, data_dim, &rows);                 // every refusal that needs no GPU
    n = (int)res.rows;
    m.sync();                                                  // run()'s epochs in flight, the validation lane's pass
    gcnhip_ctx *ctx = m.env.ctx;
    const size_t nk = (size_t)n * (size_t)k;
    // {rows [n] | points | pos [n x k]}
    int32_t *d_int = d_mq_int.need((size_t)n + 1 + nk), *d_points = d_int + n, *d_pos = d_points + 1;
    float *d_d2 = d_mq_d2.need(nk);
    const int dim = mapq_pack(rows, n, k, data, data_dim, normalize, d_mq_pack[0], d_int, d_points);
    GCNHIP_CHECK(gcnhip_knn_rows(ctx, d_mq_pack[0].p, n, dim, k, d_pos, d_d2));
    int32_t points = 0;
    GCNHIP_CHECK(gcnhip_d2h(ctx, &points, d_points, sizeof(int32_t)));
    std::vector<int32_t> host_pos(ids && !pos ? nk : 0);
    if (ids && !pos) pos = host_pos.data();
    if (pos) GCNHIP_CHECK(gcnhip_d2h(ctx, pos, d_pos, nk * sizeof(int32_t)));
    if (d2) GCNHIP_CHECK(gcnhip_d2h(ctx, d2, d_d2, nk * sizeof(float)));
    m.sync();
    res.points = points;
    mapq_points("knn", k, points);
    if (ids)                                                   // a position's node: the list is the one the pack was made of
        for (size_t e = 0; e < nk; e++) ids[e] = pos[e] < 0 ? -1 : data ? pos[e] : m.node_id(rows[(size_t)pos[e]]);
    return res;
}

ModelQueries::MapQuality ModelQueries::map_quality(const float *coords, int64_t coords_rows, int coords_dim, int k, int split, const int *nodes, int n,
                                                   const float *data, int data_dim, bool normalize, int32_t *per_node) {
    MapQuality res;
    std::vector<int> rows;
    res.rows = mapq_rows("map_quality", k, split, nodes, n, data, data_dim, &rows);
    res.k = k;
    if (!coords || coords_dim < 1 || coords_dim > 256)
        throw GcnHipFailure(-1, "map_quality: coords of a width in 1..256, got " + std::to_string(coords_dim));
    if (coords_rows != res.rows)
        throw GcnHipFailure(-1, "map_quality: the query lists " + std::to_string(res.rows) + " rows, coords has " + std::to_string(coords_rows));
    n = (int)res.rows;
    m.sync();
    gcnhip_ctx *ctx = m.env.ctx;
    const size_t nk = (size_t)n * (size_t)k;
    // {rows [n] | points of the input space, of the map | knn_x | knn_y | rank_x | rank_y [n x k] | per node [n x 3]}
    int32_t *d_int = d_mq_int.need((size_t)n + 2 + 4 * nk + 3 * (size_t)n), *d_points = d_int + n, *d_kx = d_points + 2, *d_ky = d_kx + nk,
            *d_rx = d_ky + nk, *d_ry = d_rx + nk, *d_per = d_ry + nk;
    float *d_d2 = d_mq_d2.need(nk);
    int64_t *d_tot = d_mq_totals.need(4);
    const int dim_x = mapq_pack(rows, n, k, data, data_dim, normalize, d_mq_pack[0], d_int, d_points);
    float *d_y = d_mq_coords.need((size_t)n * (size_t)coords_dim);                          // the map: a table by list position
    GCNHIP_CHECK(gcnhip_h2d(ctx, d_y, coords, (size_t)n * (size_t)coords_dim * sizeof(float)));
    size_t pack_bytes = 0;
    if (gcnhip_mapq_plan(n, coords_dim, k, &pack_bytes, nullptr) != 0) throw GcnHipFailure(-1, std::string("map_quality: ") + gcnhip_last_error());
    unsigned char *px = d_mq_pack[0].p, *py = d_mq_pack[1].need(pack_bytes);
    GCNHIP_CHECK(gcnhip_tsne_pack(ctx, d_y, coords_dim, n, coords_dim, nullptr, nullptr, n, py, pack_bytes, d_points + 1));
    GCNHIP_CHECK(gcnhip_knn_rows(ctx, px, n, dim_x, k, d_kx, d_d2));
    GCNHIP_CHECK(gcnhip_knn_rows(ctx, py, n, coords_dim, k, d_ky, d_d2));
    GCNHIP_CHECK(gcnhip_nbr_ranks(ctx, px, n, dim_x, k, d_ky, d_rx));                       // where the map's neighbours stand in the input space
    GCNHIP_CHECK(gcnhip_nbr_ranks(ctx, py, n, coords_dim, k, d_kx, d_ry));                  // and the input space's neighbours on the map
    GCNHIP_CHECK(gcnhip_mapq_sums(ctx, px, dim_x, py, coords_dim, n, k, d_kx, d_ky, d_rx, d_ry, d_per, d_tot));
    int64_t tot[4] = {};
    int32_t points[2] = {};
    GCNHIP_CHECK(gcnhip_d2h(ctx, tot, d_tot, sizeof tot));
    GCNHIP_CHECK(gcnhip_d2h(ctx, points, d_points, sizeof points));
    if (per_node) GCNHIP_CHECK(gcnhip_d2h(ctx, per_node, d_per, 3 * (size_t)n * sizeof(int32_t)));
    m.sync();
    // every position of the map is a point of it, so the two walks rank the same candidates only when every listed row is one too
    // (kmeans_list refuses a node outside the graph, and a caller's table lists its own rows)
    if (points[0] != n || points[1] != n || tot[3] != n)
        throw GcnHipFailure(-1, "map_quality: " + std::to_string(points[0]) + " of the " + std::to_string(n) + " listed rows are points of the input space");
    res.points = tot[3];
    mapq_points("map_quality", k, res.points);
    for (int q = 0; q < 3; q++) res.sums[q] = tot[q];
    std::string err;
    double s[3];
    if (gcn_map_quality_metrics(res.sums, res.points, k, s, &err) != 0) throw GcnHipFailure(-1, err);
    res.trustworthiness = s[0]; res.continuity = s[1]; res.knn_overlap = s[2];
    return res;
}
