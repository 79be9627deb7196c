// hdbscan_query.cpp — ModelQueries::hdbscan: the density clusters of the hidden layer of a trained model (or of a caller's table)
// without a radius (queries.h has the contract, include/gcnhip_driver.h the definitions, csrc/hdbscan.hip the kernels, host/hdbscan.h
// what is derived from the tree).  Off the epoch path: the hidden layer comes from embed_forward and no training module is touched.
#include "queries.h"
#include "gcn.h"
#include "hdbscan.h"
#include "hip_check.h"
#include <algorithm>
#include <cstring>
#include <numeric>

int64_t ModelQueries::hdbscan_rows(int min_cluster_size, int min_samples, int split, const int *nodes, int n, const float *data, int data_dim,
                                   std::vector<int> *rows) {
    const double one = 1.0;
    const int64_t listed = dbscan_rows("hdbscan", split, nodes, n, data, data_dim, &one, 1, 1, rows);   // the rows and every refusal DBSCAN has for them
    const std::string w = "hdbscan: ";
    if (min_cluster_size < 2) throw GcnHipFailure(-1, w + "min_cluster_size must be at least 2, got " + std::to_string(min_cluster_size));
    if (min_samples < 1 || min_samples > 33)
        throw GcnHipFailure(-1, w + "min_samples must be in 1..33 (the core distance is a row of the exact k-nearest-neighbour walk), got " +
                                    std::to_string(min_samples));
    if (listed > HDBSCAN_MAX_ROWS) throw GcnHipFailure(-1, w + "at most 65536 rows (an edge's two ends share a 64-bit key with its weight), got " + std::to_string(listed));
    hdbscan_points(min_samples, listed, "rows");
    return listed;
}

void ModelQueries::hdbscan_points(int min_samples, int64_t have, const char *what) const {
    const int64_t need = 2 * (int64_t)(min_samples - 1) + 1;
    if (have < need)
        throw GcnHipFailure(-1, "hdbscan: at least 2 (min_samples - 1) + 1 = " + std::to_string(need) + " " + what + ", got " + std::to_string(have));
}

ModelQueries::Hdbscan ModelQueries::hdbscan(int min_cluster_size, int min_samples, int split, const int *nodes, int n, const float *data, int data_dim,
                                            bool normalize, bool leaf, bool allow_single_cluster, int32_t *labels, double *probabilities, float *core2,
                                            int32_t *mst_lo, int32_t *mst_hi, float *mst_d2, double *linkage, int32_t *sizes, int64_t *contingency) {
    Hdbscan res;
    std::vector<int> rows;
    res.rows = hdbscan_rows(min_cluster_size, min_samples, split, nodes, n, data, data_dim, &rows);      // every refusal that needs no GPU
    n = (int)res.rows;
    if (n < 1) throw GcnHipFailure(-1, "hdbscan: invalid argument (no rows)");
    m.sync();                                                  // run()'s epochs in flight, the validation lane's pass
    gcnhip_ctx *ctx = m.env.ctx;
    const size_t nn = (size_t)n, k = (size_t)(min_samples - 1);
    // {rows | labels [n] | edges [3 x n] | knn positions [n x k] | points | counts [2 x HDBSCAN_BATCH]}
    int32_t *d_int = d_hd_int.need(nn * (5 + k) + 1 + 2 * HDBSCAN_BATCH), *d_labels = d_int + nn, *d_edges = d_labels + nn, *d_pos = d_edges + 3 * nn,
            *d_points = d_pos + nn * k, *d_counts = d_points + 1;
    float *d_d2 = d_hd_f32.need(std::max(nn * k, (size_t)1));
    EmbedTable t;
    const int32_t *d_rows = nullptr;
    if (data) {
        float *d = d_hd_data.need(nn * (size_t)data_dim);
        GCNHIP_CHECK(gcnhip_h2d(ctx, d, data, nn * (size_t)data_dim * sizeof(float)));
        t = EmbedTable{d, data_dim, n, data_dim, nullptr};
    } else {
        t = embed_forward(normalize);
        GCNHIP_CHECK(gcnhip_h2d(ctx, d_int, rows.data(), nn * sizeof(int32_t)));
        d_rows = d_int;
    }
    size_t pack_bytes = 0, state_bytes = 0;
    if (gcnhip_hdbscan_plan(n, t.dim, &pack_bytes, &state_bytes) != 0) throw GcnHipFailure(-1, std::string("hdbscan: ") + gcnhip_last_error());
    unsigned char *d_pack = d_hd_pack.need(pack_bytes), *d_state = d_hd_state.need(state_bytes);

    GCNHIP_CHECK(gcnhip_tsne_pack(ctx, t.data, t.ld, t.rows, t.dim, t.inv_norm, d_rows, n, d_pack, pack_bytes, d_points));
    if (k) GCNHIP_CHECK(gcnhip_knn_rows(ctx, d_pack, n, t.dim, (int)k, d_pos, d_d2));
    int32_t points = 0;
    GCNHIP_CHECK(gcnhip_d2h(ctx, &points, d_points, sizeof(int32_t)));
    std::vector<float> knn_d2(nn * k);
    if (k) GCNHIP_CHECK(gcnhip_d2h(ctx, knn_d2.data(), d_d2, nn * k * sizeof(float)));
    m.sync();
    res.points = points;
    hdbscan_points(min_samples, points, "points");
    GCNHIP_CHECK(gcnhip_hdbscan_start(ctx, d_pack, n, t.dim, k ? d_d2 : nullptr, (int)k, d_state, state_bytes));
    for (int64_t comps = points; comps > 1;) {                 // the components at least halve per round: it ends
        for (int r = 0; r < HDBSCAN_BATCH; r++) {
            GCNHIP_CHECK(gcnhip_hdbscan_nearest(ctx, d_pack, n, t.dim, d_state, state_bytes));
            GCNHIP_CHECK(gcnhip_hdbscan_merge(ctx, d_pack, n, t.dim, d_state, state_bytes, d_edges, d_counts + 2 * r));
        }
        int32_t counts[2 * HDBSCAN_BATCH];
        GCNHIP_CHECK(gcnhip_d2h(ctx, counts, d_counts, sizeof counts));
        m.sync();
        for (int r = 0; r < HDBSCAN_BATCH && comps > 1; r++) { // a round at one component changes nothing
            if (counts[2 * r] >= comps) throw GcnHipFailure(-1, "hdbscan: a round merged nothing");
            res.rounds++;
            comps = counts[2 * r];
            res.edges = counts[2 * r + 1];
        }
    }
    const size_t ne = (size_t)res.edges;
    std::vector<int32_t> raw(3 * nn), lo(ne), hi(ne);
    if (ne) GCNHIP_CHECK(gcnhip_d2h(ctx, raw.data(), d_edges, 3 * nn * sizeof(int32_t)));
    m.sync();
    std::vector<size_t> order(ne);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {      // (w, lo, hi): the same bits on every run
        const uint32_t wa = (uint32_t)raw[2 * nn + a], wb = (uint32_t)raw[2 * nn + b];
        return wa != wb ? wa < wb : raw[a] != raw[b] ? raw[a] < raw[b] : raw[nn + a] < raw[nn + b];
    });
    std::vector<float> w(ne);
    for (size_t e = 0; e < ne; e++) {
        lo[e] = raw[order[e]];
        hi[e] = raw[nn + order[e]];
        const uint32_t bits = (uint32_t)raw[2 * nn + order[e]];
        std::memcpy(&w[e], &bits, sizeof bits);
    }
    if (mst_lo) std::copy(lo.begin(), lo.end(), mst_lo);
    if (mst_hi) std::copy(hi.begin(), hi.end(), mst_hi);
    if (mst_d2) std::copy(w.begin(), w.end(), mst_d2);
    if (core2)
        for (size_t i = 0; i < nn; i++) core2[i] = k ? knn_d2[i * k + (k - 1)] : 0.f;
    std::vector<int32_t> lab(nn);
    std::vector<double> prob(nn), w64(w.begin(), w.end());
    int64_t info[3] = {};
    std::string err;
    if (gcn_hdbscan_tree(lo.data(), hi.data(), w64.data(), (int64_t)ne, n, min_cluster_size, leaf, allow_single_cluster, lab.data(), prob.data(), linkage,
                         info, &err) != 0)
        throw GcnHipFailure(-1, err);
    res.clusters = info[1];
    res.noise = res.points - (int64_t)std::count_if(lab.begin(), lab.end(), [](int32_t l) { return l >= 0; });
    if (labels) std::copy(lab.begin(), lab.end(), labels);
    if (probabilities) std::copy(prob.begin(), prob.end(), probabilities);
    if (sizes) {
        std::fill(sizes, sizes + nn, 0);
        for (const int32_t l : lab)
            if (l >= 0) sizes[l]++;
    }
    if (contingency && !data && res.clusters >= 1 && res.clusters <= 256) {
        const int C = m.params.output_dim, kc = (int)res.clusters;
        if (!d_label_all) d_label_all = arena.upload(m.data->label.data() + m.row_start(), (size_t)m.n_local);
        int32_t *d_cont = d_hd_cont.need((size_t)kc * C + 1);  // {counts [k x C] | skipped}
        GCNHIP_CHECK(gcnhip_h2d(ctx, d_labels, lab.data(), nn * sizeof(int32_t)));
        GCNHIP_CHECK(gcnhip_contingency_rows(ctx, d_labels, d_label_all, m.n_local, d_rows, n, kc, C, d_cont, d_cont + (size_t)kc * C));
        std::vector<int32_t> cnt((size_t)kc * C + 1);
        GCNHIP_CHECK(gcnhip_d2h(ctx, cnt.data(), d_cont, cnt.size() * sizeof(int32_t)));
        m.sync();
        for (size_t e = 0; e < (size_t)kc * C; e++) contingency[e] = cnt[e];
        res.contingency_rows = kc;
        res.skipped = cnt[(size_t)kc * C];
    }
    return res;
}
