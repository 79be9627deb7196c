// overlap_query.cpp — ModelQueries::clustering / link_overlap: triangles and clustering coefficients of the model's nodes, and the
// common-neighbour scores of node pairs, counted where the adjacency lies (queries.h has the contract, csrc/overlap.hip the
// definitions and the kernels, host/overlap.h the measures).  Off the epoch path: no training module is touched, no forward runs.
#include "queries.h"
#include "gcn.h"
#include "hip_check.h"
#include "overlap.h"
#include <algorithm>

void ModelQueries::overlap_sets() {
    int n_rows = 0, nnz = 0;
    GCNHIP_CHECK(gcnhip_graph_arrays(m.graph, nullptr, nullptr, nullptr, &n_rows, &nnz));
    int64_t bytes = 0;
    GCNHIP_CHECK(gcnhip_overlap_plan(m.graph, &bytes));
    int32_t *idx = d_ov_idx.need((size_t)nnz), *len = d_ov_len.need((size_t)n_rows), *sort = d_ov_sort.need((size_t)bytes / 4);
    GCNHIP_CHECK(gcnhip_overlap_sets(m.env.ctx, m.graph, idx, len, sort, bytes));
}

ModelQueries::Overlap ModelQueries::clustering(int split, const int *nodes, int n, int64_t *t2, int32_t *deg, int64_t *totals) {
    const char *what = "clustering";
    require(what, ONE_RANK);
    if (split < 0 || split > 3 || n < 0)
        throw GcnHipFailure(-1, std::string(what) + ": invalid argument (split is 0 with a node query, or 1 train, 2 validation, 3 test)");
    const std::vector<int> rows = kmeans_list(what, split, nodes, n);     // a node id outside the graph is refused here
    Overlap res;
    res.rows = n;
    m.sync();                                                  // run()'s epochs in flight, the validation lane's pass
    gcnhip_ctx *ctx = m.env.ctx;
    overlap_sets();
    const size_t nn = (size_t)n;
    int32_t *d_int = d_ov_int.need(2 * nn);                    // {rows | deg}
    int64_t *d_long = d_ov_long.need(nn + 9);                  // {t2 | totals [8] | skipped}
    if (n > 0) GCNHIP_CHECK(gcnhip_h2d(ctx, d_int, rows.data(), nn * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_overlap_rows(ctx, m.graph, d_ov_idx.p, d_ov_len.p, d_int, n, d_long, d_int + nn, d_long + nn, d_long + nn + 8));
    int64_t h[9];
    GCNHIP_CHECK(gcnhip_d2h(ctx, h, d_long + nn, sizeof h));
    if (totals) std::copy(h, h + 8, totals);
    res.skipped = h[8];
    if (t2 && n > 0) GCNHIP_CHECK(gcnhip_d2h(ctx, t2, d_long, nn * sizeof(int64_t)));
    if (deg && n > 0) GCNHIP_CHECK(gcnhip_d2h(ctx, deg, d_int + nn, nn * sizeof(int32_t)));
    m.sync();
    return res;
}

ModelQueries::Overlap ModelQueries::link_overlap(const int *src, const int *dst, int n, int weight_mask, int32_t *cn, int32_t *un, int64_t *pa, int64_t *aa,
                                                 int64_t *ra) {
    const char *what = "link_overlap";
    require(what, ONE_RANK);
    if (n < 0 || (n > 0 && (!src || !dst))) throw GcnHipFailure(-1, std::string(what) + ": invalid argument");
    if (weight_mask & ~(OVERLAP_ADAMIC_ADAR | OVERLAP_RESOURCE_ALLOCATION))
        throw GcnHipFailure(-1, std::string(what) + ": the weights are 1 (adamic_adar) and 2 (resource_allocation), got mask " + std::to_string(weight_mask));
    std::vector<int> a, b;
    if (n > 0) { query_rows(what, src, n, a); query_rows(what, dst, n, b); }
    Overlap res;
    res.rows = n;
    m.sync();
    gcnhip_ctx *ctx = m.env.ctx;
    overlap_sets();
    const size_t nn = (size_t)n, nl = (size_t)m.n_local;
    std::vector<int32_t> len(std::max<size_t>(nl, 1));
    if (nl > 0) GCNHIP_CHECK(gcnhip_d2h(ctx, len.data(), d_ov_len.p, nl * sizeof(int32_t)));   // one int32 per node, once per call
    int32_t *d_int = d_ov_int.need(4 * nn);                    // {src | dst | cn | un}
    int64_t *d_long = d_ov_long.need(nn + nl + 1);             // {wsum | wt | skipped}
    if (n > 0) {
        GCNHIP_CHECK(gcnhip_h2d(ctx, d_int, a.data(), nn * sizeof(int32_t)));
        GCNHIP_CHECK(gcnhip_h2d(ctx, d_int + nn, b.data(), nn * sizeof(int32_t)));
    }
    int64_t *d_wt = d_long + nn, *d_skipped = d_long + nn + nl;
    std::vector<int64_t> wt(std::max<size_t>(nl, 1));
    const int kinds[2] = {OVERLAP_ADAMIC_ADAR, OVERLAP_RESOURCE_ALLOCATION};
    int64_t *const outs[2] = {aa, ra};
    bool counted = false;
    for (int k = 0; k < 2; k++) {
        if (!(weight_mask & kinds[k])) continue;
        for (size_t r = 0; r < nl; r++) wt[r] = gcn_overlap_weight(kinds[k], len[r]);
        if (nl > 0) GCNHIP_CHECK(gcnhip_h2d(ctx, d_wt, wt.data(), nl * sizeof(int64_t)));
        GCNHIP_CHECK(gcnhip_overlap_pairs(ctx, m.graph, d_ov_idx.p, d_ov_len.p, d_int, d_int + nn, n, d_wt, d_int + 2 * nn, d_int + 3 * nn, d_long, d_skipped));
        if (outs[k] && n > 0) GCNHIP_CHECK(gcnhip_d2h(ctx, outs[k], d_long, nn * sizeof(int64_t)));
        counted = true;
    }
    if (!counted)
        GCNHIP_CHECK(gcnhip_overlap_pairs(ctx, m.graph, d_ov_idx.p, d_ov_len.p, d_int, d_int + nn, n, nullptr, d_int + 2 * nn, d_int + 3 * nn, nullptr, d_skipped));
    GCNHIP_CHECK(gcnhip_d2h(ctx, &res.skipped, d_skipped, sizeof(int64_t)));
    if (cn && n > 0) GCNHIP_CHECK(gcnhip_d2h(ctx, cn, d_int + 2 * nn, nn * sizeof(int32_t)));
    if (un && n > 0) GCNHIP_CHECK(gcnhip_d2h(ctx, un, d_int + 3 * nn, nn * sizeof(int32_t)));
    for (size_t i = 0; pa && i < nn; i++) pa[i] = (int64_t)len[a[i]] * (int64_t)len[b[i]];
    m.sync();
    return res;
}
