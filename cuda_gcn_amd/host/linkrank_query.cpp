// linkrank_query.cpp — ModelQueries::link_ranks: the filtered rank of held-out edges among every node of the model, under the scores
// of the hidden layer (queries.h has the contract, include/gcnhip_driver.h the definitions, csrc/linkrank.hip the kernels,
// host/linkrank.h the metrics).  Off the epoch path: one evaluation forward as similar() makes it, no training module is touched.
#include "queries.h"
#include "gcn.h"
#include "hip_check.h"
#include <algorithm>

ModelQueries::LinkRanks ModelQueries::link_ranks(const int *src, const int *dst, int n, int metric, bool filtered, bool exclude_self, int32_t *above,
                                                 int32_t *equal) {
    const char *what = "link_ranks";
    embed_check(what, metric);
    if (n < 0 || (n > 0 && (!src || !dst || !above || !equal))) throw GcnHipFailure(-1, std::string(what) + ": invalid argument");
    // dataset ids -> local rows; an id that is no node stays a query and is answered -1 / -1
    const int N = m.params.num_nodes;
    std::vector<int> ids, rows;
    std::vector<int32_t> q(2 * (size_t)n, -1);                 // src, then dst
    for (int i = 0; i < n; i++)
        for (const int id : {src[i], dst[i]})
            if (id >= 0 && id < N) ids.push_back(id);
    query_rows(what, ids.data(), (int)ids.size(), rows);
    size_t at = 0;
    for (int i = 0; i < n; i++) {
        if (src[i] >= 0 && src[i] < N) q[i] = rows[at++];
        if (dst[i] >= 0 && dst[i] < N) q[(size_t)n + i] = rows[at++];
    }
    LinkRanks res;
    res.queries = n;
    m.sync();                                                  // run()'s epochs in flight, the validation lane's pass
    gcnhip_ctx *ctx = m.env.ctx;
    const EmbedTable t = embed_forward(metric == METRIC_COSINE);
    if (n == 0 || t.rows < 1) {
        std::fill(above, above + n, -1);
        std::fill(equal, equal + n, -1);
        m.sync();
        return res;
    }
    const int *x_ptr = nullptr;
    if (filtered) {                                            // the canonical sets of the adjacency, where the overlap pass leaves them
        overlap_sets();
        GCNHIP_CHECK(gcnhip_graph_arrays(m.graph, &x_ptr, nullptr, nullptr, nullptr, nullptr));
    }
    size_t bytes = 0;
    if (gcnhip_link_rank_plan(t.rows, n, 0, &res.chunk_rows, &res.n_chunks, &bytes) != 0) throw GcnHipFailure(-1, std::string(what) + ": " + gcnhip_last_error());
    const size_t nn = (size_t)n;
    int32_t *d_q = d_lr_int.need(4 * nn), *d_above = d_q + 2 * nn, *d_equal = d_above + nn;   // {src | dst | above | equal}
    GCNHIP_CHECK(gcnhip_h2d(ctx, d_q, q.data(), 2 * nn * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_link_ranks(ctx, t.data, t.ld, t.rows, t.dim, t.inv_norm, d_q, d_q + nn, n, x_ptr, filtered ? d_ov_len.p : nullptr,
                                   filtered ? d_ov_idx.p : nullptr, exclude_self ? 1 : 0, 0, d_lr_thr.need(bytes / sizeof(float)), bytes, 3, d_above, d_equal));
    GCNHIP_CHECK(gcnhip_d2h(ctx, above, d_above, nn * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_d2h(ctx, equal, d_equal, nn * sizeof(int32_t)));
    m.sync();
    res.invalid = std::count_if(above, above + n, [](int32_t a) { return a < 0; });
    return res;
}
