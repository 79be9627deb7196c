// louvain_query.cpp — ModelQueries::communities: the modularity communities of the model's adjacency (queries.h has the contract,
// csrc/louvain.hip the definitions and the kernels, host/louvain.h the modularity).  The sets are rebuilt as clustering() does;
// the levels are looped here, two coarse levels in turn, and the labels are composed where they lie.  Only the per-level scalars
// cross to the host.  Off the epoch path: no training module is touched, no forward runs.
#include "queries.h"
#include "gcn.h"
#include "hip_check.h"
#include <algorithm>

LouvainRun ModelQueries::communities(int max_levels, int max_sweeps, int32_t *labels, int32_t *level_labels, int level_capacity,
                                      int64_t *contingency) {
    const char *what = "communities";
    require(what, ONE_RANK);
    if (max_levels < 1 || max_sweeps < 0) throw GcnHipFailure(-1, std::string(what) + ": max_levels is at least 1 and max_sweeps at least 0");
    if (!m.node_order().empty())
        throw GcnHipFailure(-1, std::string(what) + ": the model renumbered its nodes (" + m.node_order_name() + "); the labels are defined on the dataset's ids");
    m.sync();
    gcnhip_ctx *ctx = m.env.ctx;
    overlap_sets();
    const int *g_ptr = nullptr;
    int n0 = 0, nnz = 0;
    GCNHIP_CHECK(gcnhip_graph_arrays(m.graph, &g_ptr, nullptr, nullptr, &n0, &nnz));
    int64_t bytes = 0;
    GCNHIP_CHECK(gcnhip_louvain_plan(n0, nnz, &bytes));
    const size_t nn = (size_t)n0 + 1, ne = (size_t)std::max(nnz, 1);
    void *scratch = d_lv_scratch.need((size_t)bytes / 8 + 2);
    int32_t *d_int = d_lv_int.need(4 * nn + 2 * (2 * nn + 2 * ne));   // {labels | comm | label | - } and two levels of {ptr | len | idx | w}
    int64_t *d_long = d_lv_long.need(3 * nn);                          // {tot | self_w of the two levels}
    int32_t *d_labels = d_int, *d_comm = d_int + nn, *d_label = d_int + 2 * nn;
    struct Level {
        const int32_t *ptr, *len, *idx;
        const uint32_t *w;
        const int64_t *self_w;
        int n;
        int64_t entries;
    } cur = {g_ptr, d_ov_len.p, d_ov_idx.p, nullptr, nullptr, n0, nnz};
    LouvainRun run;
    std::vector<int32_t> ids((size_t)n0);
    for (int i = 0; i < n0; i++) ids[i] = i;
    if (n0 > 0) GCNHIP_CHECK(gcnhip_h2d(ctx, d_labels, ids.data(), (size_t)n0 * sizeof(int32_t)));
    run.communities = n0;
    for (int level = 0; level < max_levels; level++) {
        int64_t info[8];
        GCNHIP_CHECK(gcnhip_louvain_level(ctx, cur.n, cur.entries, cur.ptr, cur.len, cur.idx, cur.w, cur.self_w, max_sweeps, d_comm, d_long, info, scratch, bytes));
        run.levels.push_back({cur.n, info[0], info[2]});
        run.numerator = info[2];
        run.m2 = info[3];
        if (!info[1]) break;
        int32_t *base = d_int + 4 * nn + (size_t)(level & 1) * (2 * nn + 2 * ne);
        int32_t *c_ptr = base, *c_len = base + nn, *c_idx = base + 2 * nn;
        uint32_t *c_w = (uint32_t *)(base + 2 * nn + ne);
        int64_t *c_self = d_long + nn + (size_t)(level & 1) * nn;
        int64_t cinfo[2];
        GCNHIP_CHECK(gcnhip_louvain_coarsen(ctx, cur.n, cur.entries, cur.ptr, cur.len, cur.idx, cur.w, cur.self_w, d_comm, d_label, c_ptr, c_len, c_idx, c_w,
                                            c_self, cinfo, scratch, bytes, 0));
        GCNHIP_CHECK(gcnhip_louvain_compose(ctx, d_labels, n0, d_label, cur.n));
        if (level_labels && level < level_capacity) GCNHIP_CHECK(gcnhip_d2h(ctx, level_labels + (size_t)level * n0, d_labels, (size_t)n0 * sizeof(int32_t)));
        cur = {c_ptr, c_len, c_idx, c_w, c_self, (int)cinfo[0], cinfo[1]};
        run.communities = cinfo[0];
    }
    if (contingency && !m.opt_.multilabel && m.params.output_dim <= 64 && run.communities >= 1 && run.communities <= 256) {
        const int C = m.params.output_dim, k = (int)run.communities;   // the clusterings' path: at most 256 rows of the table
        if (!d_label_all) d_label_all = arena.upload(m.data->label.data() + m.row_start(), (size_t)m.n_local);
        GCNHIP_CHECK(gcnhip_h2d(ctx, d_comm, ids.data(), (size_t)n0 * sizeof(int32_t)));
        int32_t *d_cont = d_db_cont.need((size_t)k * C + 1);   // {counts [k x C] | skipped}
        GCNHIP_CHECK(gcnhip_contingency_rows(ctx, d_labels, d_label_all, m.n_local, d_comm, n0, k, C, d_cont, d_cont + (size_t)k * C));
        std::vector<int32_t> cnt((size_t)k * C + 1);
        GCNHIP_CHECK(gcnhip_d2h(ctx, cnt.data(), d_cont, cnt.size() * sizeof(int32_t)));
        for (size_t e = 0; e < (size_t)k * C; e++) contingency[e] = cnt[e];
        run.contingency_rows = k;
        run.skipped = cnt[(size_t)k * C];
    }
    if (labels && n0 > 0) GCNHIP_CHECK(gcnhip_d2h(ctx, labels, d_labels, (size_t)n0 * sizeof(int32_t)));
    m.sync();
    return run;
}
