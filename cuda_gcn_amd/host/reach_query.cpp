// reach_query.cpp — ModelQueries::label_distance / components / reach: how far the model's nodes are from the labels it learns
// from, and which of them hang together, found where the adjacency lies (queries.h has the contract, csrc/reach.hip the
// definitions and the kernels, host/reach.h the measures).  Off the epoch path: no training module is touched; the one forward of
// reach() is predict()'s.
#include "queries.h"
#include "gcn.h"
#include "hip_check.h"
#include "reach.h"
#include <algorithm>

namespace {
constexpr size_t RC_SCRATCH = GCNHIP_REACH_SCRATCH, RC_TOTALS = 6, RC_STRATA = (size_t)(REACH_MAX_HOPS + 2) * 4;
}

int64_t ModelQueries::reach_rows(const char *what, int split, const int *nodes, int n, int source_mask, const int *source_nodes, int n_sources,
                                 int max_hops, int hops, bool predicted) {
    const std::string w = std::string(what) + ": ";
    require(what, ONE_RANK | (predicted ? SINGLE_LABEL | CLASS_AGGREGATION : 0));
    if (hops < 1 || hops > REACH_MAX_HOPS) throw GcnHipFailure(-1, w + "hops must be in 1..32, got " + std::to_string(hops));
    if (max_hops < 0) throw GcnHipFailure(-1, w + "max_hops must be at least 0 (0: no limit), got " + std::to_string(max_hops));
    if (split < 0 || split > 3) throw GcnHipFailure(-1, w + "invalid argument (split is 0 with a node query, or 1 train, 2 validation, 3 test)");
    if (source_mask & ~0xE) throw GcnHipFailure(-1, w + "invalid argument (the source splits are 1 train, 2 validation, 3 test)");
    if (n < 0 || n_sources < 0 || (!source_mask && n_sources > 0 && !source_nodes)) throw GcnHipFailure(-1, w + "invalid argument");
    reach_sources(what, source_mask, source_nodes, n_sources); // a node id outside the graph is refused here
    int listed = n;
    kmeans_list(what, split, nodes, listed);
    return listed;
}

std::vector<int> ModelQueries::reach_sources(const char *what, int source_mask, const int *source_nodes, int n_sources) {
    std::vector<int> rows;
    if (source_mask) {
        const int r0 = m.row_start();
        for (int r = 0; r < m.n_local; r++) {
            const int s = m.data->split[r0 + r];
            if (s >= 1 && s <= 3 && (source_mask >> s & 1)) rows.push_back(r);
        }
    } else if (n_sources > 0) {
        query_rows(what, source_nodes, n_sources, rows);
    }
    return rows;
}

void ModelQueries::reach_traverse(const std::vector<int> &sources, int max_hops, bool want_nearest, int64_t *level_counts, int capacity, Reach &res) {
    gcnhip_ctx *ctx = m.env.ctx;
    const size_t nl = (size_t)m.n_local;
    int32_t *d_seeds = d_rc_seeds.need(sources.size()), *d_dist = d_rc_dist.need(nl), *d_near = want_nearest ? d_rc_nearest.need(nl) : nullptr;
    int64_t *d_counts = d_rc_counts.need(RC_SCRATCH + RC_TOTALS + RC_STRATA + 1);
    if (!sources.empty()) GCNHIP_CHECK(gcnhip_h2d(ctx, d_seeds, sources.data(), sources.size() * sizeof(int32_t)));
    int64_t first = 0;
    const bool own = !level_counts || capacity < 1;            // the count of level 0 is wanted either way
    GCNHIP_CHECK(gcnhip_hop_distance(ctx, m.graph, d_seeds, (int)sources.size(), max_hops, d_dist, d_near, d_counts, &res.levels,
                                     own ? &first : level_counts, own ? 1 : capacity, &res.skipped));
    res.sources = own ? first : level_counts[0];
}

void ModelQueries::reach_components(const std::vector<int> &sources, int64_t *totals, Reach &res) {
    gcnhip_ctx *ctx = m.env.ctx;
    const size_t nl = (size_t)m.n_local;
    std::vector<int32_t> mark(std::max<size_t>(nl, 1), 0);
    for (int r : sources) mark[r] = 1;
    int32_t *d_mark = d_rc_mark.need(nl), *d_comp = d_rc_comp.need(nl), *d_size = d_rc_size.need(nl), *d_marked = d_rc_marked.need(nl);
    int64_t *d_counts = d_rc_counts.need(RC_SCRATCH + RC_TOTALS + RC_STRATA + 1);
    GCNHIP_CHECK(gcnhip_h2d(ctx, d_mark, mark.data(), mark.size() * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_components(ctx, m.graph, d_comp, d_counts, &res.rounds));
    GCNHIP_CHECK(gcnhip_component_counts(ctx, d_comp, d_mark, m.n_local, d_size, d_marked, d_counts + RC_SCRATCH));
    int64_t h[RC_TOTALS];
    GCNHIP_CHECK(gcnhip_d2h(ctx, h, d_counts + RC_SCRATCH, sizeof h));
    if (totals) std::copy(h, h + RC_TOTALS, totals);
}

void ModelQueries::reach_pick(const int32_t *d_per_row, const std::vector<int> &rows, bool as_node, int32_t *out) {
    if (!out || rows.empty()) return;
    std::vector<int32_t> all((size_t)std::max(m.n_local, 1));
    if (m.n_local > 0) GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, all.data(), d_per_row, (size_t)m.n_local * sizeof(int32_t)));
    for (size_t i = 0; i < rows.size(); i++) {
        const int32_t x = all[rows[i]];
        out[i] = as_node && x >= 0 && x < m.n_local ? m.node_id(x) : x;
    }
}

ModelQueries::Reach ModelQueries::label_distance(int source_mask, const int *source_nodes, int n_sources, int split, const int *nodes, int n, int max_hops,
                                                 int32_t *dist, int32_t *nearest, int64_t *level_counts, int capacity) {
    const char *what = "label_distance";
    Reach res;
    res.rows = reach_rows(what, split, nodes, n, source_mask, source_nodes, n_sources, max_hops, 1, false);   // every refusal, before any launch
    if (capacity < 0 || (capacity > 0 && !level_counts)) throw GcnHipFailure(-1, std::string(what) + ": invalid argument");
    const std::vector<int> rows = kmeans_list(what, split, nodes, n);
    const std::vector<int> sources = reach_sources(what, source_mask, source_nodes, n_sources);
    m.sync();                                                  // run()'s epochs in flight, the validation lane's pass
    reach_traverse(sources, max_hops, nearest != nullptr, level_counts, capacity, res);
    std::vector<int32_t> d(rows.size());
    reach_pick(d_rc_dist.p, rows, false, d.data());
    for (int32_t x : d) res.unreachable += x < 0;
    if (dist) std::copy(d.begin(), d.end(), dist);
    if (nearest) reach_pick(d_rc_nearest.p, rows, true, nearest);
    m.sync();
    return res;
}

ModelQueries::Reach ModelQueries::components(int split, const int *nodes, int n, int source_mask, const int *source_nodes, int n_sources,
                                             int32_t *component, int32_t *size, int64_t *totals) {
    const char *what = "components";
    Reach res;
    res.rows = reach_rows(what, split, nodes, n, source_mask, source_nodes, n_sources, 0, 1, false);
    const std::vector<int> rows = kmeans_list(what, split, nodes, n);
    const std::vector<int> sources = reach_sources(what, source_mask, source_nodes, n_sources);
    m.sync();
    reach_components(sources, totals, res);
    if (size && !rows.empty()) {                               // the size sits at the root: picked through the row's label
        std::vector<int32_t> comp(rows.size()), all((size_t)std::max(m.n_local, 1));
        reach_pick(d_rc_comp.p, rows, false, comp.data());
        GCNHIP_CHECK(gcnhip_d2h(m.env.ctx, all.data(), d_rc_size.p, (size_t)m.n_local * sizeof(int32_t)));
        for (size_t i = 0; i < rows.size(); i++) size[i] = all[comp[i]];
    }
    reach_pick(d_rc_comp.p, rows, true, component);
    m.sync();
    return res;
}

ModelQueries::Reach ModelQueries::reach(int split, const int *nodes, int n, int source_mask, const int *source_nodes, int n_sources, int hops,
                                        bool predicted, int32_t *dist, int32_t *nearest, int32_t *component, int64_t *strata, int64_t *totals,
                                        int64_t *level_counts, int capacity) {
    const char *what = "reach";
    Reach res;
    res.rows = reach_rows(what, split, nodes, n, source_mask, source_nodes, n_sources, 0, hops, predicted);   // every refusal, before any launch
    if (capacity < 0 || (capacity > 0 && !level_counts)) throw GcnHipFailure(-1, std::string(what) + ": invalid argument");
    if (m.data->label.size() < (size_t)(m.row_start() + m.n_local)) throw GcnHipFailure(-1, std::string(what) + ": the dataset holds no label per node");
    const std::vector<int> rows = kmeans_list(what, split, nodes, n);
    const std::vector<int> sources = reach_sources(what, source_mask, source_nodes, n_sources);
    m.sync();                                                  // run()'s epochs in flight, the validation lane's pass
    gcnhip_ctx *ctx = m.env.ctx;
    const size_t nn = (size_t)n;
    int32_t *d_rows = d_rc_rows.need(nn);
    if (n > 0) GCNHIP_CHECK(gcnhip_h2d(ctx, d_rows, rows.data(), nn * sizeof(int32_t)));
    if (!d_label_all) d_label_all = arena.upload(m.data->label.data() + m.row_start(), (size_t)m.n_local);
    if (predicted) forward_predict(nullptr, false);            // d_pred of every local row; the logits are not stored
    reach_traverse(sources, 0, true, level_counts, capacity, res);
    reach_components(sources, totals, res);
    int64_t *d_strata = d_rc_counts.p + RC_SCRATCH + RC_TOTALS;
    const size_t cells = (size_t)(hops + 2) * 4;
    GCNHIP_CHECK(gcnhip_distance_strata(ctx, d_rc_dist.p, d_rc_nearest.p, predicted ? d_pred.p : nullptr, d_label_all, m.n_local, d_rows, n,
                                        m.params.output_dim, hops, d_strata, d_strata + cells));
    std::vector<int64_t> h(cells + 1);
    GCNHIP_CHECK(gcnhip_d2h(ctx, h.data(), d_strata, h.size() * sizeof(int64_t)));
    if (strata) std::copy(h.begin(), h.begin() + cells, strata);
    res.unlabelled = h[cells];
    res.unreachable = h[(size_t)(hops + 1) * 4];
    reach_pick(d_rc_dist.p, rows, false, dist);
    reach_pick(d_rc_nearest.p, rows, true, nearest);
    reach_pick(d_rc_comp.p, rows, true, component);
    m.sync();
    return res;
}
