// gcn_schedule.cpp — what HipGCN decides about a graph at load: the node order (several GPUs), the aggregation's row
// schedule and the column-slice width of the hidden-width launch.
#include "gcn.h"
#include "cluster.h"
#include <cstdio>
#include <cstring>
#include "hip_check.h"

// Rank blocks are contiguous ranges of the node order.  When the order the dataset came in forces the all-gather (the
// neediest rank would read more than 75 % of the other ranks' rows) the graph is priced under orders derived from its
// structure (partition.h); if one of them gets by with halo lists, the dataset is renumbered once, here, before anything
// is built from it.  Every rank computes the same answer.
void HipGCN::renumber_nodes(int world) {
    const int N = params.num_nodes;
    const std::vector<int> &gp = data->graph.indptr, &gi = data->graph.indices;
    const bool force = (flags & HIPGCN_STRUCTURE_PARTITION) != 0;
    StructureGroups sg;
    const OrderCost ids = exchange_cost(gp.data(), gi.data(), N, world);
    if ((force || ids.halo_share > 0.75) && N >= 4096) sg = structure_groups(gp.data(), gi.data(), N);
    NodeOrderChoice ch = choose_node_order(gp.data(), gi.data(), N, world, sg.useful ? sg.group.data() : nullptr, force);
    if (ch.order.empty()) return;
    if (env.comm->rank() == 0 && opt_.verbose)
        fprintf(stderr, "gcn-hip: nodes renumbered by %s: neediest rank reads %ld rows per exchange instead of %ld (all-gather: %ld)\n",
                ch.name, ch.chosen.recv_rows_max, ch.ids.recv_rows_max, (long)(world - 1) * ch.ids.rows_max);
    renumbered.reset(new GCNData());
    GCNData &d = *renumbered;
    permute_csr(gp.data(), gi.data(), N, ch.order, d.graph.indptr, d.graph.indices);
    const std::vector<int> &fp = data->feature_index.indptr, &fi = data->feature_index.indices;
    d.feature_index.indptr.assign((size_t)N + 1, 0);
    for (int k = 0; k < N; k++) d.feature_index.indptr[k + 1] = d.feature_index.indptr[k] + (fp[ch.order[k] + 1] - fp[ch.order[k]]);
    d.feature_value.resize(data->feature_value.size());
    if (!fi.empty()) d.feature_index.indices.resize(fi.size());
    d.split.resize(N); d.label.resize(N);
    for (int k = 0; k < N; k++) {
        const int o = ch.order[k];
        const size_t n = (size_t)(fp[o + 1] - fp[o]), dst = (size_t)d.feature_index.indptr[k];
        if (n) memcpy(&d.feature_value[dst], &data->feature_value[(size_t)fp[o]], n * sizeof(float));
        if (n && !fi.empty()) memcpy(&d.feature_index.indices[dst], &fi[(size_t)fp[o]], n * sizeof(int));
        d.split[k] = data->split[o];
        d.label[k] = data->label[o];
    }
    if (!data->multihot.empty()) {                     // multi-label rows follow their node
        const size_t wpr = data->multihot.size() / N;
        d.multihot.resize(data->multihot.size());
        for (int k = 0; k < N; k++)
            std::copy(data->multihot.begin() + (size_t)ch.order[k] * wpr, data->multihot.begin() + ((size_t)ch.order[k] + 1) * wpr,
                      d.multihot.begin() + (size_t)k * wpr);
    }
    node_order_ = std::move(ch.order);
    node_order_name_ = ch.name;
    data = renumbered.get();
}

// Which rows the aggregation has in flight together decides its speed (what the XCD L2s hold; whether hub rows
// overlap with the tail of short rows) and nothing else: every schedule gives the same bits.  Candidates:
// descending degree; label-major when the labels are communities of this graph (Reddit: subreddits), else group-major over
// groups found in the graph by modularity local moving (cluster.h) when that finds any; degree rank
// dealt into 256 equal-mix groups (graphs with a long tail of short rows, e.g. R-MAT).  Each is timed on the
// hidden-width aggregation of this rank's rows and the fastest is kept for all of this rank's adjacency objects.
void HipGCN::apply_schedule(gcnhip_ctx *ctx, gcnhip_graph *g) {
    const int r0 = part.start[env.comm->rank()];
    if (sched_mode == 3)                                      // groups found in the graph: the same group-major order as labels
        GCNHIP_CHECK(gcnhip_graph_set_schedule(ctx, g, 1, structure_group.data() + r0, 0));
    else
        GCNHIP_CHECK(gcnhip_graph_set_schedule(ctx, g, sched_mode, sched_mode == 1 ? data->label.data() + r0 : nullptr, sched_groups));
}

// Column-slice width of the XCD-sliced hidden-width launch (round 5): 64-float slices (two per 128-wide row: each XCD's L2
// sees half the table) or 32-float slices (four: a quarter of the table per L2, twice the re-reads of the index stream,
// 128-byte requests).  Which wins depends on where the graph's reuse sits (tools/exp_structure.py, bench.py's structure legs):
// with row groups that fit an L2 and hold most of the edges the wide slices do (reddit-syn: 0.76 vs 0.84 ms); on a graph whose
// reuse is its hub rows the narrow ones (reddit-syn-h0: 1.22 vs 1.11 ms; -h03 1.02 vs 0.98; -zipf 0.97 vs 0.89); past the
// Infinity Cache the wide ones again (R-MAT scale 21: 4.57 vs 5.20 ms).  The two widths split a row's sum over 4 or 8 lane
// groups, i.e. associate it differently, so the choice must NOT depend on a timing (two runs of one dataset print the same
// bits): it is a rule on the graph — narrow when the gathered table is cache-resident and less than 45 % of the stored
// edges stay inside a row group (label or found community) whose 256-byte slices fit half an L2 (8192 rows).
void HipGCN::choose_slice_width() {
    const int N = params.num_nodes, H = params.hidden_dim;
    slice_floats = 64;
    int cur_gl = 0;
    GCNHIP_CHECK(gcnhip_ctx_get_option(env.ctx, "gs_l", &cur_gl));
    if (cur_gl == 8 || cur_gl == 4) {                      // preset (GCNHIP_GS_L): report what the launches will use; the lane mirrors it
        const int f = cur_gl * 4;
        if (H % f == 0 && H / f > 1 && H / f <= 8 && 8 % (H / f) == 0) slice_floats = f;
        return;
    }
    if (cur_gl != 0 || !opt_.slice_tuning || H % 64 != 0 || H / 32 > 8 || 8 % (H / 32) != 0) return;
    if ((size_t)N * H * sizeof(float) > ((size_t)256 << 20)) return;                 // HBM regime: wide
    // (the groups the schedule candidates were built from — labels when they are communities of the graph, else what the
    //  group search found — NOT the candidate the timing picked: every schedule gives the same bits, the slice width does not)
    const int *group = labels_assortative ? data->label.data() : (!structure_group.empty() ? structure_group.data() : nullptr);
    double share = 0.0;
    if (group) {
        std::vector<int> size;
        for (int i = 0; i < N; i++) {
            if (group[i] < 0) continue;
            if ((size_t)group[i] >= size.size()) size.resize((size_t)group[i] + 1, 0);
            size[group[i]]++;
        }
        const std::vector<int> &gp = data->graph.indptr, &gi = data->graph.indices;
        long inside = 0, total = 0;
        for (int i = 0; i < N; i++)
            for (int e = gp[i]; e < gp[i + 1]; e++) {
                if (gi[e] == i) continue;
                total++;
                inside += group[i] >= 0 && group[gi[e]] == group[i] && size[group[i]] <= 8192;
            }
        share = total ? (double)inside / (double)total : 0.0;
    }
    slice_floats = share < 0.45 ? 32 : 64;
    GCNHIP_CHECK(gcnhip_ctx_set_option(env.ctx, "gs_l", slice_floats == 32 ? 8 : 0));
    if (opt_.verbose && env.comm->rank() == 0)
        fprintf(stderr, "gcn-hip: hidden-width aggregation: %.0f %% of the edges inside a row group that fits an L2 -> %d-float column slices\n",
                100 * share, slice_floats);
}

void HipGCN::tune_schedule() {
    if (n_local < 4096 && opt_.schedule < 0) return;         // launch-bound graphs: nothing to gain
    const int H = params.hidden_dim;
    gcnhip_graph *g = replicate_l1 ? graph_l1 : graph;       // the layer-1 aggregation, the widest one
    if (opt_.schedule >= 0) {
        // pinned (HIPGCN_SCHEDULE): no candidate is timed, so no tuning launch shares a kernel name with the epochs' launches
        sched_mode = opt_.schedule; sched_groups = opt_.schedule == 2 ? opt_.schedule_groups : 0;
        if (sched_mode == 3 && structure_group.empty()) sched_mode = 0;      // the search found no usable groups
        if (sched_mode == 3) sched_groups = structure_n_groups;
        if (sched_mode != 0) {
            apply_schedule(env.ctx, graph);
            if (graph_l1) apply_schedule(env.ctx, graph_l1);
        }
        choose_slice_width();
        return;
    }
    // the slice width first (a rule on the graph, not a timing): the candidates are timed with the launch the epochs will use
    choose_slice_width();
    HipVariable *in = variables[1].get(), *out = variables[3].get();
    float *src = in->full ? in->full : in->data;
    const size_t src_elems = in->full ? in->full_elems : in->elems();
    GCNHIP_CHECK(gcnhip_memset_async(env.ctx, src, 0, src_elems * sizeof(float)));
    struct Cand { int mode, groups; };
    std::vector<Cand> cands = {{0, 0}, {2, 256}};
    if (labels_assortative) cands.push_back({1, 0});
    if (!structure_group.empty()) cands.push_back({3, structure_n_groups});
    void *e0, *e1;
    GCNHIP_CHECK(gcnhip_event_create(&e0));
    GCNHIP_CHECK(gcnhip_event_create(&e1));
    float best = 0.f;
    Cand pick = cands[0];
    // the candidates are timed with the launch the epoch uses: the factored operator (no coefficient stream, 6-10 % of a
    // launch) on the fused f32 path, the reference's per-edge coefficients otherwise
    gcnhip_gs_opts gso;
    memset(&gso, 0, sizeof gso);
    gso.scaling = factored_ ? 2 : 0;
    bool fresh = true;                                       // g still has the schedule it was built with: descending degree = candidate 0
    for (const Cand &c : cands) {
        sched_mode = c.mode; sched_groups = c.groups;
        if (!(fresh && c.mode == 0)) apply_schedule(env.ctx, g);
        fresh = false;
        float ms = 0.f;
        // two launches warm the caches, size the scratch and let the clock settle, five are timed.  (Until round 6: one and
        // two — on reddit-syn-h0, where the candidates are 5 % apart, the driver's run picked plain degree order, 245 epochs/s,
        // where the same tree had picked dealt-256 an hour earlier, 254.)
        for (int it = 0; it < 7; it++) {
            if (it == 2) GCNHIP_CHECK(gcnhip_event_record(env.ctx, e0));
            GCNHIP_CHECK(gcnhip_graphsum_ex(env.ctx, g, &gso, src, in->ld, out->data, out->ld, H));
        }
        GCNHIP_CHECK(gcnhip_event_record(env.ctx, e1));
        GCNHIP_CHECK(gcnhip_event_elapsed_ms(e0, e1, &ms));
        if (best == 0.f || ms < best) { best = ms; pick = c; }
    }
    const bool g_has_pick = sched_mode == pick.mode && sched_groups == pick.groups;    // the last candidate timed is still applied to g
    sched_mode = pick.mode; sched_groups = pick.groups;
    if (!(g == graph && g_has_pick)) apply_schedule(env.ctx, graph);
    if (graph_l1 && !(g == graph_l1 && g_has_pick)) apply_schedule(env.ctx, graph_l1);
    gcnhip_event_destroy(e0);
    gcnhip_event_destroy(e1);
    GCNHIP_CHECK(gcnhip_memset_async(env.ctx, out->data, 0, out->elems() * sizeof(float)));
}
