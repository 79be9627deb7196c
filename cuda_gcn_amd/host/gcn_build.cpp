// gcn_build.cpp — HipGCN's construction and teardown: argument checks, device objects and buffers, module wiring, the
// validation lane, release.  (What init() decides about the graph on the way is in gcn_schedule.cpp.)
#include "gcn.h"
#include "queries.h"
#include "class_weights.h"
#include "cluster.h"
#include <chrono>
#include <future>
#include <cstdio>
#include "hip_check.h"

GCNParams GCNParams::get_default() { return {2708, 1433, 16, 7, 0.5, 0.01, 5e-4, 100, 0}; }

namespace {
// Are the labels communities of THIS graph?  Edge homophily (share of stored non-loop edges whose two ends carry
// the same label) against what label frequencies alone would give; the hint is used at twice chance or more.
bool labels_are_assortative(const GCNData &d, int N, int C) {
    if ((int)d.label.size() != N || C <= 1) return false;
    const std::vector<int> &gp = d.graph.indptr, &gi = d.graph.indices;
    std::vector<double> freq(C, 0.0);
    for (int i = 0; i < N; i++) {
        if (d.label[i] < 0 || d.label[i] >= C) return false;
        freq[d.label[i]] += 1.0;
    }
    double chance = 0;
    for (int c = 0; c < C; c++) chance += (freq[c] / N) * (freq[c] / N);
    long same = 0, total = 0;
    for (int i = 0; i < N; i++)
        for (int e = gp[i]; e < gp[i + 1]; e++) {
            if (gi[e] == i) continue;
            total++;
            same += d.label[gi[e]] == d.label[i];
        }
    return total > 0 && (double)same / (double)total >= 2.0 * chance;
}
}  // namespace

HipGCN::HipGCN(GCNParams p, GCNData *input_data, const HipGCNOptions &opt) : params(p), data(input_data), flags(opt.flags) {
    // a constructor that throws runs no destructor: release whatever init() had built before the failure
    try {
        init(opt);
    } catch (...) {
        release();
        throw;
    }
}

void HipGCN::init(const HipGCNOptions &opt) {
    device_ = opt.device;
    opt_ = opt;                 // every switch comes from the options (HipGCNOptions::from_environment for the HIPGCN_* variables)
    // opt.verbose: where the model build's wall time goes (stderr), phase by phase
    const bool verbose = opt.verbose && opt.rank == 0;
    auto t_phase = std::chrono::steady_clock::now();
    auto phase = [&](const char *what) {
        if (!verbose) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "gcn-hip: build %-34s %8.3f s\n", what, std::chrono::duration<double>(now - t_phase).count());
        t_phase = now;
    };
    // argument checks first: nothing is allocated for a request that cannot be served
    if (opt.world > 1 && !opt.comm && !opt.host_allgather && !(flags & HIPGCN_NULL_COMM) && !opt.nccl_id)
        throw GcnHipFailure(-1, "world > 1 needs an RCCL unique id");
    if (params.num_nodes < 1 || params.hidden_dim < 1 || params.output_dim < 1 || params.input_dim < 1)
        throw GcnHipFailure(-1, "HipGCN: empty model dimensions");
    if ((int)data->graph.indptr.size() != params.num_nodes + 1 || (int)data->split.size() != params.num_nodes ||
        (int)data->label.size() != params.num_nodes || (int)data->feature_index.indptr.size() != params.num_nodes + 1)
        throw GcnHipFailure(-1, "HipGCN: GCNData arrays do not match num_nodes");
    if (opt.multilabel) {
        if (params.output_dim > 256) throw GcnHipFailure(-1, "HipGCN: multi-label mode takes at most 256 classes");
        if (data->multihot.size() != (size_t)params.num_nodes * ((params.output_dim + 31) / 32))
            throw GcnHipFailure(-1, "HipGCN: the multi-hot label matrix does not hold num_nodes rows of ceil(output_dim / 32) words");
    }
    if (!opt.class_weights.empty()) {
        std::string why;
        if (params.output_dim > 256) throw GcnHipFailure(-1, "HipGCN: class weights take at most 256 classes");
        if (gcn_class_weights_check(opt.class_weights.data(), opt.class_weights.size(), params.output_dim, &why) != 0)
            throw GcnHipFailure(-1, "HipGCN: " + why);
        if (!opt.multilabel)                           // every rank holds the whole dataset: the sums are global and the same everywhere
            for (int s = 1; s <= 3; s++) {
                bool any = false;
                for (int i = 0; i < params.num_nodes && !any; i++) any = data->split[i] == s;
                const double ws = gcn_class_weight_sum(params.num_nodes, params.output_dim, data->split.data(), data->label.data(), s,
                                                       opt.class_weights.data());
                if (any && !(ws > 0))
                    throw GcnHipFailure(-1, "HipGCN: the class weights of split " + std::to_string(s) + "'s rows sum to 0 (its weighted mean is undefined)");
                split_wsum[s] = (float)ws;
            }
    }
    GCNHIP_CHECK(gcnhip_ctx_create(&env.ctx, opt.device, nullptr));
    arena.bind(env.ctx);
    queries_.reset(new ModelQueries(*this));                    // allocates nothing until the first query
    if (opt.gemm >= 0) GCNHIP_CHECK(gcnhip_ctx_set_option(env.ctx, "gemm_bf16x3", opt.gemm ? 2 : 0));   // HIPGCN_GEMM; else the library's default
    timers.reset(new DeviceTimers(env.ctx));
    timers->enabled = (flags & HIPGCN_TIMERS) != 0;
    env.timers = timers.get();
    if (opt.comm) {
        if (opt.own_comm) owned_comm.reset(opt.comm);
    } else if (opt.world > 1 && opt.host_allgather) {
        owned_comm.reset(make_host_comm(env.ctx, opt.rank, opt.world, opt.host_allgather, opt.host_allreduce, opt.host_user));
    } else if (opt.world > 1 && (flags & HIPGCN_NULL_COMM)) {
        owned_comm.reset(new NullComm(opt.rank, opt.world));
    } else if (opt.world > 1) {                                // (an id is there: checked above)
        owned_comm.reset(make_rccl_comm(env.ctx, opt.rank, opt.world, opt.nccl_id));
    } else {
        owned_comm.reset(new SelfComm());
    }
    env.comm = opt.comm ? opt.comm : owned_comm.get();
    env.seed = (uint64_t)opt.seed * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull;
    env.bf16_tables = (flags & HIPGCN_BF16_TABLES) != 0;
    // The factored aggregation (gcnhip_graphsum_ex): no per-edge coefficient stream; the gathered matrices are stored
    // pre-multiplied by dinv of their row (the producers fold the factor into a row-wise epilogue or a value array).  The
    // fused f32 path only; HIPGCN_EDGE_COEF restores the reference's per-edge coefficients.
    factored_ = !(flags & (HIPGCN_MODULAR | HIPGCN_BF16_TABLES | HIPGCN_EDGE_COEF));
    const int world = env.comm->size(), rank = env.comm->rank();
    const int N = params.num_nodes, F = params.input_dim, H = params.hidden_dim, C = params.output_dim;

    // ---- node order (several GPUs: by structure when the ids carry no locality), row partition, this rank's slice
    // How remote rows will arrive is decided BEFORE the node order: renumbering exists to turn an all-gather into halo
    // lists, so a run whose exchange is pinned to the all-gather (the flag, HIPGCN_EXCHANGE=allgather, or the default over
    // RCCL until the halo exchange has met a peer) keeps its ids — no second host copy of X, no group search, and rows,
    // dropout decisions and get_var() stay in the dataset's order.
    int exchange_mode = (flags & HIPGCN_EXCHANGE_HALO) ? 2 : ((flags & HIPGCN_EXCHANGE_ALLGATHER) ? 1 : 0);
    if (opt.exchange >= 0) exchange_mode = opt.exchange;
    // Over RCCL the per-graph decision is opt-in (HIPGCN_EXCHANGE=auto|halo, or the flag): the halo exchange is a grouped
    // ncclSend/ncclRecv that has run against real peers only in gcnhost_rccl_selftest_world, so an unasked-for run takes
    // the in-place all-gather.  bench.py's launcher runs that self-test as a throw-away group of ranks and then asks
    // for `auto`.  (Host-staged transports and tests decide per graph as before.)
    const bool over_rccl = world > 1 && !opt.comm && !opt.host_allgather && !(flags & HIPGCN_NULL_COMM);
    if (over_rccl && exchange_mode == 0 && opt.exchange != 0) exchange_mode = 1;
    // Parity mode (HIPGCN_HOST_MASKS) replays the reference's RNG stream in the DATASET's element order
    // (host_masks_for_epoch): a renumbered run would hand node k's decisions to another node, so it keeps its ids too
    // (HIPGCN_STRUCTURE_PARTITION still forces the renumbering; the run is then the parity run of the renumbered dataset).
    const bool may_renumber = world > 1 && !(flags & HIPGCN_ID_PARTITION) &&
                              ((flags & HIPGCN_STRUCTURE_PARTITION) || (exchange_mode != 1 && !(flags & HIPGCN_HOST_MASKS)));
    if (may_renumber) renumber_nodes(world);
    phase("context, comm, node order");
    const std::vector<int> &gp = data->graph.indptr, &gi = data->graph.indices;
    part = make_partition(gp.data(), N, world);
    const int r0 = part.start[rank], r1 = part.start[rank + 1];
    n_local = r1 - r0;
    nnzA_local = (long)gp[r1] - gp[r0];
    labels_assortative = !(flags & (HIPGCN_NO_ROW_GROUPS | HIPGCN_NO_LABEL_HINT)) && labels_are_assortative(*data, N, C);
    // no usable labels: look for row groups in the graph itself (one pass over the edges per sweep, every rank the same
    // result); whether they are used is decided by timing, like every other schedule (tune_schedule)
    // (on a host thread beside the object builds and H2D copies below: one sweep over an R-MAT graph of scale 22 is 3 s, and its
    //  result is not needed before the schedules are timed)
    std::future<StructureGroups> groups_search;
    if (!(flags & HIPGCN_NO_ROW_GROUPS) && !labels_assortative && n_local >= 4096 && opt.structure_groups &&
        (opt.schedule < 0 || opt.schedule == 3 || opt.slice_tuning))   // the slice rule reads the groups whatever picked the schedule
        groups_search = std::async(std::launch::async, [&gp, &gi, N]() { return structure_groups(gp.data(), gi.data(), N); });
    struct JoinGroups {                       // never leave the thread running over a dataset that is being torn down
        std::future<StructureGroups> &f;
        ~JoinGroups() { if (f.valid()) f.wait(); }
    } join_groups{groups_search};
    phase("labels / structure groups");
    xplan = make_exchange_plan(gp.data(), gi.data(), N, part, rank, exchange_mode);
    env.plan = &xplan;
    env.xbuf = &xbuf;
    if (world > 1) {
        const LocalGraph lg = build_table_graph(gp.data(), gi.data(), N, part, xplan);
        GCNHIP_CHECK(gcnhip_graph_create(env.ctx, &graph, lg.indptr.data(), lg.indices.data(), lg.n_rows, lg.n_cols, lg.col_deg.data()));
    } else {
        GCNHIP_CHECK(gcnhip_graph_create(env.ctx, &graph, gp.data(), gi.data(), N, N, nullptr));
    }
    GCNHIP_CHECK(gcnhip_graph_reserve_width(env.ctx, graph, std::max(params.hidden_dim, params.output_dim)));
    phase("adjacency object (gcnhip_graph_create)");
    const std::vector<int> &fp = data->feature_index.indptr, &fi = data->feature_index.indices;
    const long f0 = fp[r0], f1 = fp[r1];
    {
        std::vector<int> lp(n_local + 1);
        for (int r = 0; r <= n_local; r++) lp[r] = fp[r0 + r] - fp[r0];
        GCNHIP_CHECK(gcnhip_feat_create(env.ctx, &feat, lp.data(), fi.empty() ? nullptr : fi.data() + f0,
                                        data->feature_value.data() + f0, n_local, F));
    }
    // Replicating X.W1 trades a 119 MB all-gather per forward for 0.4 ms of extra GEMM on every rank.  With 2-4
    // GPUs each rank receives over 1-3 xGMI links (~60 GB/s each) and the GEMM is cheaper; with 8 GPUs seven
    // links feed the gather (~0.3 ms) while the replicated GEMMs would be 45 % of the per-rank compute.
    // (ALLGATHER plans only: a HALO plan moves few rows, and its table is not in global row order)
    replicate_l1 = world > 1 && !xplan.halo && (world <= 4 || (flags & HIPGCN_REPLICATE_L1)) && !(flags & (HIPGCN_NO_REPLICATE_L1 | HIPGCN_MODULAR));
    if (replicate_l1) {
        GCNHIP_CHECK(gcnhip_feat_create(env.ctx, &feat_full, fp.data(), fi.empty() ? nullptr : fi.data(),
                                        data->feature_value.data(), N, F));
        full_vals = gcnhip_feat_values(feat_full);
        graph_l1 = create_rows_graph(env.ctx);
    }
    phase("feature objects (gcnhip_feat_create)");
    // truth per split, once (the reference rebuilds and re-uploads it per call: cuda_gcn.cu:85-97)
    {
        int32_t *d_split = arena.upload(data->split.data() + r0, (size_t)n_local);
        int32_t *d_label = arena.upload(data->label.data() + r0, (size_t)n_local);
        double cnt[4] = {0, 0, 0, 0};
        for (int s = 1; s <= 3; s++) {
            d_truth[s] = arena.alloc<int32_t>((size_t)(n_local ? n_local : 1));
            GCNHIP_CHECK(gcnhip_set_truth(env.ctx, d_truth[s], d_split, d_label, n_local, s));
            for (int i = r0; i < r1; i++) cnt[s] += data->split[i] == s;
        }
        GCNHIP_CHECK(gcnhip_ctx_sync(env.ctx));
        arena.release(d_split);
        arena.release(d_label);
        env.comm->allreduce_sum_host(cnt, 4);
        for (int s = 1; s <= 3; s++) split_count[s] = (int)cnt[s];
        if (opt.multilabel) {                          // this rank's rows, in the (possibly renumbered) row order of `data`
            ml_wpr = (C + 31) / 32;
            std::vector<uint32_t> mine(data->multihot.begin() + (size_t)r0 * ml_wpr, data->multihot.begin() + (size_t)r1 * ml_wpr);
            if (mine.empty()) mine.assign(ml_wpr, 0u);
            d_ml_truth = arena.upload(mine.data(), mine.size());
        }
        if (!opt.class_weights.empty()) d_class_w = arena.upload(opt.class_weights.data(), opt.class_weights.size());
    }

    // The last aggregation of a forward computes only the rows the loss and the accuracy read
    // (CrossEntropyLoss::forward skips truth < 0, module.cpp:131-133; get_accuracy, gcn.cpp:86-88):
    // one registered row subset per split.
    if (!(flags & HIPGCN_ALL_ROWS)) add_split_rowsets(env.ctx, graph, split_rows);
    if (!(flags & HIPGCN_MODULAR) || opt.multilabel || !opt.class_weights.empty()) {
        // the loss walks the rows of the scored split only (it skips the others anyway, module.cpp:131-133)
        for (int s = 1; s <= 3; s++) {
            std::vector<int32_t> rows;
            for (int r = 0; r < n_local; r++)
                if (data->split[r0 + r] == s) rows.push_back(r);
            split_local_n[s] = (int)rows.size();
            d_split_list[s] = arena.upload(rows.data(), rows.size());
        }
    }

    // training-split bit per table row (= node, on one GPU): dZ is zero elsewhere, GraphSum's backward skips those rows
    {
        const size_t n_pos = world > 1 ? (size_t)xplan.table_rows : (size_t)N;
        std::vector<uint32_t> bits(n_pos / 32 + 2, 0u);
        for (size_t t = 0; t < n_pos; t++) {
            const int j = world > 1 ? xplan.table_global[t] : (int)t;
            if (j >= 0 && data->split[j] == 1) bits[t >> 5] |= 1u << (t & 31);
        }
        d_train_bits = arena.upload(bits.data(), bits.size());
        bwd_bits = d_train_bits;
        h_train_bits = std::move(bits);
    }

    // ---- variables (numbering of gcn.cpp:21-54)
    variables.resize(7);
    for (auto &v : variables) v.reset(new HipVariable());
    const ExchangePlan *xp = world > 1 ? &xplan : nullptr;
    if (flags & HIPGCN_MODULAR) {
        variables[0]->alloc(env.ctx, 1, (int)(f1 - f0), false);
        input = variables[0].get();
        input_vals = input->data;
    } else {
        input_vals = gcnhip_feat_values(feat);
    }
    if (replicate_l1) variables[1]->alloc_replicated(env.ctx, N, n_local, r0, H, true);   // H0: every row computed here
    else variables[1]->alloc(env.ctx, n_local, H, true, true, false, xp);    // H0: data gathered
    variables[3]->alloc(env.ctx, n_local, H, true, false, true, xp);    // H1: grad gathered
    rebuild_dh1 = world > 1 && !(flags & (HIPGCN_GATHER_DH1 | HIPGCN_MODULAR));
    variables[4]->alloc(env.ctx, n_local, C, true, true, rebuild_dh1, xp);   // Z0: data gathered (+ grad when dH1 is rebuilt)
    variables[6]->alloc(env.ctx, n_local, C, true, false, true, xp);    // Z : grad gathered
    if (world > 1) {
        // widest row (in 4-byte words) an exchange will carry: f32 rows of H / C, mask words, bf16 rows
        const int ldH = variables[1]->ld, ldC = variables[4]->ld;
        exchange_buffers_create(env.ctx, xplan, std::max(std::max(ldH, ldC), (H + 63) / 64 * 64), &xbuf);
    }
    output = variables[6].get();
    HipVariable *W1 = variables[2].get(), *W2 = variables[5].get();
    W1->alloc(env.ctx, F, H, false);
    W2->alloc(env.ctx, H, C, false);
    // both weight gradients and the 4 loss/accuracy scalars share one buffer: one all-reduce per epoch
    gradbuf_elems = W1->elems() + W2->elems() + 4;
    {
        gradbuf = arena.alloc_zeroed<float>(gradbuf_elems);
        W1->grad = gradbuf; W1->requires_grad = true;
        W2->grad = gradbuf + W1->elems(); W2->requires_grad = true;
        d_result = gradbuf + W1->elems() + W2->elems();
        d_result_i = arena.alloc<int32_t>(4);                             // {correct, total}, or the multi-label {TP, FP, FN, rows}
        d_ring = arena.alloc_zeroed<float>((size_t)RING * 4 * 8);
        // two epoch words: [0] the epoch being (or about to be) trained, read by the training pass; [1] the epoch whose update
        // ran last, naming the metrics row of an evaluation on this stream.  Adam's launch moves both (gcnhip_adam_step_advance),
        // so an epoch starts without a counter launch.  Before the first update: 0 and -1 (the row an evaluation of the
        // initial weights has always used).
        env.d_epoch = arena.alloc<uint32_t>(2);
        env.d_epoch_done = env.d_epoch + 1;
        GCNHIP_CHECK(gcnhip_memset_async(env.ctx, env.d_epoch, 0, sizeof(uint32_t)));
        GCNHIP_CHECK(gcnhip_memset_async(env.ctx, env.d_epoch_done, 0xFF, sizeof(uint32_t)));
    }
    // Glorot with the reference's RNG and draw order: all of W1, then all of W2 (gcn.cpp:30,49)
    rng.seed_time((unsigned)opt.seed);
    {
        Variable h1(F * H), h2(H * C);
        h1.glorot(F, H, rng);
        h2.glorot(H, C, rng);
        W1->upload(h1.data.data());
        W2->upload(h2.data.data());
    }
    if (flags & HIPGCN_HOST_MASKS) {
        keep0_first = replicate_l1 ? 0 : f0;
        h_keep0.resize(replicate_l1 ? (size_t)fp[N] : (size_t)(f1 - f0));
        h_keep1.resize((size_t)n_local * H);
        d_keep0 = arena.alloc<uint8_t>(h_keep0.size() + 16);
        d_keep1 = arena.alloc<uint8_t>(h_keep1.size() + 16);
        env.keep_input = d_keep0;
        env.keep_input_bwd = d_keep0 + (f0 - keep0_first);
        env.keep_hidden = d_keep1;
    }
    phase("truth, row subsets, variables, Glorot");
    if (groups_search.valid()) {
        StructureGroups sg = groups_search.get();
        if (sg.useful) { structure_group = std::move(sg.group); structure_n_groups = sg.n_groups; }
        phase("structure groups (waited for)");
    }
    if (!(flags & HIPGCN_NO_ROW_GROUPS)) tune_schedule();
    phase("row schedules timed (tune_schedule)");
    // The output layer's backward aggregates dZ, which is zero outside the training split: the edges that point at those
    // rows leave the operator for good (a third of Reddit's, 95 % of Cora's) — after the row order has been chosen,
    // which the restricted object inherits.
    if (!(flags & HIPGCN_MASKED_BWD) && n_local > 0)
        GCNHIP_CHECK(gcnhip_graph_create_restricted(env.ctx, &graph_bwd_out, graph, h_train_bits.data()));
    // decided from world, flags and the storage format only — the same on every rank: the exchange lane's communicator is
    // an ncclCommSplit, a collective over the parent; a rank that owns no rows still creates it (and skips only the cuts)
    if ((flags & HIPGCN_OVERLAP_EXCHANGE) && world > 1 && !env.bf16_tables) build_overlap();
    build_modules();
    if (!(flags & (HIPGCN_NO_AGG_FIRST_EVAL | HIPGCN_MODULAR)) && gcnhip_feat_is_dense(feat) && n_local > 0) build_agg_first_eval();
    phase("restricted operator, modules, A^.X");
    if (factored_) apply_factored_scales();
    phase("factored scales");
    // opt-in everywhere: with several GPUs the lane brings a second communicator and the turnstile, which must be measured
    // on a multi-GPU node before they may become a default there (bench.py tries both schedules)
    if (!(flags & HIPGCN_NO_EVAL_LANE) && (flags & HIPGCN_EVAL_LANE)) {
        try {
            build_eval_lane();
        } catch (const GcnHipFailure &e) {
            // e.g. an RCCL without ncclCommSplit: every rank fails the same way and falls back to one lane
            fprintf(stderr, "gcn-hip: validation lane disabled (%s)\n", e.what());
            destroy_lane();
        }
    }
    AdamParams ap = AdamParams::get_default();
    ap.lr = params.learning_rate;
    ap.weight_decay = params.weight_decay;
    optimizer.reset(new HipAdam());
    optimizer->init(&env, {{W1, true}, {W2, false}}, ap, params.epochs > 0 ? params.epochs + 8 : 8);   // gcn.cpp:62-65
    GCNHIP_CHECK(gcnhip_ctx_sync(env.ctx));
    phase("validation lane, optimizer");
}

// The first layer of the factored model multiplies D^-1/2 X (and, for evaluation, D^-1/2 (A^ X)): the factor that the
// aggregation's input rows must carry rides in the value arrays, so no GEMM or sparse kernel changes, and the weight
// gradient X'^T . (raw sum) comes out as the reference's X^T . dH0.  Called once, after A^.X has been built from the
// unscaled X.
void HipGCN::apply_factored_scales() {
    const float *dinv_row = nullptr;
    GCNHIP_CHECK(gcnhip_graph_scales(graph, &dinv_row, nullptr, nullptr, nullptr));
    GCNHIP_CHECK(gcnhip_feat_scale_rows(env.ctx, feat, dinv_row));
    if (feat_agg) GCNHIP_CHECK(gcnhip_feat_scale_rows(env.ctx, feat_agg, dinv_row));
    if (feat_full) {                                           // every row of X on every rank: the global degrees are graph_l1's columns
        const float *dinv_all = nullptr;
        GCNHIP_CHECK(gcnhip_graph_scales(graph_l1, nullptr, nullptr, &dinv_all, nullptr));
        GCNHIP_CHECK(gcnhip_feat_scale_rows(env.ctx, feat_full, dinv_all));
    }
}

// one registered row subset of g per split code
void HipGCN::add_split_rowsets(gcnhip_ctx *ctx, gcnhip_graph *g, gcnhip_rowset *out[4]) {
    const int r0 = part.start[env.comm->rank()];
    for (int s = 1; s <= 3; s++) {
        std::vector<uint32_t> bits((size_t)n_local / 32 + 2, 0u);
        for (int r = 0; r < n_local; r++)
            if (data->split[r0 + r] == s) bits[r >> 5] |= 1u << (r & 31);
        GCNHIP_CHECK(gcnhip_graph_add_rowset(ctx, g, bits.data(), &out[s]));
    }
}

// The adjacency of this rank cut in two by the owner of the column: edges whose source row is one of this rank's own rows
// (complete as soon as the producer kernel has finished) and edges that need a row of another rank (complete when the
// exchange has finished).  Both halves keep the parent's coefficients and row order.  The same cut of the restricted
// operator of the output layer's backward, and the split subsets of the last aggregation on both halves.
void HipGCN::build_overlap() {
    const size_t n_pos = (size_t)xplan.table_rows;
    std::vector<uint32_t> own(n_pos / 32 + 2, 0u), other(n_pos / 32 + 2, 0u);
    for (size_t t = 0; t < n_pos; t++) {
        const bool mine = (int)t >= xplan.own_offset && (int)t < xplan.own_offset + n_local;
        (mine ? own : other)[t >> 5] |= 1u << (t & 31);
    }
    xlane.reset(new ExchangeLane(env.ctx, device_, env.comm, xplan, (int)xbuf.max_ld_words, timers->enabled));     // collective: every rank
    env.xlane = xlane.get();
    if (n_local == 0) return;             // no rows, no operators to cut: the modules see no split_loc and aggregate nothing
    GCNHIP_CHECK(gcnhip_graph_create_restricted(env.ctx, &graph_loc, graph, own.data()));
    GCNHIP_CHECK(gcnhip_graph_create_restricted(env.ctx, &graph_rem, graph, other.data()));
    if (graph_bwd_out) {
        GCNHIP_CHECK(gcnhip_graph_create_restricted(env.ctx, &graph_bwd_loc, graph_bwd_out, own.data()));
        GCNHIP_CHECK(gcnhip_graph_create_restricted(env.ctx, &graph_bwd_rem, graph_bwd_out, other.data()));
    }
    if (!(flags & HIPGCN_ALL_ROWS)) {
        add_split_rowsets(env.ctx, graph_loc, split_rows_loc);
        add_split_rowsets(env.ctx, graph_rem, split_rows_rem);
    }
}

// hand the halves of the cut operator to an aggregation (output_layer: also the halves of its restricted backward
// operator and the per-half subsets of the scored rows)
void HipGCN::wire_overlap(HipGraphSum *gs, bool output_layer) {
    if (!graph_loc) return;
    gs->split_loc = graph_loc; gs->split_rem = graph_rem;
    if (!output_layer) return;
    gs->bwd_split_loc = graph_bwd_loc; gs->bwd_split_rem = graph_bwd_rem;
    if (!(flags & HIPGCN_ALL_ROWS)) { gs->fwd_out_rows_loc = &scored.out_rows_loc; gs->fwd_out_rows_rem = &scored.out_rows_rem; }
}

// The loss module of one site (the modular list, the fused list, the evaluation lane).  Multi-label models take the sigmoid
// loss, the others the softmax loss; class weights, when the model has them, go to either.  Both are loss kernels on the stored
// logits, except the unweighted softmax loss, which rides in the epilogue of the launch that produces the logits (f32 tables, at
// most 64 classes; the paths that cut that launch in two — exchange overlap — or gather bf16 tables keep the loss kernel:
// HipGraphSum::forward decides).
Module *HipGCN::make_loss(const LossSite &s) {
    const int C = params.output_dim;
    if (opt_.multilabel) {
        auto *bce = new HipBCELoss(s.env, s.Z, d_ml_truth, ml_wpr, &s.split->count, s.d_result, s.d_result_i, C);
        bce->rows_list = &s.split->rows; bce->rows_n = &s.split->rows_n; bce->grad_row_scale = s.grad_row_scale;
        bce->d_pos_weight = d_class_w;
        return bce;
    }
    auto *ce = new HipCrossEntropyLoss(s.env, s.Z, &s.split->truth, &s.split->count, s.d_result, s.d_result_i, C, s.shift_in_place);
    if (s.list_rows) { ce->rows_list = &s.split->rows; ce->rows_n = &s.split->rows_n; }
    ce->grad_row_scale = s.grad_row_scale;
    ce->d_weight = d_class_w; ce->weight_sum = &s.split->wsum;
    if (s.epilogue && !d_class_w && opt_.loss_epilogue && C <= 64 && !s.env->bf16_tables) {
        const size_t n = (size_t)2 * std::max(n_local, 1);
        ce->row_terms = (s.env == &env ? arena : lane->arena).upload(std::vector<float>(n, 0.f).data(), n);   // on the site's context
        s.epilogue->loss = ce;
    }
    return ce;
}

void HipGCN::build_modules() {
    const int N = n_local, F = params.input_dim, H = params.hidden_dim, C = params.output_dim;
    const int rank = env.comm->rank();
    const uint64_t nnz_off = (uint64_t)data->feature_index.indptr[part.start[rank]];
    const uint64_t hid_off = (uint64_t)part.start[rank] * H;
    HipVariable *H0 = variables[1].get(), *W1 = variables[2].get(), *H1 = variables[3].get(),
                *Z0 = variables[4].get(), *W2 = variables[5].get(), *Z = variables[6].get();
    const float p = params.dropout;
    static const uint8_t *const no_mask = nullptr;
    if (flags & HIPGCN_MODULAR) {
        // the reference's list, one for one (gcn.cpp:23-59)
        modules.push_back(new HipDropout(&env, input, p, KEY_INPUT_DROPOUT, nnz_off, (flags & HIPGCN_HOST_MASKS) ? &env.keep_input : &no_mask));
        modules.push_back(new HipSparseMatmul(&env, &input_vals, W1, H0, feat, N, F, H, 0.f, nnz_off));
        { auto *gs = new HipGraphSum(&env, H0, H1, graph, H); wire_overlap(gs, false); modules.push_back(gs); }
        modules.push_back(new HipReLU(&env, H1));
        modules.push_back(new HipDropout(&env, H1, p, KEY_HIDDEN_DROPOUT, hid_off, (flags & HIPGCN_HOST_MASKS) ? &env.keep_hidden : &no_mask));
        modules.push_back(new HipMatmul(&env, H1, W2, Z0, N, H, C));
        { auto *gs = new HipGraphSum(&env, Z0, Z, graph, C); gs->bwd_row_bits = &bwd_bits; gs->bwd_graph = graph_bwd_out; gs->fwd_out_rows = &scored.out_rows; wire_overlap(gs, true); modules.push_back(gs); logits_gs = gs; }
        // the reference's loss visits every row; the losses beyond it (multi-label, class weights) take the split's row list
        modules.push_back(make_loss({&env, Z, &scored, d_result, d_result_i, true, nullptr,
                                     opt_.multilabel || d_class_w != nullptr, nullptr}));
    } else {
        const float scale = 1 / (1 - p);
        auto *sm = new HipSparseMatmul(&env, &input_vals, W1, H0, feat, N, F, H, p, nnz_off);
        auto *gs = new HipGraphSum(&env, H0, H1, graph, H, p, hid_off);
        auto *mm = new HipMatmul(&env, H1, W2, Z0, N, H, C, scale);
        if (replicate_l1) { sm->sp_full = feat_full; sm->vals_full = &full_vals; gs->fwd_graph_replicated = graph_l1; }
        wire_overlap(gs, false);
        if (factored_) {
            const float *dinv_row = nullptr, *dinv2_row = nullptr, *dinv2_col = nullptr;
            GCNHIP_CHECK(gcnhip_graph_scales(graph, &dinv_row, &dinv2_row, nullptr, &dinv2_col));
            gs->fwd_scaling = 2; gs->bwd_scaling = 3;          // H1' = dropout(relu(dinv^2 . sum)) ; dH0' = raw sum (dW1 = X'^T . dH0')
            mm->da_row_scale = dinv2_row;                      // dH1' = dinv^2 . mask . (T . W2^T)
            mm->da_row_scale_full = dinv2_col;                 // rows of the gathered table (several GPUs: dH1 rebuilt for all of them)
        }
        // single GPU: the ReLU/dropout mask of H1 leaves the aggregation's store epilogue as one bit per element and the
        // Matmul backward reads those instead of H1 (-119 MB per epoch at Reddit scale); HIPGCN_NO_MASK_BITS: re-read H1
        if (env.comm->size() == 1 && H % 32 == 0 && !env.bf16_tables && opt_.mask_bits) {
            const int wpr = H / 32;
            d_pos_bits = arena.upload(std::vector<uint32_t>((size_t)N * wpr, 0u).data(), (size_t)N * wpr);
            gs->mask_bits_out = d_pos_bits;
            mm->mask_bits = d_pos_bits; mm->mask_wpr = wpr;
        }
        if (rebuild_dh1) {
            const int wpr = (H + 31) / 32;
            d_pos_bits = arena.upload(std::vector<uint32_t>((size_t)xplan.table_rows * wpr, 0u).data(), (size_t)xplan.table_rows * wpr);
            gs->pos_bits_full = d_pos_bits; gs->wpr = wpr; gs->out_grad_complete = true;
            mm->pos_bits_full = d_pos_bits; mm->wpr = wpr; mm->all_rows = xplan.table_rows;
        }
        modules.push_back(sm);
        modules.push_back(gs);
        modules.push_back(mm);
        HipGraphSum *gs_logits = nullptr;
        {
            auto *gs = new HipGraphSum(&env, Z0, Z, graph, C);
            gs->bwd_row_bits = &bwd_bits; gs->bwd_graph = graph_bwd_out; gs->fwd_out_rows = &scored.out_rows;
            if (factored_) { gs->fwd_scaling = 1; gs->bwd_scaling = 3; }     // Z = dinv . sum(Z0') (the true logits); T = raw sum of dZ'
            wire_overlap(gs, true);
            modules.push_back(gs);
            gs_logits = gs;
            logits_gs = gs;
        }
        const float *dinv = nullptr;
        if (factored_) GCNHIP_CHECK(gcnhip_graph_scales(graph, &dinv, nullptr, nullptr, nullptr));   // dZ' = dinv . dZ
        modules.push_back(make_loss({&env, Z, &scored, d_result, d_result_i, false, dinv, true, gs_logits}));
    }
}

// This rank's rows of the adjacency with GLOBAL column ids (the degrees of all nodes are its column degrees), scratch
// reserved for the widest aggregation: what reads a replicated table, on either context, and what A^.X is built from.
gcnhip_graph *HipGCN::create_rows_graph(gcnhip_ctx *ctx) {
    const std::vector<int> &gp = data->graph.indptr, &gi = data->graph.indices;
    const int N = params.num_nodes, r0 = part.start[env.comm->rank()];
    std::vector<int> lp(n_local + 1), deg(N);
    for (int r = 0; r <= n_local; r++) lp[r] = gp[r0 + r] - gp[r0];
    for (int j = 0; j < N; j++) deg[j] = gp[j + 1] - gp[j];
    gcnhip_graph *g = nullptr;
    GCNHIP_CHECK(gcnhip_graph_create(ctx, &g, lp.data(), gi.data() + gp[r0], n_local, N, deg.data()));
    const int rc = gcnhip_graph_reserve_width(ctx, g, std::max(params.hidden_dim, params.output_dim));
    if (rc != 0) gcnhip_graph_destroy(ctx, g);
    GCNHIP_CHECK(rc);
    return g;
}

// A^.X for this rank's rows (needs every column of the adjacency and the matching rows of X: with several GPUs
// both are taken from the whole dataset once and released), then the evaluation module list that uses it.
void HipGCN::build_agg_first_eval() {
    const int world = env.comm->size();
    const int N = params.num_nodes, F = params.input_dim, H = params.hidden_dim;
    if (world == 1) {
        GCNHIP_CHECK(gcnhip_feat_create_aggregated(env.ctx, &feat_agg, graph, feat));
    } else {
        const std::vector<int> &fp = data->feature_index.indptr, &fi = data->feature_index.indices;
        gcnhip_graph *g_all = graph_l1;
        gcnhip_feat *x_all = feat_full;
        try {
            if (!g_all) g_all = create_rows_graph(env.ctx);
            if (!x_all)
                GCNHIP_CHECK(gcnhip_feat_create(env.ctx, &x_all, fp.data(), fi.empty() ? nullptr : fi.data(), data->feature_value.data(), N, F));
            GCNHIP_CHECK(gcnhip_feat_create_aggregated(env.ctx, &feat_agg, g_all, x_all));
        } catch (...) {
            if (g_all && g_all != graph_l1) gcnhip_graph_destroy(env.ctx, g_all);
            if (x_all && x_all != feat_full) gcnhip_feat_destroy(env.ctx, x_all);
            throw;
        }
        if (g_all != graph_l1) gcnhip_graph_destroy(env.ctx, g_all);
        if (x_all != feat_full) gcnhip_feat_destroy(env.ctx, x_all);
    }
    agg_vals = gcnhip_feat_values(feat_agg);
    // H1 = ReLU((A^.X).W1) written straight into variable 3; from there on the training modules' own forward(false)
    auto *sm = new HipSparseMatmul(&env, &agg_vals, variables[2].get(), variables[3].get(), feat_agg, n_local, F, H, 0.f, 0);
    sm->relu_out = true;
    // nothing but H1.W2 reads an evaluation's hidden matrix: both products in one launch, H1 not stored (get_var(3) rebuilds it)
    if (opt_.eval_fusion && !env.bf16_tables) sm->fuse_next = dynamic_cast<HipMatmul *>(modules[2]);
    eval_modules.push_back(sm);
    for (size_t i = 2; i < modules.size(); i++) eval_modules.push_back(modules[i]);
}

void HipGCN::build_eval_lane() {
    const int world = env.comm->size(), rank = env.comm->rank();
    const int N = n_local, F = params.input_dim, H = params.hidden_dim, C = params.output_dim;
    lane.reset(new EvalLane());
    EvalLane &L = *lane;
    HipSparseMatmul *lane_sm = nullptr;
    GCNHIP_CHECK(gcnhip_ctx_create(&L.env.ctx, /*device of the main context*/ device_, nullptr));
    L.arena.bind(L.env.ctx);
    GCNHIP_CHECK(gcnhip_ctx_set_corun(L.env.ctx, 1));           // the lane's kernels share the chip with the training pass
    if (slice_floats == 32 || slice_floats == 16) GCNHIP_CHECK(gcnhip_ctx_set_option(L.env.ctx, "gs_l", slice_floats / 4));   // as on the training context
    if (opt_.gemm >= 0) GCNHIP_CHECK(gcnhip_ctx_set_option(L.env.ctx, "gemm_bf16x3", opt_.gemm ? 2 : 0));
    L.timers.reset(new DeviceTimers(L.env.ctx));
    L.timers->enabled = timers->enabled;
    L.env.timers = L.timers.get();
    L.comm.reset(env.comm->clone_for(L.env.ctx));
    L.env.comm = L.comm.get();
    L.env.plan = &xplan;
    L.env.xbuf = &L.xbuf;
    if (world > 1) exchange_buffers_create(L.env.ctx, xplan, xbuf.max_ld_words, &L.xbuf);
    L.env.seed = env.seed;
    L.env.bf16_tables = env.bf16_tables;
    L.env.d_epoch = L.arena.alloc<uint32_t>(1);
    GCNHIP_CHECK(gcnhip_memset_async(L.env.ctx, L.env.d_epoch, 0xFF, sizeof(uint32_t)));
    L.d_result = L.arena.alloc<float>(4);
    L.d_result_i = L.arena.alloc<int32_t>(4);
    // same adjacency, own scratch for split rows: a device-side clone of the training lane's object, in the row schedule that
    // lane measured as fastest (round 4: rebuilding it from the host lists was 0.67 s of a 1.8 s model build at Reddit scale)
    GCNHIP_CHECK(gcnhip_graph_clone(L.env.ctx, &L.graph, graph));
    if (!(flags & HIPGCN_ALL_ROWS)) add_split_rowsets(L.env.ctx, L.graph, L.split_rows);
    const ExchangePlan *xp = world > 1 ? &xplan : nullptr;
    L.H0.reset(new HipVariable()); L.H1.reset(new HipVariable()); L.Z0.reset(new HipVariable()); L.Z.reset(new HipVariable());
    if (feat_agg) {
        // aggregate-first: the lane's hidden layer is one GEMM on A^.X — no H0, no hidden-width aggregation, no exchange
    } else if (replicate_l1) {
        L.graph_l1 = create_rows_graph(L.env.ctx);
        apply_schedule(L.env.ctx, L.graph_l1);
        L.H0->alloc_replicated(L.env.ctx, params.num_nodes, N, part.start[rank], H, false);
    } else {
        L.H0->alloc(L.env.ctx, N, H, false, true, false, xp);
    }
    L.H1->alloc(L.env.ctx, N, H, false);
    L.Z0->alloc(L.env.ctx, N, C, false, true, false, xp);
    L.Z->alloc(L.env.ctx, N, C, false);
    const uint64_t nnz_off = (uint64_t)data->feature_index.indptr[part.start[rank]];
    eval_vals = gcnhip_feat_values(feat);
    if (feat_agg) {
        auto *sm = new HipSparseMatmul(&L.env, &agg_vals, variables[2].get(), L.H1.get(), feat_agg, N, F, H, 0.f, 0);
        sm->relu_out = true;
        lane_sm = sm;
        L.modules.push_back(sm);
    } else {
        auto *sm = new HipSparseMatmul(&L.env, &eval_vals, variables[2].get(), L.H0.get(), feat, N, F, H, 0.f, nnz_off);
        auto *gs = new HipGraphSum(&L.env, L.H0.get(), L.H1.get(), L.graph, H, 0.f, 0);   // ReLU epilogue, no dropout in eval
        if (factored_) gs->fwd_scaling = 2;
        if (replicate_l1) { sm->sp_full = feat_full; sm->vals_full = &full_vals; gs->fwd_graph_replicated = L.graph_l1; }
        L.modules.push_back(sm);
        L.modules.push_back(gs);
    }
    {
        auto *mm = new HipMatmul(&L.env, L.H1.get(), variables[5].get(), L.Z0.get(), N, H, C);
        if (lane_sm && opt_.eval_fusion && !L.env.bf16_tables) lane_sm->fuse_next = mm;      // as on the training context
        L.modules.push_back(mm);
    }
    auto *gs_logits = new HipGraphSum(&L.env, L.Z0.get(), L.Z.get(), L.graph, C);
    gs_logits->fwd_out_rows = &L.scored.out_rows;
    if (factored_) gs_logits->fwd_scaling = 1;
    L.modules.push_back(gs_logits);
    L.modules.push_back(make_loss({&L.env, L.Z.get(), &L.scored, L.d_result, L.d_result_i, false, nullptr, true,
                                   gs_logits}));             // the loss epilogue as on the training context
    GCNHIP_CHECK(gcnhip_event_create_sync(&L.ev_weights));
    GCNHIP_CHECK(gcnhip_event_create_sync(&L.ev_done));
    GCNHIP_CHECK(gcnhip_event_create_sync(&L.ev_fork));
    GCNHIP_CHECK(gcnhip_ctx_sync(L.env.ctx));
}

// whatever of the lane exists (it may be half built when build_eval_lane threw)
void HipGCN::destroy_lane() {
    if (!lane) return;
    EvalLane &L = *lane;
    if (L.env.ctx) {
        gcnhip_ctx_sync(L.env.ctx);
        for (auto m : L.modules) delete m;
        L.modules.clear();
        L.H0.reset(); L.H1.reset(); L.Z0.reset(); L.Z.reset();
        if (L.graph) gcnhip_graph_destroy(L.env.ctx, L.graph);
        if (L.graph_l1) gcnhip_graph_destroy(L.env.ctx, L.graph_l1);
        L.arena.free_all();
        for (void *e : {L.ev_weights, L.ev_done, L.ev_fork})
            if (e) gcnhip_event_destroy(e);
        L.timers.reset();
        exchange_buffers_destroy(&L.xbuf);
        L.comm.reset();
        gcnhip_ctx_destroy(L.env.ctx);
    }
    lane.reset();
}

HipGCN::~HipGCN() { release(); }

void HipGCN::release() {
    if (!env.ctx) return;
    gcnhip_ctx_sync(env.ctx);
    destroy_lane();
    queries_.reset();                                         // the queries' scratch, before the adjacency object and the context
    if (!eval_modules.empty()) delete eval_modules[0];       // the rest are borrowed from `modules`
    eval_modules.clear();
    for (auto m : modules) delete m;
    modules.clear();
    // W1/W2 grads live in gradbuf (interior pointers: never freed through the variable)
    if (variables.size() == 7 && gradbuf) {
        if (variables[2]) variables[2]->grad = nullptr;
        if (variables[5]) variables[5]->grad = nullptr;
    }
    variables.clear();
    optimizer.reset();
    if (epoch_graph) { gcnhip_graph_exec_destroy(epoch_graph); epoch_graph = nullptr; }
    readback_destroy();
    env.xlane = nullptr;
    xlane.reset();                                            // its communicator goes before the parent's
    for (gcnhip_graph *g : {graph_loc, graph_rem, graph_bwd_loc, graph_bwd_rem, graph_bwd_out, graph, graph_l1})   // cuts before what they were cut from
        if (g) gcnhip_graph_destroy(env.ctx, g);
    for (gcnhip_feat *f : {feat, feat_full, feat_agg})
        if (f) gcnhip_feat_destroy(env.ctx, f);
    arena.free_all();                                         // every buffer the modules, variables and operators above borrowed
    timers.reset();
    exchange_buffers_destroy(&xbuf);
    owned_comm.reset();
    gcnhip_ctx_destroy(env.ctx);
    env.ctx = nullptr;
}
