// gcn_epochs.cpp — HipGCN's passes: training, evaluation and the validation lane, the captured replay, run_epochs, the
// pipelined read-back, run() and the timers.
#include "gcn.h"
#include <chrono>
#include <deque>
#include <cstdio>
#include "hip_check.h"

void HipGCN::sync() {
    if (xlane) GCNHIP_CHECK(gcnhip_ctx_sync(xlane->ctx));
    GCNHIP_CHECK(gcnhip_ctx_sync(env.ctx));
    if (lane) GCNHIP_CHECK(gcnhip_ctx_sync(lane->env.ctx));
}

double HipGCN::timer_total(timer_instance t, long *count) {
    long c0 = 0, c1 = 0, c2 = 0;
    double s = timers->total(t, &c0);
    if (lane) s += lane->timers->total(t, &c1);
    if (xlane) s += xlane->timers->total(t, &c2);             // exchanges on the exchange stream (TMR_COMM)
    if (count) *count = c0 + c1 + c2;
    return s;
}
void HipGCN::timers_reset() {
    timers->reset();
    if (lane) lane->timers->reset();
    if (xlane) xlane->timers->reset();
}

void HipGCN::set_timers(bool on) {
    sync();
    timers->enabled = on;
    if (lane) lane->timers->enabled = on;
    if (xlane) xlane->timers->enabled = on;
}

// split s of the per-split tables as the split being scored; `rows`: the split subsets of the adjacency object the pass
// aggregates through (the lane has its own; the halves of the cut operator exist on the training context only)
void HipGCN::fill_scored(ScoredSplit &d, int s, gcnhip_rowset *const *rows) const {
    const bool own = rows == split_rows;
    d.truth = d_truth[s];
    d.count = split_count[s];
    d.wsum = split_wsum[s];
    d.out_rows = rows[s];
    d.out_rows_loc = own ? split_rows_loc[s] : nullptr;
    d.out_rows_rem = own ? split_rows_rem[s] : nullptr;
    d.rows = d_split_list[s];
    d.rows_n = split_local_n[s];
}

void HipGCN::set_truth(int s) { fill_scored(scored, s, split_rows); }   // gcn.cpp:78-81: here a pointer switch

// set_input (gcn.cpp:73-76), modular mode only: device-to-device, never from the host
void HipGCN::refresh_input() {
    if (flags & HIPGCN_MODULAR)
        GCNHIP_CHECK(gcnhip_d2d_async(env.ctx, input->data, gcnhip_feat_values(feat), (size_t)gcnhip_feat_nnz(feat) * sizeof(float)));
}

// replay the reference's RNG consumption for one training epoch: nnzX draws for
// the input dropout, then N*h draws for the hidden one (module.cpp:207-221;
// order fixed by the module list, gcn.cpp:23,42).  Every rank walks the whole
// stream and keeps its slice, so the decisions do not depend on the partition.
void HipGCN::host_masks_for_epoch() {
    const int thr = (int)(params.dropout * MY_RAND_MAX);
    const int rank = env.comm->rank();
    const long nnz_total = data->feature_index.indptr[params.num_nodes];
    const long f0 = keep0_first;
    for (long i = 0; i < nnz_total; i++) {
        const bool keep = (int)rng.next() >= thr;
        if (i >= f0 && i < f0 + (long)h_keep0.size()) h_keep0[i - f0] = keep;
    }
    const long H = params.hidden_dim, h0 = (long)part.start[rank] * H, total = (long)params.num_nodes * H;
    for (long i = 0; i < total; i++) {
        const bool keep = (int)rng.next() >= thr;
        if (i >= h0 && i < h0 + (long)h_keep1.size()) h_keep1[i - h0] = keep;
    }
    GCNHIP_CHECK(gcnhip_h2d(env.ctx, d_keep0, h_keep0.data(), h_keep0.size()));
    GCNHIP_CHECK(gcnhip_h2d(env.ctx, d_keep1, h_keep1.data(), h_keep1.size()));
}

// A pass's metrics row (slot `slot` of the ring row *epoch_word names): loss/accuracy of its forward + the L2 term of the
// weights it used.  One GPU: the loss launch fills the row itself (gcnhip_metrics_record_with_next_loss, armed before the
// forward) — its result needs no all-reduce first.  HIPGCN_RECORD_LAUNCH (options.loss_records_metrics = false) keeps the
// separate launch (A/B); several GPUs always take it, after the all-reduce.
void HipGCN::metrics_before(HipEnv &e, int slot, const uint32_t *epoch_word) {
    if (e.comm->size() == 1 && opt_.loss_records_metrics)
        GCNHIP_CHECK(gcnhip_metrics_record_with_next_loss(e.ctx, d_ring, RING, slot, epoch_word, optimizer->d_sumsq));
}

// ... after the forward.  Several GPUs add up the n floats that END with the 4 of `result`: 4 for an evaluation, the whole
// gradient buffer (whose tail the result is) for a training pass — one all-reduce per epoch.
void HipGCN::metrics_after(HipEnv &e, DeviceTimers &t, int slot, const uint32_t *epoch_word, float *result, size_t n) {
    if (e.comm->size() > 1) {
        t.start(TMR_COMM);
        e.comm->allreduce_sum(result + 4 - n, n);
        t.stop(TMR_COMM);
    }
    if (!(e.comm->size() == 1 && opt_.loss_records_metrics))
        GCNHIP_CHECK(gcnhip_metrics_record(e.ctx, d_ring, RING, slot, epoch_word, result, nullptr, optimizer->d_sumsq));
}

void HipGCN::train_begin() {
    // (*env.d_epoch is this epoch's number already: the previous epoch's Adam launch advanced it)
    metrics_before(env, 0, env.d_epoch);
    epochs_done++;
    refresh_input();
    if (flags & HIPGCN_HOST_MASKS) host_masks_for_epoch();
    set_truth(1);
}

void HipGCN::train_end() {
    metrics_after(env, *timers, 0, env.d_epoch, d_result, gradbuf_elems);      // ... then the update
    if (lane && lane->pending) {                    // the previous validation pass still reads W1, W2 and the L2 term
        GCNHIP_CHECK(gcnhip_stream_wait_event(env.ctx, lane->ev_done));
        lane->pending = false;
    }
    optimizer->step();
    if (lane) GCNHIP_CHECK(gcnhip_event_record(env.ctx, lane->ev_weights));
}

void HipGCN::train_epoch_async() {              // gcn.cpp:107-118
    h1_from_fused_eval = false;                 // the training forward stores H1
    train_begin();
    for (auto m : modules) m->forward(true);
    for (int i = (int)modules.size() - 1; i >= 0; i--) modules[i]->backward();
    train_end();
}

// validation forward of the epoch that just finished, on the second stream
void HipGCN::lane_begin(int s) {
    EvalLane &L = *lane;
    GCNHIP_CHECK(gcnhip_stream_wait_event(L.env.ctx, L.ev_weights));
    // the lane's epoch word names the ring row: the epoch whose weights are evaluated, whatever was called in between
    const long want = epochs_done - 1;
    GCNHIP_CHECK(gcnhip_counter_add(L.env.ctx, L.env.d_epoch, (uint32_t)(want - L.epoch_word)));
    L.epoch_word = want;
    fill_scored(L.scored, s, L.split_rows);
    metrics_before(L.env, s == 2 ? 1 : 2, L.env.d_epoch);
}

void HipGCN::lane_end(int s) {
    EvalLane &L = *lane;
    metrics_after(L.env, *L.timers, s == 2 ? 1 : 2, L.env.d_epoch, L.d_result, 4);
    GCNHIP_CHECK(gcnhip_event_record(L.env.ctx, L.ev_done));
    L.pending = true;
}

void HipGCN::eval_on_lane(int s) {
    lane_begin(s);
    for (auto m : lane->modules) m->forward(false);
    lane_end(s);
}

// eval(e) on the lane and train(e+1) on the main stream, enqueued stage by stage in alternation.  Both need only
// the weights Adam(e) wrote.  The collectives of the two communicators execute in enqueue order (comm.cpp,
// turnstile), so enqueueing all of eval(e) first would make train(e+1)'s first all-gather wait for the whole
// validation pass; zipped, each collective waits only for the other lane's previous one, and the lanes' compute
// overlaps with each other's exchanges.
void HipGCN::eval_then_train_zipped(int s) {
    lane_begin(s);
    train_begin();
    const size_t nb = lane->modules.size(), na = modules.size();
    if (env.comm->size() == 1) {
        // One GPU: nothing to exchange, so the point of the second stream is to run kernels with different bottlenecks
        // side by side.  Both passes start with the same MFMA-bound GEMM; the validation pass is therefore released
        // only when the training GEMM has finished, and its GEMM then shares the chip with the gather-bound
        // hidden-width aggregation of the training pass.
        modules[0]->forward(true);
        GCNHIP_CHECK(gcnhip_event_record(env.ctx, lane->ev_fork));
        GCNHIP_CHECK(gcnhip_stream_wait_event(lane->env.ctx, lane->ev_fork));
        for (size_t i = 0; i < nb; i++) lane->modules[i]->forward(false);
        lane_end(s);
        for (size_t i = 1; i < na; i++) modules[i]->forward(true);
        for (int i = (int)na - 1; i >= 0; i--) modules[i]->backward();
        train_end();
        return;
    }
    for (size_t i = 0; i < std::max(na, nb); i++) {
        if (i < nb) lane->modules[i]->forward(false);
        if (i < na) modules[i]->forward(true);
    }
    lane_end(s);
    for (int i = (int)na - 1; i >= 0; i--) modules[i]->backward();
    train_end();
}

void HipGCN::eval_async(int s) {                // gcn.cpp:120-128
    refresh_input();
    set_truth(s);
    // (an evaluation on this stream scores the weights of the last update: the row of env.d_epoch_done, not of the epoch to come)
    metrics_before(env, s == 2 ? 1 : 2, env.d_epoch_done);
    for (auto m : eval_modules.empty() ? modules : eval_modules) m->forward(false);
    h1_from_fused_eval = !eval_modules.empty() && static_cast<HipSparseMatmul *>(eval_modules[0])->hidden_not_stored;
    metrics_after(env, *timers, s == 2 ? 1 : 2, env.d_epoch_done, d_result, 4);
}

std::pair<float, float> HipGCN::read_metrics(long epoch_index, int slot) {
    float row[8];
    if (lane) GCNHIP_CHECK(gcnhip_ctx_sync(lane->env.ctx));
    const uint32_t e = (uint32_t)epoch_index;   // epoch_index == -1 (eval before any training) wraps like the device word
    GCNHIP_CHECK(gcnhip_d2h(env.ctx, row, d_ring + ((size_t)(e % RING) * 4 + slot) * 8, sizeof row));
    return ring_metrics(row);
}

std::pair<float, float> HipGCN::ring_metrics(const float *row) const {
    const float l2 = params.weight_decay * row[4] / 2;                          // gcn.cpp:104
    if (opt_.multilabel)                                                        // {loss_sum, rows * C, 2 TP, 2 TP + FP + FN}
        return {row[0] / row[1] + l2, row[3] > 0.f ? row[2] / row[3] : 0.f};
    if (!opt_.class_weights.empty())                                            // {sum of w . term, sum of w, correct, total}: the weighted mean
        return {row[0] / row[1] + l2, (float)row[2] / (int)row[3]};
    const float loss = row[0] / (int)row[1];                                    // module.cpp:154
    const float acc = (float)row[2] / (int)row[3];                              // gcn.cpp:95
    return {loss + l2, acc};
}

std::pair<float, float> HipGCN::train_epoch() {
    train_epoch_async();
    return read_metrics(epochs_done - 1, 0);
}

std::pair<float, float> HipGCN::eval(int s) {
    eval_async(s);
    return read_metrics(epochs_done - 1, s == 2 ? 1 : 2);
}

// One epoch (train + validation) is a fixed launch sequence whose epoch-dependent inputs all live in device memory, so it
// is captured once into a hipGraph and replayed (single GPU, one stream, device RNG, no per-op timers).  The first epoch
// runs eagerly so every scratch buffer has its final size.
bool HipGCN::enqueue_epoch_replay() {
    const bool graph_ok = env.comm->size() == 1 && !lane && !timers->enabled && !(flags & (HIPGCN_HOST_MASKS | HIPGCN_NO_GRAPH));
    if (!(graph_ok && epochs_done >= 1 && optimizer->can_replay(1))) return false;
    if (!epoch_graph) {
        const long epochs_before = epochs_done;
        const int steps_before = optimizer->steps();
        GCNHIP_CHECK(gcnhip_capture_begin(env.ctx));
        try {
            train_epoch_async();
            eval_async(2);
        } catch (...) {
            // never leave the stream capturing: end the capture, drop whatever it recorded, restore
            // the host-side counters, then let the caller see the failure
            void *broken = nullptr;
            gcnhip_capture_end(env.ctx, &broken);
            if (broken) gcnhip_graph_exec_destroy(broken);
            epochs_done = epochs_before;
            optimizer->note_replayed(steps_before - optimizer->steps());
            throw;
        }
        GCNHIP_CHECK(gcnhip_capture_end(env.ctx, &epoch_graph));
        // the capture only recorded: undo its host-side bookkeeping, then run it for real
        epochs_done = epochs_before;
        optimizer->note_replayed(steps_before - optimizer->steps());
    }
    GCNHIP_CHECK(gcnhip_graph_launch(env.ctx, epoch_graph));
    epochs_done++;
    optimizer->note_replayed(1);
    return true;
}

// One epoch of the current schedule — its training pass and the validation of the weights it leaves — within a run of
// consecutive epochs that the caller enqueues before it waits for them (first / last: of that run).  With the validation
// lane the run is: the first training pass alone, then validation of epoch e zipped with training of epoch e+1, the last
// validation alone; so on return epoch e's validation is enqueued, and (unless last) so is epoch e+1's training pass.
// (One GPU with per-op timers on: one stream, so that every launch is timed alone — zipped() is then false.)
void HipGCN::enqueue_epoch(bool first, bool last) {
    if (zipped()) {
        if (first) train_epoch_async();
        if (last) eval_on_lane(2); else eval_then_train_zipped(2);
    } else if (!enqueue_epoch_replay()) {
        train_epoch_async();
        eval_async(2);
    }
}

void HipGCN::run_epochs(int n, float *trace) {
    int done = 0;
    while (done < n) {
        const int chunk = std::min(n - done, RING);
        const long first = epochs_done;
        for (int i = 0; i < chunk; i++) enqueue_epoch(i == 0, i == chunk - 1);
        sync();
        if (trace) {
            std::vector<float> ring((size_t)RING * 32);
            GCNHIP_CHECK(gcnhip_d2h(env.ctx, ring.data(), d_ring, ring.size() * sizeof(float)));
            for (int i = 0; i < chunk; i++) {
                const uint32_t e = (uint32_t)(first + i);
                for (int slot = 0; slot < 2; slot++) {
                    const float *row = &ring[((size_t)(e % RING) * 4 + slot) * 8];
                    const std::pair<float, float> m = ring_metrics(row);
                    trace[(size_t)(done + i) * 4 + slot * 2] = m.first;
                    trace[(size_t)(done + i) * 4 + slot * 2 + 1] = m.second;
                }
            }
        }
        done += chunk;
    }
}

void HipGCN::readback_create(bool own_stream) {
    if (readback && (readback->ctx != nullptr) != own_stream) readback_destroy();
    if (readback) return;
    readback.reset(new Readback());
    Readback &R = *readback;
    if (own_stream) GCNHIP_CHECK(gcnhip_ctx_create(&R.ctx, device_, nullptr));
    GCNHIP_CHECK(gcnhip_host_alloc((void **)&R.host, (size_t)PIPELINE_DEPTH * READBACK_GROUP_MAX * 32 * sizeof(float)));
    for (int k = 0; k < PIPELINE_DEPTH; k++) {
        if (own_stream) GCNHIP_CHECK(gcnhip_event_create_sync(&R.ev_ready[k]));
        GCNHIP_CHECK(gcnhip_event_create_sync(&R.ev_copied[k]));
    }
}

void HipGCN::readback_destroy() {
    if (!readback) return;
    Readback &R = *readback;
    if (R.ctx) gcnhip_ctx_sync(R.ctx);
    for (int k = 0; k < PIPELINE_DEPTH; k++) {
        if (R.ev_ready[k]) gcnhip_event_destroy(R.ev_ready[k]);
        if (R.ev_copied[k]) gcnhip_event_destroy(R.ev_copied[k]);
    }
    gcnhip_host_free(R.host);
    if (R.ctx) gcnhip_ctx_destroy(R.ctx);
    readback.reset();
}

// everything of epochs e .. e+n-1 (0-based) has been enqueued, the last validation pass on `producer`: behind it, their
// ring rows (32 floats each; slots 0 = train and 1 = validation are read) are copied to slot k of the pinned buffer.  The
// ring wraps at RING rows: at most two copies.  The copy goes on `producer` itself.  With a stream of its own for the
// read-back (round 4's first version) the copy leaves the producer's timeline, but a barrier packet then sits on a second
// hardware queue for as long as the group runs, and the producer's own launches slow down beside it: gcn-hip per epoch,
// own stream -> producer's stream: Cora 102 -> 81 us (captured epoch replayed), Pubmed 124 -> 114 us and Reddit
// 3329 -> 3291 us (validation lane); profiles/r04_cli_run_loop.json, DESIGN.md §4.10.
void HipGCN::readback_enqueue(long e, int n, int k, gcnhip_ctx *producer) {
    Readback &R = *readback;
    gcnhip_ctx *on = producer;
    if (R.ctx) {
        GCNHIP_CHECK(gcnhip_event_record(producer, R.ev_ready[k]));
        GCNHIP_CHECK(gcnhip_stream_wait_event(R.ctx, R.ev_ready[k]));
        on = R.ctx;
    }
    float *dst = R.host + (size_t)k * READBACK_GROUP_MAX * 32;
    const int r0 = (int)((uint32_t)e % RING), n1 = std::min(n, RING - r0);
    GCNHIP_CHECK(gcnhip_d2h_async(on, dst, d_ring + (size_t)r0 * 32, (size_t)n1 * 32 * sizeof(float)));
    if (n > n1) GCNHIP_CHECK(gcnhip_d2h_async(on, dst + (size_t)n1 * 32, d_ring, (size_t)(n - n1) * 32 * sizeof(float)));
    GCNHIP_CHECK(gcnhip_event_record(on, R.ev_copied[k]));
}

void HipGCN::run() {                            // gcn.cpp:130-158
    if (params.early_stopping > 0 || (flags & HIPGCN_SYNC_EPOCHS) || params.epochs < 1) run_synchronous();
    else run_pipelined();
    report_test();
}

// No printed number feeds back into the run (no early stopping): epochs are enqueued ahead of the line being printed, and
// their metrics come back in GROUPS of consecutive epochs — one event wait and one small copy per group, up to
// PIPELINE_DEPTH groups in flight.  The first READBACK_CALIBRATION epochs go one per group; their steady completion rate
// then sets the group size so that a group spans about READBACK_GROUP_SECONDS (1 on Reddit-size graphs, where an epoch is
// milliseconds; 16 on Cora / Pubmed, whose ~100 us epochs would otherwise spend as long on the host's per-epoch event and
// copy calls as on the device).  Lines of a group are printed together, each with time= the group's interval / its size.
// With the validation lane, eval(e) is zipped with train(e+1) exactly as in run_epochs (enqueue_epoch).
void HipGCN::run_pipelined() {
    // the read-back copies ride on the producer's stream; HIPGCN_READBACK_STREAM=1 gives them their own (measured
    // slower at every size, see readback_enqueue; kept so that the measurement can be repeated)
    readback_create(opt_.readback_stream);
    Readback &R = *readback;
    const bool talk = env.comm->rank() == 0;
    const long E = params.epochs, first = epochs_done;
    long evald = 0, grouped = 0, printed = 0;            // epochs (of this run) with: validation pass enqueued / a read-back
                                                         // enqueued / their line out
    struct Group { long e0; int n, slot; };
    std::deque<Group> inflight;
    long n_groups = 0;
    int group = 1;                                       // epochs per read-back group
    bool group_settled = false;                          // pinned by HIPGCN_READBACK_GROUP, or set after the calibration epochs
    if (opt_.readback_group > 0) {
        group = std::max(1, std::min(opt_.readback_group, (int)READBACK_GROUP_MAX));
        group_settled = true;
    }
    double total_train = 0, calib = 0;
    auto t_prev = std::chrono::high_resolution_clock::now();
    const bool verbose = opt_.verbose;
    double host_enqueue_s = 0, host_wait_s = 0;
    while (printed < E) {
        const auto t_enq0 = std::chrono::high_resolution_clock::now();
        while ((int)inflight.size() < PIPELINE_DEPTH && grouped < E) {
            const int n = (int)std::min<long>(group, E - grouped);
            for (; evald < grouped + n; evald++) enqueue_epoch(evald == 0, evald == E - 1);
            const int slot = (int)(n_groups++ % PIPELINE_DEPTH);
            readback_enqueue(first + grouped, n, slot, zipped() ? lane->env.ctx : env.ctx);
            inflight.push_back({grouped, n, slot});
            grouped += n;
        }
        const Group g = inflight.front();
        inflight.pop_front();
        const auto t_wait0 = std::chrono::high_resolution_clock::now();
        GCNHIP_CHECK(gcnhip_event_sync(R.ev_copied[g.slot]));
        const auto t_now = std::chrono::high_resolution_clock::now();
        host_enqueue_s += std::chrono::duration<double>(t_wait0 - t_enq0).count();
        host_wait_s += std::chrono::duration<double>(t_now - t_wait0).count();
        const double dt_group = std::chrono::duration_cast<std::chrono::duration<double>>(t_now - t_prev).count();
        t_prev = t_now;
        total_train += dt_group;
        const float dt = (float)(dt_group / g.n);
        for (int i = 0; i < g.n; i++) {
            const float *tr = R.host + ((size_t)g.slot * READBACK_GROUP_MAX + i) * 32, *va = tr + 8;
            print_line(g.e0 + i + 1, ring_metrics(tr), ring_metrics(va), dt);
        }
        printed += g.n;
        if (!group_settled && printed > READBACK_CALIBRATION / 2 && printed <= READBACK_CALIBRATION) calib += dt_group;
        if (!group_settled && printed == READBACK_CALIBRATION) {      // (groups of one until here: printed counts epochs one by one)
            const double per_epoch = calib / (READBACK_CALIBRATION / 2);
            const int want = per_epoch > 0 ? (int)(READBACK_GROUP_SECONDS / per_epoch) : 1;
            group = 1;
            while (group * 2 <= want && group * 2 <= READBACK_GROUP_MAX) group *= 2;
            group_settled = true;
            if (verbose && talk) fprintf(stderr, "[hipgcn] read-back groups of %d epochs (%.1f us per epoch while calibrating)\n", group, 1e6 * per_epoch);
        }
    }
    sync();
    if (talk) printf("total training time=%.5f\n", (float)total_train);
    if (verbose && talk)
        fprintf(stderr, "[hipgcn] run loop: %.1f us per epoch enqueueing, %.1f us per epoch waiting for read-backs\n", 1e6 * host_enqueue_s / E, 1e6 * host_wait_s / E);
}

void HipGCN::run_synchronous() {
    int epoch = 1;
    std::vector<float> loss_history;
    double total_train = 0;
    const bool talk = env.comm->rank() == 0;
    for (; epoch <= params.epochs; epoch++) {
        auto t0 = std::chrono::high_resolution_clock::now();
        train_epoch_async();
        if (lane) eval_on_lane(2); else eval_async(2);
        const std::pair<float, float> train = read_metrics(epochs_done - 1, 0);     // one synchronisation per epoch
        const std::pair<float, float> val = read_metrics(epochs_done - 1, 1);
        const float dt = std::chrono::duration_cast<std::chrono::duration<float>>(std::chrono::high_resolution_clock::now() - t0).count();
        total_train += dt;
        print_line(epoch, train, val, dt);
        loss_history.push_back(val.first);
        if (params.early_stopping > 0 && epoch >= params.early_stopping) {
            float recent_loss = 0.0;
            for (int i = epoch - params.early_stopping; i < epoch; i++) recent_loss += loss_history[i];
            if (val.first > recent_loss / params.early_stopping) {
                if (talk) printf("Early stopping...\n");
                break;
            }
        }
    }
    if (talk) printf("total training time=%.5f\n", (float)total_train);
}

void HipGCN::report_test() {
    auto t0 = std::chrono::high_resolution_clock::now();
    const std::pair<float, float> test = eval(3);
    const float dt = std::chrono::duration_cast<std::chrono::duration<float>>(std::chrono::high_resolution_clock::now() - t0).count();
    print_line(0, {}, test, dt);
}

// the reference's output lines (gcn.cpp:137-157), rank 0 only: epoch >= 1 the epoch's line (train, then validation), 0 the
// test line (`train` unused); a multi-label model names its second column f1
void HipGCN::print_line(long epoch, std::pair<float, float> train, std::pair<float, float> scored_now, float dt) const {
    if (env.comm->rank() != 0) return;
    const char *m = opt_.multilabel ? "f1" : "acc";
    if (epoch)
        printf("epoch=%ld train_loss=%.5f train_%s=%.5f val_loss=%.5f val_%s=%.5f time=%.5f\n", epoch, train.first, m, train.second,
               scored_now.first, m, scored_now.second, dt);
    else
        printf("test_loss=%.5f test_%s=%.5f time=%.5f\n", scored_now.first, m, scored_now.second, dt);
}
