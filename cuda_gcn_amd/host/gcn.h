// gcn.h — the model driver.  GCNParams / GCNData are the reference's types
// (src/seq/gcn.h:9-22); HipGCN has the shape of GCN / CUDAGCN
// (src/seq/gcn.h:24-44, src/cuda/cuda_gcn.cuh:11-34): constructed from
// (GCNParams, GCNData*), driven by run().  Everything between the two lives on
// the GPU; per epoch the host reads back 2 x 8 floats.
#pragma once
#include <memory>
#include <utility>
#include <vector>
#include "comm.h"
#include "device_arena.h"
#include "module.h"
#include "optim.h"
#include "partition.h"
#include "sparse.h"
#include "timer.h"
#include "variable.h"

struct GCNParams {
    int num_nodes, input_dim, hidden_dim, output_dim;
    float dropout, learning_rate, weight_decay;
    int epochs, early_stopping;
    static GCNParams get_default();          // {2708,1433,16,7, 0.5, 0.01, 5e-4, 100, 0} (gcn.cpp:9-11)
};

class GCNData {
public:
    SparseIndex feature_index, graph;
    std::vector<int> split;
    std::vector<int> label;
    std::vector<float> feature_value;
    // multi-label truth (beyond the reference): num_nodes rows of ceil(output_dim / 32) words, bit (c & 31) of word c >> 5 =
    // class c (host/labels.h).  Read by HipGCN only when HipGCNOptions::multilabel is set; `label` is then unused for the loss.
    std::vector<uint32_t> multihot;
};

enum HipGCNFlags {
    HIPGCN_MODULAR = 1,       // one module per reference module instead of the fused epilogues
    HIPGCN_HOST_MASKS = 2,    // parity mode: dropout decisions from the reference's host RNG stream
    HIPGCN_TIMERS = 4,        // record device-event timers per op
    HIPGCN_NO_GRAPH = 8,      // never replay epochs from a captured hipGraph
    HIPGCN_EVAL_LANE = 16,    // validation forward on a second stream, overlapped with the next training epoch (opt-in; with
                              // several GPUs it adds a second communicator: not the default until measured on such a node)
    HIPGCN_NO_EVAL_LANE = 32, // never
    HIPGCN_NO_REPLICATE_L1 = 64, // multi-GPU: all-gather H0 instead of computing X.W1 for all rows on every rank
    HIPGCN_REPLICATE_L1 = 128,   // ... or force the replication (default: 2-4 GPUs replicate, 8 gather)
    HIPGCN_GATHER_DH1 = 256,     // multi-GPU: all-gather dH1 (128 wide) instead of dZ0 (48 wide) + 1 bit per element of H1
    HIPGCN_BF16_TABLES = 2048,   // opt-in, beyond the reference: GraphSum gathers bfloat16 copies of its inputs (f32 accumulate)
    HIPGCN_ALL_ROWS = 4096,      // compute every row of the logits (default: only rows of the scored split, which is all the loss and accuracy read)
    HIPGCN_NO_AGG_FIRST_EVAL = 8192, // evaluation forwards keep the reference's order A^.(X.W1) instead of (A^.X).W1 with A^.X built once
    HIPGCN_EXCHANGE_ALLGATHER = 16384, // multi-GPU: always all-gather whole row blocks before an aggregation
    HIPGCN_EXCHANGE_HALO = 32768,      // ... or always exchange only the rows some local edge points at (default: decided per graph)
    HIPGCN_NO_LABEL_HINT = 524288,     // never use the dataset's labels as row groups of the aggregation's schedule (groups are then
                                       // looked for in the graph itself, cluster.h)
    HIPGCN_MASKED_BWD = 131072,        // the output layer's backward masks the known-zero rows of dZ at every launch instead of
                                       // aggregating through an operator that has lost the edges pointing at them
    // 65536 and 262144 are retired (measured-slower variants, removed): not to be reused; a caller that sets them gets the default path
    HIPGCN_NULL_COMM = 1024,     // world > 1 without transport: collectives are no-ops (per-rank compute timing only)
    HIPGCN_NO_ROW_GROUPS = 512,  // keep the aggregation's plain descending-degree row schedule (no timing of alternatives)
    HIPGCN_OVERLAP_EXCHANGE = 1048576,  // multi-GPU: exchanges on their own stream; each aggregation starts on the edges that point at
                                        // this rank's own rows while the other ranks' rows arrive, then adds the rest (the order of a
                                        // row's sum then depends on the partition: float tolerance, not bit-identity, across P)
    HIPGCN_STRUCTURE_PARTITION = 2097152, // multi-GPU: rank blocks formed from groups found in the graph (cluster.h) instead of
                                          // contiguous id ranges, when that shrinks the neediest rank's halo (default: decided per graph)
    HIPGCN_ID_PARTITION = 4194304,        // ... never
    HIPGCN_EDGE_COEF = 16777216,          // aggregate with the reference's per-edge coefficients 1/sqrt(deg deg) (module.cpp:91-93) instead of
                                          // the factored form dinv[r] * sum(dinv[c] * x[c]) (default on the fused f32 path: no coefficient
                                          // stream beside the indices, -6..10 % per aggregation; same real numbers, two more roundings per term)
    HIPGCN_SYNC_EPOCHS = 8388608,         // run(): wait for every epoch before the next is enqueued (the reference's loop, gcn.cpp:133-151:
                                          // `time=` is then that epoch's own latency).  Default: epochs are enqueued ahead of the line being
                                          // printed whenever no decision depends on a printed number (early_stopping == 0)
};

struct HipGCNOptions {
    int device = 0;
    long seed = 0;            // plays time(NULL) of src/seq/rand.cpp:7
    int flags = 0;
    Comm *comm = nullptr;     // NULL: single GPU.  Not owned unless own_comm.
    bool own_comm = false;
    // multi-GPU: RCCL unique id (GCN_NCCL_ID_BYTES) and rank/world when comm == NULL and world > 1
    int rank = 0, world = 1;
    const char *nccl_id = nullptr;
    // or a host-staged transport (tests: torch.distributed gloo through callbacks)
    gcn_host_allgather_fn host_allgather = nullptr;
    gcn_host_allreduce_fn host_allreduce = nullptr;
    void *host_user = nullptr;

    // ---- switches that have no flag bit.  HipGCN itself never reads the environment: the two places that build a model
    // from outside (main.cpp, capi.cpp) call from_environment() ONCE and hand the result in.
    bool verbose = false;                 // HIPGCN_VERBOSE: where the model build's wall time goes, run-loop statistics (stderr)
    int exchange = -1;                    // HIPGCN_EXCHANGE: -1 unset, 0 auto (per graph), 1 allgather, 2 halo
    bool structure_groups = true;         // HIPGCN_NO_STRUCTURE_GROUPS clears: never search the graph for row groups
    bool eval_fusion = true;              // HIPGCN_NO_EVAL_FUSION clears: evaluation forwards store the hidden matrix and run H1.W2 as its own launch
    bool loss_epilogue = true;            // HIPGCN_NO_LOSS_EPILOGUE clears: the loss kernel reads the stored logits (round 4) instead of riding in the class-width aggregation's epilogue
    bool mask_bits = true;                // HIPGCN_NO_MASK_BITS clears: the Matmul backward re-reads H1 instead of one bit per element
    bool loss_records_metrics = true;     // HIPGCN_RECORD_LAUNCH clears: the metrics row gets a launch of its own (A/B)
    bool readback_stream = false;         // HIPGCN_READBACK_STREAM: run()'s read-back copies on a stream of their own (measured slower)
    int readback_group = 0;               // HIPGCN_READBACK_GROUP: epochs per read-back group (0: calibrated)
    // HIPGCN_SCHEDULE=degree|label|dealt[-G]|structure: pin the aggregation's row schedule instead of timing the candidates at
    // load (-1: timed).  A pinned run launches no tuning kernels, so a kernel-trace profile of it holds the epochs' launches only.
    int schedule = -1, schedule_groups = 256;
    bool slice_tuning = true;             // HIPGCN_NO_SLICE_TUNING clears: the hidden-width aggregation keeps 64-float column slices
                                          // (default: chosen per graph by a rule on its structure, HipGCN::choose_slice_width)
    // HIPGCN_GEMM=f32|bf16x3: arithmetic of the dense first-layer products (0: exact-f32 MFMA, 1: three-plane bf16 split on the
    // bf16 MFMA pipe, same f32 error bound; -1: the library's default)
    int gemm = -1;
    // Multi-label mode (beyond the reference; chosen here, never from the environment): the truth is GCNData::multihot, the loss
    // the per-class sigmoid cross-entropy on the stored logits (gcnhip_bce_fwd_rows), and the accuracy column of every metric
    // micro-F1.  1 <= output_dim <= 256.
    bool multilabel = false;
    // Class weights of the loss (beyond the reference; chosen here, never from the environment; host/class_weights.h).  Empty: off,
    // every path is the unweighted one.  Single-label: w[output_dim], the loss is the weighted mean sum(w . term) / sum(w) of
    // gcnhip_wxent_fwd_rows (accuracy is not weighted).  Multi-label: pos_weight[output_dim] on the positive term
    // (gcnhip_wbce_fwd_rows).  The loss then always runs on the stored logits (no loss epilogue).  Refused: a wrong length, a
    // negative / NaN / infinite weight, more than 256 classes, a scored split whose weights sum to 0 (single-label).
    std::vector<float> class_weights;

    // `base` with every HIPGCN_* variable of the process environment applied (flag variables OR their bit in)
    static HipGCNOptions from_environment(HipGCNOptions base);
};

// Which split a pass scores: what set_truth (gcn.cpp:78-81) switches, as one value.  The loss module and the class-width
// aggregation hold pointers to the fields; the training context has one, the validation lane its own.
struct ScoredSplit {
    int32_t *truth = nullptr;                                  // d_truth of the split
    int count = 0;                                             // its labelled rows, all ranks
    float wsum = 0.f;                                          // single-label class weights: sum of w[label] over it, all ranks
    gcnhip_rowset *out_rows = nullptr;                         // its rows of the adjacency (all the loss reads); NULL with HIPGCN_ALL_ROWS
    gcnhip_rowset *out_rows_loc = nullptr, *out_rows_rem = nullptr;   // HIPGCN_OVERLAP_EXCHANGE: the same on the two halves of the cut
    int32_t *rows = nullptr; int rows_n = 0;                   // its local row ids, ascending (the loss walks only these)
};

class HipGCN {
public:
    GCNParams params;
    HipGCN(GCNParams params, GCNData *data, const HipGCNOptions &opt = HipGCNOptions());
    ~HipGCN();
    HipGCN(const HipGCN &) = delete;

    // gcn.cpp:130-158, same output lines.  With early stopping (or HIPGCN_SYNC_EPOCHS) the loop is the reference's: enqueue
    // one epoch, wait, print, decide.  Otherwise nothing the host prints feeds back into the run, so epochs are enqueued
    // ahead of the line being printed and their metrics are copied back behind them in groups of consecutive epochs
    // (1 when an epoch takes milliseconds, up to READBACK_GROUP_MAX when it takes tens of microseconds; run_pipelined):
    // `time=` is then the interval between consecutive group completions / the group's size and `total training time`
    // their sum = the wall time of the whole loop.
    void run();
    std::pair<float, float> train_epoch();                    // synchronises to return (loss, acc)
    std::pair<float, float> eval(int current_split);
    // enqueue n x (train_epoch + eval(2)) with no host synchronisation in between, then read back
    // 4 floats per epoch into trace (may be NULL)
    void run_epochs(int n, float *trace);
    void sync();

    // introspection for tests / bench
    int rank() const { return env.comm->rank(); }
    int schedule_mode() const { return sched_mode; }
    int schedule_groups() const { return sched_groups; }
    int schedule_slice_floats() const { return slice_floats; }  // column-slice width the hidden-width aggregation was tuned to (64 or 32)
    int world() const { return env.comm->size(); }
    const char *transport() const { return env.comm->transport(); }
    int transport_ranks() const { return env.comm->transport_ranks(); }
    int local_rows() const { return n_local; }
    int row_start() const { return part.start[env.comm->rank()]; }
    const RowPartition &partition() const { return part; }
    // multi-GPU: the model may renumber the nodes before it partitions them (partition.h, choose_node_order): row r of
    // this rank is then node node_order()[row_start() + r] of the dataset it was given.  Empty: the ids were kept.
    const std::vector<int> &node_order() const { return node_order_; }
    const char *node_order_name() const { return node_order_name_; }
    const ExchangePlan &exchange_plan() const { return xplan; }
    // variable k as in gcn.cpp:21-54 (1 H0, 2 W1, 3 H1, 4 Z0, 5 W2, 6 Z); rows x cols floats, this rank's rows.
    // FACTORED FORM (default on the fused f32 path; factored() tells, HIPGCN_EDGE_COEF restores the reference's values): the
    // matrices an aggregation gathers from are stored pre-multiplied by dinv = 1/sqrt(deg) of their row, so get_var returns
    // dinv.H0 (1), dinv.H1 (3), dinv.Z0 (4) and, as gradients, dinv.dZ (6), dinv.dH1 (3), dZ0/dinv (4), dH0/dinv (1); the
    // logits Z (6), the weights and their gradients are the reference's own.  row_scale() returns dinv for this rank's rows.
    // PARTIAL-ROW CONTRACT of variable 6 (and 4 on an evaluation forward): by default the last aggregation of a forward
    // computes only the rows of the split being scored — all the loss and the accuracy read (module.cpp:131-133,
    // gcn.cpp:86-88) — so after train_epoch() only rows of the training split hold this epoch's logits, after eval(s)
    // only rows of split s; the other rows keep whatever an earlier forward left (or the zeros of the allocation).  The
    // reference fills every row on every forward: construct with HIPGCN_ALL_ROWS to get that.
    void get_var(int k, bool grad, std::vector<float> &out, int *rows, int *cols);
    bool factored() const { return factored_; }
    void row_scale(std::vector<float> &dinv);                 // 1/sqrt(deg) of this rank's rows (deg of the full graph, self loop included)
    void set_weights(const float *w1, const float *w2);       // [F x h], [h x C] row-major

    // Prediction (beyond the reference, which only prints accuracy): an evaluation forward with the current weights — no
    // dropout, the model's usual evaluation order (aggregate-first when that is on) — whose logit aggregation carries the
    // prediction epilogue (gcnhip_graphsum_predict) on the requested rows.  nodes: n DATASET node ids, each a row of this
    // rank (repeats allowed); NULL: every row of this rank, in the order of local rows (node_order()/row_start() name
    // them).  pred[i] = argmax of node i's logits (lowest class on a tie), prob[i] = its softmax probability, logp
    // (may be NULL) [n x C] = the log-softmax rows.  Several GPUs: a collective (the logit aggregation's exchange) —
    // every rank calls it, each with its own nodes.  Training state is not touched: the metrics ring, the current split,
    // the logits (variable 6) and the captured epoch graph are left as they were; a train_epoch() after it has the
    // same bits as one without it.  Synchronises.
    void predict(const int *nodes, int n, int32_t *pred, float *prob, float *logp);
    // Multi-label prediction, the same contract as predict() (dataset ids, NULL = every row of this rank, a collective, training
    // state untouched, synchronises): one evaluation forward whose logits go to scratch (not variable 6), then
    // gcnhip_bce_predict_rows.  bits [n x ceil(C / 32)]: bit (c & 31) of word c >> 5 = (z_c > 0); prob (may be NULL) [n x C] =
    // sigmoid(z).  Only on a multi-label model (predict() only on a single-label one).
    void predict_multilabel(const int *nodes, int n, uint32_t *bits, float *prob);
    bool multilabel() const { return opt_.multilabel; }
    bool weighted() const { return !opt_.class_weights.empty(); }
    // Per-class evaluation (beyond the reference): one evaluation forward with the current weights (no dropout) over a set of
    // rows, and integer counts per class formed on the GPU behind it.  Rows: the nodes of `split` (1 train, 2 validation,
    // 3 test — eval's codes) on this rank, `nodes` then ignored; or, with split == 0, the `nodes` query with predict()'s
    // conventions (n dataset ids, each a row of this rank, repeats counted as often as listed; NULL: every row of this rank).
    // Single-label model: the logit aggregation runs gcnhip_graphsum_predict on those rows only, then gcnhip_confusion_rows;
    // counts [C x C], counts[t * C + p] = rows with truth t predicted as p; *unlabelled = rows whose truth is outside [0, C)
    // (not in the matrix), *rows_counted = rows in the matrix.  Multi-label model: predict_multilabel's forward (logits to
    // scratch), then gcnhip_bce_class_counts_rows; counts [3 x C] = TP, FP, FN per class (z > 0 predicts the class),
    // *rows_counted = the rows, *unlabelled = 0.  Several GPUs: a collective like predict(); each rank counts its own rows, the
    // counts are summed exactly over the ranks and every rank returns the same totals.  Only the counts cross to the host.
    // Training state is not touched: the metrics ring, the current split, the logits (variable 6) and the captured epoch
    // graph are left as they were; a train_epoch() after it has the same bits as one without it.  Synchronises.  More than
    // 64 (single-label) or 256 (multi-label) classes: an error.  host/report.h derives precision / recall / F1 from the counts.
    void evaluate(int split, const int *nodes, int n, int64_t *counts, int64_t *rows_counted, int64_t *unlabelled);
    // Label propagation and Correct & Smooth (beyond the reference; Huang et al., 2020): the graph and the known labels used
    // at inference time.  Every iteration is one gcnhip_graphsum_blend launch through `graph` with its per-edge coefficients,
    // ping-ponging two of four [local rows x ld] f32 tables from the arena (allocated on first use; ld by the row rule of
    // variable 6).  Arrays are in DATASET node order.  predict()'s contract: the call starts with sync(); the metrics ring, the
    // current split, variable 6 and the captured epoch graph are untouched.  Refused with a message before any launch: more
    // than one rank (every iteration would need a table exchange), alpha outside [0, 1], iters < 0, a width outside 1..64, and
    // for the two label schemes a multi-label model or more than 64 classes.  splits_mask: bit s = the labelled nodes of split
    // s are known (2 = the training split).
    //   propagate: Y_{k+1} = clamp(alpha . A^ . Y_k + (1 - alpha) . y0, lo, hi), Y_0 = y0 [num_nodes x dim]; out = Y_iters, pred
    //   (may be NULL) its row argmax (lowest column on a tie).  Needs neither labels nor trained weights.
    //   label_propagation: propagate from the one-hot rows of the known nodes (zero rows elsewhere), clamp [0, 1].
    //   correct_and_smooth: one hooked evaluation forward leaves the log-softmax rows on the device; gcnhip_cs_error_rows,
    //   iters_correct blends clamped to [-1, 1], gcnhip_cs_correct_rows, iters_smooth blends clamped to [0, 1], the last of which
    //   writes pred — the only array that must cross to the host; g (may be NULL) is copied when asked for.
    void propagate(const float *y0, int dim, float alpha, int iters, float lo, float hi, float *out, int32_t *pred);
    void label_propagation(float alpha, int iters, int splits_mask, int32_t *pred, float *y);
    void correct_and_smooth(float alpha_correct, int iters_correct, float alpha_smooth, int iters_smooth, int splits_mask, int32_t *pred, float *g);
    // Temperature scaling and calibration error (beyond the reference; Guo et al., 2017): are predict()'s probabilities to be
    // trusted, and one scalar T that repairs them — softmax(z / T) with T fitted on a held-out split.  All three work on the
    // log-softmax rows predict()'s hooked forward leaves on the device (log_softmax(z / T) = log_softmax(log_softmax(z) / T)) with
    // the row-local kernels of csrc/calib.hip, and hold predict()'s contract: the call starts with sync(); the metrics ring, the
    // current split, variable 6 and the captured epoch graph are untouched.  Rows: the labelled nodes of `split` (1 train,
    // 2 validation, 3 test), or with split == 0 the `nodes` query scored against the dataset's labels, as evaluate() takes them.
    // Refused with a message before any launch: a multi-label model, more than 64 classes, more than one rank (the double sums
    // would need an exact all-reduce that the float transport does not give), bins outside 1..64, a temperature that is not
    // finite and > 0, and for calibrate a split without labelled rows.
    //   calibration: one forward, one gcnhip_calib_nll_rows and one gcnhip_calib_bins_rows launch at beta = 1 / temperature;
    //   sums[4] = {sum nll, sum d nll / d beta, sum d2 nll / d beta2, rows}, count / correct [bins], conf_sum [bins]: the 4 + 3 . bins
    //   numbers that cross to the host (host/calibration.h turns them into the report).
    //   calibrate: one forward, then a safeguarded Newton iteration on the convex NLL(beta) run by the host — a step is one nll
    //   launch and one 32-byte copy.  From beta = 1 inside the bracket [0.01, 100], which moves with the sign of the gradient; the
    //   Newton step beta - g / h when h > 0 and it stays strictly inside the bracket, else the geometric midpoint (while the end
    //   the step goes to is still the outer limit, the step is at least a factor 2, so a minimum that is not there is left behind
    //   within the 40 steps); stops when
    //   |delta beta| <= 1e-6 beta or after 40 steps.  at_bound: the result sits on an end of [0.01, 100] (a split the model
    //   classifies perfectly: the NLL falls in beta without end).  With bins > 0 the reliability counts of the same rows at T = 1
    //   and at the fitted T are formed by two more launches on the rows already there: count / correct / conf_sum [2 x bins].
    //   calibrate does not set the temperature.
    //   set_temperature(T != 1): predict() keeps the log-softmax rows, runs gcnhip_calib_scale_rows on the queried rows and returns
    //   the scaled prob (and logp); pred does not depend on T.  correct_and_smooth() scales its rows in place before the residual.
    //   At T == 1 (the default) neither launches anything new.  Training, eval, evaluate and the weights file ignore it.
    struct Calibrated {
        float temperature = 1.f;
        double nll_before = 0, nll_after = 0;                  // mean NLL of the split at beta = 1 and at the result
        int steps = 0;
        bool at_bound = false;
        int64_t rows = 0;
    };
    void calibration(int split, const int *nodes, int n, float temperature, int bins, double *sums, int64_t *count, int64_t *correct, double *conf_sum);
    Calibrated calibrate(int split, int bins, int64_t *count, int64_t *correct, double *conf_sum);
    void set_temperature(float t);
    float temperature() const { return temperature_; }
    // Weights file (host/weights.h): save_weights writes W1, W2 of this model (rank 0 of several writes the same weights every
    // rank holds); load_weights checks the file's widths against the model (mismatch: an error, never a reshape) and hands the
    // weights to set_weights.  Adam's moments and step count are NOT in the file: a loaded model that trains further starts
    // Adam afresh (resuming a run exactly is out of scope).
    void save_weights(const char *path);
    void load_weights(const char *path);
    DeviceTimers &device_timers() { return *timers; }
    double timer_total(timer_instance t, long *count);        // both lanes
    void timers_reset();
    // switch the per-op device-event timers on or off (both lanes).  While they are on, run_epochs does not
    // replay the captured epoch (event records per op are not part of it).
    void set_timers(bool on);
    long n_edges_local() const { return nnzA_local; }

private:
    GCNData *data;
    std::unique_ptr<GCNData> renumbered;                       // the dataset in node_order_ (owned), when the ids were not kept
    std::vector<int> node_order_;
    const char *node_order_name_ = "ids";
    void renumber_nodes(int world);
    HipEnv env;
    DeviceArena arena;                                         // every device buffer of the training context that no other object owns
    std::unique_ptr<Comm> owned_comm;
    std::unique_ptr<DeviceTimers> timers;
    RowPartition part;
    ExchangePlan xplan;                                        // layout of gathered tables, send/receive lists
    ExchangeBuffers xbuf;
    int n_local = 0;
    long nnzA_local = 0;
    int flags = 0;
    bool factored_ = false;
    void apply_factored_scales();                              // X, A^.X and the replicated X of this rank -> D^-1/2 . (them)
    int device_ = 0;
    HipGCNOptions opt_;                                        // the switches of this model (a copy; comm pointers not used after init)
    const float *eval_vals = nullptr;
    HostRng rng;

    gcnhip_graph *graph = nullptr;
    gcnhip_feat *feat = nullptr;
    // multi-GPU: the first-layer product is replicated (every rank multiplies ALL rows of X by W1): one GEMM
    // of N x F x h per forward instead of an all-gather of N x h floats over xGMI
    gcnhip_feat *feat_full = nullptr;
    gcnhip_graph *graph_l1 = nullptr;                          // this rank's rows, GLOBAL column ids
    // Aggregate-first evaluation (dense X, fused mode): A^.X of this rank's rows, built once.  An evaluation forward is
    // then ReLU((A^.X).W1) — one GEMM, no hidden-width aggregation and no exchange before the hidden layer.
    gcnhip_feat *feat_agg = nullptr;
    const float *agg_vals = nullptr;
    std::vector<Module *> eval_modules;                        // [0] owned (the GEMM on A^.X); the rest are modules[2..]
    bool h1_from_fused_eval = false;                           // the last forward on the main stream kept its hidden matrix in registers (get_var(3) rebuilds it)
    void build_agg_first_eval();
    HipGraphSum *logits_gs = nullptr;                          // the class-width aggregation (producer of Z): predict() hooks it
    // predict(): the last node query's row subset (registered on `graph`, removed when the next query differs) and scratch
    std::vector<uint32_t> pred_bits;
    gcnhip_rowset *pred_rows = nullptr;
    int32_t *d_pred = nullptr;
    float *d_prob = nullptr, *d_logp = nullptr;
    const float *full_vals = nullptr;
    bool replicate_l1 = false;
    bool rebuild_dh1 = false;                                  // multi-GPU backward: gather dZ0 + mask bits, rebuild dH1 everywhere
    uint32_t *d_pos_bits = nullptr;                            // [table_rows * wpr]
    std::vector<std::unique_ptr<HipVariable>> variables;       // index = reference variable number
    HipVariable *input = nullptr, *output = nullptr;
    const float *input_vals = nullptr;                         // what SparseMatmul reads
    std::vector<Module *> modules;
    std::unique_ptr<HipAdam> optimizer;

    float *gradbuf = nullptr;                                  // [W1.grad | W2.grad | result(4)] one all-reduce
    size_t gradbuf_elems = 0;
    float *d_result = nullptr;
    int32_t *d_result_i = nullptr;
    int32_t *d_truth[4] = {};                                  // per split code 1..3
    ScoredSplit scored;                                        // follows set_truth
    void fill_scored(ScoredSplit &d, int s, gcnhip_rowset *const *rows) const;
    uint32_t *d_ml_truth = nullptr;                            // multi-label: this rank's rows of GCNData::multihot
    int ml_wpr = 0;
    float *d_ml_logits = nullptr;                              // predict_multilabel: scratch logits [local rows x ld of Z]
    uint32_t *d_ml_bits = nullptr;
    float *d_ml_prob = nullptr;
    int32_t *d_ml_rows = nullptr;
    size_t ml_query_cap = 0;
    std::pair<float, float> ring_metrics(const float *row) const;   // (loss + L2, accuracy or micro-F1) of a metrics-ring row
    void query_rows(const char *what, const int *nodes, int n, std::vector<int> &rows);   // dataset ids -> local rows (predict*)
    const gcnhip_rowset *query_subset(const std::vector<int> &rows);
    void forward_hooked(const HipGraphSum::Prediction *prediction, const HipGraphSum::Redirect *redirect);
    float *ml_logits_scratch();
    void pred_scratch();                                       // d_pred / d_prob, on first use
    // evaluate(): the counts on the device (also the float limbs of their all-reduce), an uploaded row list, every local label
    int32_t *d_eval_counts = nullptr, *d_eval_rows = nullptr, *d_label_all = nullptr;
    size_t eval_rows_cap = 0;
    // propagate / label_propagation / correct_and_smooth: four tables [local rows x smooth_ld], the merged truth of the known
    // splits, sigma = {sum |E_0|, rows}
    float *d_smooth[4] = {};
    int smooth_ld = 0;
    int32_t *d_smooth_truth = nullptr;
    float *d_sigma = nullptr;
    static int smooth_row_ld(int dim) { return dim <= 32 ? (dim + 3) / 4 * 4 : (dim + 15) / 16 * 16; }   // HipVariable's rule
    void smooth_check(const char *what, float alpha, int iters) const;
    void smooth_tables(int ld);
    const int32_t *smooth_truth(const char *what, int splits_mask, std::vector<int32_t> *host);
    float *smooth_iterate(const float *base, float *a, float *b, int ld, int dim, float alpha, int iters, float lo, float hi, int32_t *pred);
    void smooth_download(const float *table, int ld, int dim, float *out, int32_t *pred_from_rows);
    void smooth_pred_download(int32_t *pred);
    // calibration / calibrate: {nll sums [4] | conf_sum [2 x 64]} doubles and {count, correct} [2 x 2 x 64] ints on the device
    float temperature_ = 1.f;
    double *d_calib_sums = nullptr;
    int32_t *d_calib_counts = nullptr;
    void calib_check(const char *what, float temperature, int bins) const;
    // the rows a split or a query names, as evaluate() lists them, and the truth they are scored against
    struct ScoredRows { const int32_t *d_list; int n; const int32_t *truth; const gcnhip_rowset *subset; };
    ScoredRows scored_rows(const char *what, int split, const int *nodes, int n);
    const int32_t *upload_rows(const std::vector<int> &rows);
    void forward_logp(const gcnhip_rowset *subset);            // predict()'s hooked forward, d_logp kept
    void calib_bins_download(const ScoredRows &q, float beta, int bins, int slot, int64_t *count, int64_t *correct, double *conf_sum);
    gcnhip_graph *graph_bwd_out = nullptr;                     // `graph` without the edges whose source is outside the training split
    // HIPGCN_OVERLAP_EXCHANGE: `graph` and `graph_bwd_out` cut by column owner (own rows / other ranks' rows), the split
    // subsets of the last aggregation on both halves, and the exchange stream
    gcnhip_graph *graph_loc = nullptr, *graph_rem = nullptr, *graph_bwd_loc = nullptr, *graph_bwd_rem = nullptr;
    gcnhip_rowset *split_rows_loc[4] = {}, *split_rows_rem[4] = {};
    std::unique_ptr<ExchangeLane> xlane;
    void build_overlap();
    void wire_overlap(HipGraphSum *gs, bool output_layer);
    std::vector<uint32_t> h_train_bits;
    uint32_t *d_train_bits = nullptr;                          // bit per (padded) node: in the training split
    const uint32_t *bwd_bits = nullptr;
    gcnhip_rowset *split_rows[4] = {};                         // rows of `graph` whose node is in split s (all the loss reads); owned by graph
    int32_t *d_split_list[4] = {};                             // local row ids of split s, ascending (the loss walks only these)
    int split_local_n[4] = {};
    int split_count[4] = {};
    float *d_class_w = nullptr;                                // class weights [C] (HipGCNOptions::class_weights), else NULL
    float split_wsum[4] = {};                                  // single-label: sum of w[label] over split s, all ranks (the weighted gradient's divisor)
    float *d_ring = nullptr;
    static constexpr int RING = 1024;
    uint8_t *d_keep0 = nullptr, *d_keep1 = nullptr;
    std::vector<uint8_t> h_keep0, h_keep1;
    long keep0_first = 0;                                      // global nnz index of h_keep0[0]
    long epochs_done = 0;                                      // training passes enqueued = *env.d_epoch once their Adam launches have run
    void *epoch_graph = nullptr;                               // captured train_epoch + eval(2)
    bool enqueue_epoch_replay();                               // one epoch from the captured hipGraph (captures it on first use); false: not replayable
    bool zipped() const { return lane && !(timers->enabled && env.comm->size() == 1); }   // validation on the lane, beside the next training pass
    void enqueue_epoch(bool first, bool last);
    void print_line(long epoch, std::pair<float, float> train, std::pair<float, float> scored_now, float dt) const;
    // run(): read-back of an epoch's metrics row without stalling the producer streams
    static constexpr int PIPELINE_DEPTH = 4;                   // read-back groups in flight
    static constexpr int READBACK_GROUP_MAX = 64;              // epochs per read-back group, at most (RING is a multiple)
    static constexpr int READBACK_CALIBRATION = 16;            // epochs read back one by one before the group size is set
    static constexpr double READBACK_GROUP_SECONDS = 2e-3;     // a group spans about this long
    struct Readback {
        gcnhip_ctx *ctx = nullptr;                             // its own stream (NULL: copies go on the producer's)
        float *host = nullptr;                                 // pinned [PIPELINE_DEPTH][READBACK_GROUP_MAX][32]: whole ring rows
        void *ev_ready[PIPELINE_DEPTH] = {}, *ev_copied[PIPELINE_DEPTH] = {};
    };
    std::unique_ptr<Readback> readback;
    void readback_create(bool own_stream);
    void readback_destroy();
    void readback_enqueue(long first_epoch_index, int n_epochs, int slot, gcnhip_ctx *producer);
    void run_synchronous();
    void run_pipelined();
    void report_test();

    // Validation lane.  eval(e) reads only the weights Adam(e) wrote, and train(e+1) needs the same
    // weights and nothing from eval(e): the two are independent until Adam(e+1).  With more than one GPU
    // each of them alternates compute with an all-gather, so running eval(e) on its own stream /
    // communicator / activation buffers lets one lane compute while the other communicates.
    struct EvalLane {
        HipEnv env;
        DeviceArena arena;                                     // on the lane's context
        ExchangeBuffers xbuf;
        std::unique_ptr<Comm> comm;
        std::unique_ptr<DeviceTimers> timers;
        gcnhip_graph *graph = nullptr;                         // own split-row scratch
        gcnhip_graph *graph_l1 = nullptr;
        std::unique_ptr<HipVariable> H0, H1, Z0, Z;
        std::vector<Module *> modules;
        float *d_result = nullptr;
        int32_t *d_result_i = nullptr;
        gcnhip_rowset *split_rows[4] = {};                     // the lane has its own adjacency object
        ScoredSplit scored;
        void *ev_weights = nullptr, *ev_done = nullptr;        // Adam(e) -> eval(e);  eval(e) -> Adam(e+1)
        void *ev_fork = nullptr;                               // one GPU: training GEMM done -> the validation pass may start
        bool pending = false;
        long epoch_word = -1;                                  // host shadow of *env.d_epoch (starts at 0xFFFFFFFF)
    };
    std::unique_ptr<EvalLane> lane;
    void init(const HipGCNOptions &opt);
    void release();                                            // frees everything that exists; safe on a half-built object
    void destroy_lane();
    void build_eval_lane();
    void eval_on_lane(int current_split);
    void lane_begin(int current_split);
    void lane_end(int current_split);
    void eval_then_train_zipped(int current_split);
    void train_begin();
    void train_end();
    void refresh_input();
    void metrics_before(HipEnv &e, int slot, const uint32_t *epoch_word);
    void metrics_after(HipEnv &e, DeviceTimers &t, int slot, const uint32_t *epoch_word, float *result, size_t n);
    gcnhip_graph *create_rows_graph(gcnhip_ctx *ctx);          // this rank's rows of the adjacency, GLOBAL column ids, width reserved

    // row schedule of the aggregation (gcnhip_graph_set_schedule): candidates timed once, fastest kept
    int sched_mode = 0, sched_groups = 0, slice_floats = 64;
    bool labels_assortative = false;
    std::vector<int> structure_group;                          // per node: group found in the graph (cluster.h); empty: none useful
    int structure_n_groups = 0;
    void tune_schedule();
    void choose_slice_width();
    void apply_schedule(gcnhip_ctx *ctx, gcnhip_graph *g);
    void add_split_rowsets(gcnhip_ctx *ctx, gcnhip_graph *g, gcnhip_rowset *out[4]);
    void build_modules();
    // what differs between the sites that build a loss module (make_loss)
    struct LossSite {
        HipEnv *env;
        HipVariable *Z;                         // the logits
        const ScoredSplit *split;               // what the loss scores: the fields are read at every forward
        float *d_result;
        int32_t *d_result_i;
        bool shift_in_place;
        const float *grad_row_scale;
        bool list_rows;                         // false: the single-label loss visits every row, as the reference does
        HipGraphSum *epilogue;                  // the aggregation that may carry the loss epilogue, or NULL
    };
    Module *make_loss(const LossSite &s);
    void set_truth(int current_split);
    void host_masks_for_epoch();
    void train_epoch_async();
    void eval_async(int current_split);
    std::pair<float, float> read_metrics(long epoch_index, int slot);
};
