/*
 * gcnhost.h — C entry points of libgcnhost.so: the C++ host side of the GCN
 * training path (HipGCN and its Hip* modules, cuda_gcn_amd/host/) for callers
 * that are not C++ (bench.py, tests, __graft_entry__.smoke()).
 *
 * The host mirrors the reference's driver: GCN(GCNParams, GCNData*) + run()
 * (src/seq/gcn.h:24-44; CUDA twin src/cuda/cuda_gcn.cuh:11-34).  It reaches
 * the GPU only through include/gcnhip.h (and RCCL for more than one GPU).
 * Every function returns 0 on success, else the failing HIP/RCCL code (or -1);
 * gcnhost_last_error() gives the message.
 */
#ifndef GCNHOST_H
#define GCNHOST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

typedef struct gcnhost_model gcnhost_model;

/* GCNParams of the reference (src/seq/gcn.h:9-14), same field order */
typedef struct {
    int num_nodes, input_dim, hidden_dim, output_dim;
    float dropout, learning_rate, weight_decay;
    int epochs, early_stopping;
} gcnhost_params;

enum {
    GCNHOST_MODULAR = 1,      /* one module per reference module (no fused epilogues) */
    GCNHOST_HOST_MASKS = 2,   /* dropout decisions replayed from the reference's host RNG (parity runs) */
    GCNHOST_TIMERS = 4,       /* per-op device-event timers */
    GCNHOST_NO_GRAPH = 8,     /* run_epochs never replays a captured hipGraph */
    GCNHOST_EVAL_LANE = 16,   /* validation forward on a second stream, overlapped with the next training epoch */
    GCNHOST_NO_EVAL_LANE = 32, /* never (default: on when world > 1) */
    GCNHOST_NO_REPLICATE_L1 = 64, /* multi-GPU: all-gather H0 instead of replicating the first-layer product */
    GCNHOST_REPLICATE_L1 = 128,   /* force the replication (default: on for 2-4 GPUs, off for 8) */
    GCNHOST_GATHER_DH1 = 256,     /* multi-GPU backward: all-gather dH1 instead of dZ0 + mask bits */
    GCNHOST_NO_ROW_GROUPS = 512,  /* keep the plain descending-degree row schedule (no load-time timing of alternatives) */
    GCNHOST_BF16_TABLES = 2048,   /* opt-in, beyond the reference: the aggregation gathers bfloat16 copies of H0, Z0, dZ, dH1 (f32 sums) */
    GCNHOST_ALL_ROWS = 4096,      /* compute every row of the logits (default: the last aggregation computes only the rows of the
                                     scored split — all that loss and accuracy read; env HIPGCN_ALL_ROWS=1 does the same) */
    GCNHOST_NO_AGG_FIRST_EVAL = 8192, /* evaluation forwards keep the reference's order A^.(X.W1); default for a dense X: (A^.X).W1 with
                                         A^.X built once (no hidden-width aggregation in eval; env HIPGCN_NO_AGG_FIRST_EVAL=1 does the same) */
    GCNHOST_EXCHANGE_ALLGATHER = 16384, /* multi-GPU: always all-gather whole row blocks before an aggregation */
    GCNHOST_EXCHANGE_HALO = 32768,      /* ... or always exchange only the needed rows, peer to peer (default: decided per graph;
                                           env HIPGCN_EXCHANGE=halo|allgather) */
    /* 65536 and 262144 are retired (measured-slower variants, removed): not to be reused; setting them selects the default path */
    GCNHOST_NO_LABEL_HINT = 524288,   /* the labels are never used as row groups of the aggregation's schedule; groups are looked for in the
                                         graph itself (modularity local moving) and used if they time faster (env HIPGCN_NO_LABEL_HINT=1) */
    GCNHOST_MASKED_BWD = 131072,      /* the output layer's backward masks the rows of dZ outside the training split at every launch
                                         (default: aggregates through gcnhip_graph_create_restricted's operator; env HIPGCN_MASKED_BWD=1) */
    GCNHOST_NULL_COMM = 1024      /* timing aid: rank r of world > 1 with no-op collectives (per-rank compute time; numbers meaningless) */
};

#define GCNHOST_NCCL_ID_BYTES 128
typedef void (*gcnhost_allgather_fn)(void *user, float *host_full, size_t block_elems);
typedef void (*gcnhost_allreduce_fn)(void *user, double *host_buf, size_t n);

const char *gcnhost_last_error(void);
gcnhost_params gcnhost_params_default(void);               /* gcn.cpp:9-11 */
int gcnhost_nccl_unique_id(char id[GCNHOST_NCCL_ID_BYTES]);   /* rank 0; broadcast it to the others */

/* Build the model from the whole dataset in the reference's in-memory layout
 * (GCNData, src/seq/gcn.h:16-22: adjacency CSR with the self loop first,
 * feature CSR + values, split, label); each rank keeps its own row block.
 * f_indices may be NULL for a dense X (every row = columns 0..input_dim-1).
 * seed plays time(NULL) of src/seq/rand.cpp:7.  world > 1: nccl_id (from
 * gcnhost_nccl_unique_id) selects RCCL; or pass host callbacks for a
 * host-staged transport (tests). */
int gcnhost_model_create(gcnhost_model **m, const gcnhost_params *p,
                         const int *g_indptr, const int *g_indices,
                         const int *f_indptr, const int *f_indices, const float *f_val,
                         const int *split, const int *label,
                         long seed, int device, int flags,
                         int rank, int world, const char *nccl_id,
                         gcnhost_allgather_fn host_ag, gcnhost_allreduce_fn host_ar, void *host_user);
/* The same model in multi-label mode (beyond the reference): multihot = the truth as num_nodes rows of ceil(output_dim / 32)
 * uint32 words, bit (c & 31) of word c >> 5 = class c of the node (1 <= output_dim <= 256).  label may be NULL (it then only
 * serves the aggregation's schedule hint, which it skips).  The loss is the per-class sigmoid cross-entropy, and the
 * accuracy of train_epoch / eval / run_epochs / run is micro-F1 (gcnhip_bce_fwd_rows). */
int gcnhost_model_create_multilabel(gcnhost_model **m, const gcnhost_params *p,
                                    const int *g_indptr, const int *g_indices,
                                    const int *f_indptr, const int *f_indices, const float *f_val,
                                    const int *split, const int *label, const uint32_t *multihot,
                                    long seed, int device, int flags,
                                    int rank, int world, const char *nccl_id,
                                    gcnhost_allgather_fn host_ag, gcnhost_allreduce_fn host_ar, void *host_user);
/* Either of the two with per-class loss weights (beyond the reference; host/class_weights.h): class_weights [output_dim], finite
 * and not negative, at most 256 classes.  multihot == NULL: a single-label model whose loss is the weighted mean
 * sum(w[t] . term) / sum(w[t]) over the scored split (gcnhip_wxent_fwd_rows; torch's cross_entropy(weight=)); accuracy is not
 * weighted.  multihot != NULL: class_weights is the weight of every class's positive term (gcnhip_wbce_fwd_rows; torch's
 * BCEWithLogitsLoss(pos_weight=)).  class_weights == NULL: exactly gcnhost_model_create / gcnhost_model_create_multilabel.
 * Refused with a message: a negative / NaN / infinite weight, a non-empty split whose weights sum to 0 (single-label).
 * predict, evaluate, save / load of weights work on such a model as on any other. */
int gcnhost_model_create_weighted(gcnhost_model **m, const gcnhost_params *p,
                                  const int *g_indptr, const int *g_indices,
                                  const int *f_indptr, const int *f_indices, const float *f_val,
                                  const int *split, const int *label, const uint32_t *multihot, const float *class_weights,
                                  long seed, int device, int flags,
                                  int rank, int world, const char *nccl_id,
                                  gcnhost_allgather_fn host_ag, gcnhost_allreduce_fn host_ar, void *host_user);
/* "Balanced" class weights from the rows of split which_split (1 = train), host only.  multihot == NULL: w_c = n / (C . n_c)
 * over the rows whose label is in [0, C) (n their number, n_c those of class c; 0 when n_c = 0) — scikit-learn's rule.
 * multihot != NULL (label may be NULL): pw_c = (n - pos_c) / pos_c over the split's rows (1 when pos_c = 0) — the rule PyTorch
 * documents for pos_weight.  weights [num_classes]. */
int gcnhost_balanced_class_weights(int num_nodes, int num_classes, const int *split, const int *label, const uint32_t *multihot,
                                   int which_split, float *weights);
/* A class weights text file, host only: one float per line, one line per class.  *num_classes > 0: the file must have that many
 * lines; it receives the number read.  weights may be NULL (check and count only).  A wrong line count, a token that is not a
 * number, a negative, NaN or infinite value is an error whose message names the line. */
int gcnhost_class_weights_read(const char *path, int *num_classes, float *weights);
int gcnhost_model_destroy(gcnhost_model *m);

int gcnhost_model_train_epoch(gcnhost_model *m, float *loss, float *acc);      /* gcn.cpp:107-118; synchronises */
int gcnhost_model_eval(gcnhost_model *m, int split, float *loss, float *acc);  /* gcn.cpp:120-128; synchronises */
/* n x (train_epoch + eval(2)) enqueued back to back, one synchronisation at the
 * end; trace (may be NULL) gets train_loss, train_acc, val_loss, val_acc per epoch */
int gcnhost_model_run_epochs(gcnhost_model *m, int n, float *trace);
int gcnhost_model_run(gcnhost_model *m);                                       /* gcn.cpp:130-158, prints the reference's lines */
int gcnhost_model_sync(gcnhost_model *m);

/* introspection */
/* multi-GPU: how this rank's gathered tables are completed (halo = 1: per-peer send lists; 0: whole-block all-gather),
 * rows received / sent per exchange, rows of a table, and the share of remote rows the neediest rank reads */
int gcnhost_model_exchange(gcnhost_model *m, int *halo, int64_t *recv_rows, int64_t *send_rows, int *table_rows, double *halo_share);
int gcnhost_model_info(gcnhost_model *m, int *rank, int *world, int *row_start, int *local_rows, int64_t *local_edges);
/* the aggregation's row schedule this rank timed as fastest: 0 descending degree (also when not tuned), 1 label-major,
 * 2 degree rank dealt into n_groups groups, 3 group-major over n_groups groups found in the graph (modularity local moving) */
/* Several GPUs: the model may renumber the nodes by structure before partitioning them (rank blocks are contiguous in the
 * node order; HIPGCN_ID_PARTITION keeps the ids, HIPGCN_STRUCTURE_PARTITION forces the renumbering).  ids[r] (local_rows
 * entries) = the node of the caller's dataset that local row r of this rank is; *renumbered = 0 when the ids were kept. */
int gcnhost_model_row_ids(gcnhost_model *m, int *ids, int *renumbered);
/* factored aggregation (gcn.h, HIPGCN_EDGE_COEF restores the reference's per-edge coefficients): *factored says whether
 * gcnhost_model_get_var returns the gathered matrices pre-multiplied by dinv = 1/sqrt(deg) of their row (variables 1, 3, 4;
 * the logits, weights and weight gradients are never scaled); dinv [local_rows] receives that factor (may be NULL) */
int gcnhost_model_row_scale(gcnhost_model *m, float *dinv, int *factored);
int gcnhost_model_schedule(gcnhost_model *m, int *mode, int *n_groups);
/* the layer that moves this model's rows between ranks ("rccl", "host callbacks", "none") and the number of ranks THAT layer
 * counts (RCCL: ncclCommCount of the model's communicator) */
int gcnhost_model_transport(gcnhost_model *m, int *ranks, char name[32]);
/* column-slice width (floats) the hidden-width aggregation was tuned to at load: 64 (two slices of a 128-wide row) or 32 */
int gcnhost_model_slice_floats(gcnhost_model *m, int *floats);
/* variable k of gcn.cpp:21-54 (1 H0, 2 W1, 3 H1, 4 Z0, 5 W2, 6 Z): this rank's rows, row-major rows x cols.
 * out == NULL: only report the shape. */
/* Variable k of the reference's list (gcn.cpp:21-54: 1 H0, 2 W1, 3 H1, 4 Z0, 5 W2, 6 Z), this rank's rows, row-major rows x cols
 * (call with out == NULL for the shape).  Variable 6 holds CURRENT logits only for the rows of the split scored by the last
 * forward (train_epoch: split 1; eval(s): split s) unless the model was built with GCNHOST flag ALL_ROWS (4096): the
 * default path does not compute rows nobody reads; the reference fills every row. */
int gcnhost_model_get_var(gcnhost_model *m, int k, int grad, float *out, int *rows, int *cols);
int gcnhost_model_set_weights(gcnhost_model *m, const float *w1, const float *w2);
/* Prediction (beyond the reference): an evaluation forward with the current weights whose logit aggregation writes, per node,
 * the class with the largest logit (the lowest class on a tie: numpy.argmax's rule; the reference's accuracy test counts a tie
 * with the true class as correct) and its softmax probability.  nodes: n dataset node ids, each a row of this rank (repeats
 * allowed); NULL: every row of this rank in local-row order (gcnhost_model_row_ids names them).  pred / prob [n]; logp
 * (may be NULL) [n x output_dim] the log-softmax rows.  Several ranks: every rank calls it (the logit aggregation exchanges
 * rows).  Training state is not touched: a train_epoch after it gives the same bits as one without it.  Synchronises. */
int gcnhost_model_predict(gcnhost_model *m, const int *nodes, int n, int32_t *pred, float *prob, float *logp);
/* Multi-label prediction, the same contract as gcnhost_model_predict: bits [n x ceil(output_dim / 32)] the predicted class
 * sets (bit c = logit c > 0), prob (may be NULL) [n x output_dim] the sigmoid of every logit.  Only on a model made by
 * gcnhost_model_create_multilabel (and gcnhost_model_predict only on one that was not). */
int gcnhost_model_predict_multilabel(gcnhost_model *m, const int *nodes, int n, uint32_t *bits, float *prob);
/* Per-class evaluation (beyond the reference): one evaluation forward with the current weights over a set of rows, and integer
 * counts per class formed on the GPU behind it (gcnhip_confusion_rows / gcnhip_bce_class_counts_rows).  Rows: the nodes of
 * split 1 (train), 2 (validation) or 3 (test) on this rank; or, with split == 0, the `nodes` query with
 * gcnhost_model_predict's conventions (repeats are counted as often as listed; NULL: every row of this rank).
 * Single-label model: counts [output_dim x output_dim], counts[t * C + p] = rows with truth t predicted as p (the lowest class
 * on a logit tie), *rows_counted = the rows in the matrix, *unlabelled = rows whose truth is outside [0, C) (in no cell).
 * Multi-label model: counts [3 x output_dim] = TP, FP, FN per class (logit > 0 predicts the class), *rows_counted = the rows,
 * *unlabelled = 0.  Several ranks: every rank calls it; the counts are summed exactly over the ranks and every rank receives
 * the same totals.  Only the counts cross to the host.  Training state is not touched, as for gcnhost_model_predict.
 * More than 64 (single-label) or 256 (multi-label) classes is an error.  Synchronises. */
int gcnhost_model_evaluate(gcnhost_model *m, int split, const int *nodes, int n, int64_t *counts, int64_t *rows_counted, int64_t *unlabelled);
/* Label propagation and Correct & Smooth (beyond the reference): the graph and the known labels used at inference time.  Every
 * iteration is one gcnhip_graphsum_blend launch over this model's adjacency, ping-ponging two device tables; arrays are in
 * DATASET node order, [num_nodes x width] row-major.  gcnhost_model_predict's contract holds: the call synchronises first, and
 * the training state (metrics ring, current split, variable 6, the captured epoch graph) is untouched.  One rank only: with
 * several, every iteration would need a table exchange — refused with a message.  Refused before any launch, too: alpha outside
 * [0, 1], iters < 0, a width outside 1..64 and, for the two label schemes, a multi-label model or more than 64 classes.
 * splits_mask: bit s set = the labelled nodes of split s (1 train, 2 validation, 3 test) are known; e.g. 2 = train only.
 *
 * gcnhost_model_propagate: Y_0 = y0 [num_nodes x dim]; Y_{k+1} = min(max(alpha . A^ . Y_k + (1 - alpha) . Y_0, lo), hi); out
 * [num_nodes x dim] = Y_iters (iters == 0: y0), pred (may be NULL) [num_nodes] = its argmax per row, lowest column on a tie.
 * dim need not be the model's class count and no trained weights are needed.
 * gcnhost_model_label_propagation: propagate with Y_0 = the one-hot rows of the known nodes whose label is in [0, C), zero rows
 * elsewhere, clamp [0, 1]; pred [num_nodes], y (may be NULL) [num_nodes x output_dim].
 * gcnhost_model_correct_and_smooth (Huang et al., 2020): P = softmax of one evaluation forward (log-softmax kept on the device);
 * E_0 = onehot - P on the known rows, zero elsewhere (gcnhip_cs_error_rows); E_{k+1} = clamp(a1 . A^ . E_k + (1 - a1) . E_0, -1, 1);
 * G_0 = the one-hot row on known rows, P + s . E^ elsewhere with the autoscale s of gcnhip_cs_correct_rows;
 * G_{k+1} = clamp(a2 . A^ . G_k + (1 - a2) . G_0, 0, 1), whose last launch writes pred.  Only pred [num_nodes] must cross to the
 * host; g (may be NULL) [num_nodes x output_dim] is copied when asked for. */
int gcnhost_model_propagate(gcnhost_model *m, const float *y0, int dim, float alpha, int iters, float lo, float hi, float *out, int32_t *pred);
int gcnhost_model_label_propagation(gcnhost_model *m, float alpha, int iters, int splits_mask, int32_t *pred, float *y);
int gcnhost_model_correct_and_smooth(gcnhost_model *m, float alpha_correct, int iters_correct, float alpha_smooth, int iters_smooth,
                                     int splits_mask, int32_t *pred, float *g);
/* Temperature scaling and calibration error (beyond the reference; Guo et al., 2017).  predict's probabilities are softmax(z / T)
 * with one scalar T, 1 by default; these fit it, measure what it does, and set it.  All work on the log-softmax rows of one
 * evaluation forward kept on the device, with the row-local kernels gcnhip_calib_nll_rows / _bins_rows / _scale_rows, and hold
 * gcnhost_model_predict's contract: the call synchronises first and the training state is untouched.  Single-label models, at most
 * 64 classes, one rank; 1 <= bins <= 64; a temperature is finite and > 0 with the f32 quotient 1 / T at most GCNHIP_BETA_MAX = 8e37
 * (T >= 1.25e-38; gcnhip_driver.h derives the limit): anything else is refused with a message before any launch.
 *
 * gcnhost_model_calibration: the rows of `split` (1 train, 2 validation, 3 test), or with split == 0 the `nodes` query (n dataset
 * ids; NULL: every row) scored against the dataset's labels, at `temperature`.  sums[4] = {sum of the rows' negative
 * log-likelihood, its first and second derivative in beta = 1 / T, rows counted}; count / correct / conf_sum [bins]: rows, rows
 * predicted right and the sum of confidences (largest probability) per bin (b / bins, (b + 1) / bins].
 * gcnhost_model_calibrate: fits T on `split` by a safeguarded Newton iteration on the convex NLL(beta), beta in [0.01, 100], one
 * launch and a 32-byte copy per step.  out[6] = {T, mean NLL at T = 1, mean NLL at the result, steps, 1 when the result sits on
 * an end of the bracket (a split classified perfectly), rows}.  bins > 0: count / correct / conf_sum [2 x bins] = the reliability
 * counts of the same rows at T = 1 and at the fitted T; bins == 0: the three may be NULL.  It does not set the temperature.
 * gcnhost_model_set_temperature: from now on predict returns prob (and logp) at this T (pred does not depend on it) and
 * correct_and_smooth starts from the calibrated softmax; at T = 1 both launch exactly what they did.  Training, eval, evaluate and
 * the weights file ignore it.
 * gcnhost_calibration_report, host only (host/calibration.h): accuracy / confidence [bins] per bin (0 for an empty bin),
 * summary[3] = {ECE = sum_b (count_b / rows) |accuracy_b - confidence_b|, MCE = the largest gap of a non-empty bin, rows};
 * every output may be NULL. */
int gcnhost_model_calibration(gcnhost_model *m, int split, const int *nodes, int n, float temperature, int bins, double *sums, int64_t *count,
                              int64_t *correct, double *conf_sum);
int gcnhost_model_calibrate(gcnhost_model *m, int split, int bins, double *out, int64_t *count, int64_t *correct, double *conf_sum);
int gcnhost_model_set_temperature(gcnhost_model *m, float temperature);
int gcnhost_model_temperature(gcnhost_model *m, float *temperature);
int gcnhost_calibration_report(int bins, const int64_t *count, const int64_t *correct, const double *conf_sum, double *accuracy,
                               double *confidence, double *summary);
/* Split conformal prediction sets (beyond the reference; ModelQueries::conformal_fit / conformal_sets, kernels in csrc/conformal.hip):
 * a set of classes per node that holds the true class with probability >= 1 - alpha, from a threshold fitted on a held-out split.
 * Both model calls hold gcnhost_model_predict's contract (the call synchronises first, the training state is untouched) and work at
 * the model's current temperature.  Single-label models, at most 64 classes, one rank, alpha in (0, 1), method 0 (LAC: 1 - p) or
 * 1 (APS: the cumulated probability down to the class, plus lam . max(0, rank + 1 - k_reg)), lam >= 0, k_reg >= 0, diffusion in [0, 1]
 * (the scores blended with their neighbourhood mean, d . A^ . S + (1 - d) . S): anything else is refused with a message before any launch.
 *
 * gcnhost_model_conformal_fit: the rows of `split` (1 train, 2 validation, 3 test) or, with split == 0, the `nodes` query (n dataset ids;
 * NULL: every row) scored against the dataset's labels.  Fills *fit: thresh / n_cal [64] — without per_class the one threshold and the
 * number of scored rows in every entry below the class count, with it one per label.  scores (may be NULL; room for scores_cap floats):
 * the true-class score of every listed row, -1 for a row without a label; *n_scores (may be NULL) their number.  A split without
 * labelled rows is refused.
 * gcnhost_model_conformal_sets: the sets of the listed rows under *fit.  bits [n x ceil(C / 32)] and size [n] by list position (either may
 * be NULL), counts (may be NULL) [4 + 3 C + 1] = {rows, labelled rows, covered, empty sets | size_hist [C + 1] | class_support [C] |
 * class_covered [C]}.  Refused: a NaN threshold, and a fit made at another temperature than the model's current one.
 * gcnhost_conformal_quantile, host only (host/conformal.h): negative scores are dropped; with n' left, k = ceil((n' + 1)(1 - alpha)) in
 * double and the threshold is the k-th smallest score, +inf when k > n'.  labels == NULL: thresh / n_cal / k hold one entry;
 * else scores are grouped by labels[i] in [0, num_classes) and each holds num_classes entries.  n_cal and k may be NULL. */
typedef struct gcnhost_conformal {
    int method;
    float lam;
    int k_reg;
    float diffusion, temperature;
    double alpha;
    int per_class;
    float thresh[64];
    int64_t n_cal[64];
} gcnhost_conformal;
int gcnhost_model_conformal_fit(gcnhost_model *m, int split, const int *nodes, int n, double alpha, int method, float lam, int k_reg,
                                float diffusion, int per_class, gcnhost_conformal *fit, float *scores, int64_t scores_cap, int64_t *n_scores);
int gcnhost_model_conformal_sets(gcnhost_model *m, const gcnhost_conformal *fit, int split, const int *nodes, int n, uint32_t *bits,
                                 int32_t *size, int64_t *counts);
int gcnhost_conformal_quantile(const float *scores, int64_t n, double alpha, const int32_t *labels, int num_classes, float *thresh,
                               int64_t *n_cal, int64_t *k);
/* Ranking metrics (beyond the reference; ModelQueries::ranking, kernels in csrc/ranking.hip): per-class ROC-AUC and average
 * precision without a decision threshold.  Rows as gcnhost_model_evaluate takes them (split 1..3, or split == 0 with the `nodes`
 * query; repeats count as often as listed), gcnhost_model_predict's contract (the call synchronises first, the training state is
 * untouched).  A multi-label model is scored on its logits, a single-label one one-vs-rest on the log-softmax rows at the model's
 * current temperature (what gcnhost_model_predict returns as logp).  One rank, at most 64 (single-label) or 256 (multi-label)
 * classes, at most 2^24 listed rows: anything else is refused with a message before any launch.
 *
 * gcnhost_model_ranking: per class c of C = output_dim, over the listed rows with a label in [0, C) (every row of a multi-label
 * model) and a score that is not NaN: pos[c] / neg[c] = its positives P / negatives N; u2[c] = sum over the positives of
 * #{negatives scored lower} + #{negatives scored not higher} (exact); ap_sum[c] = sum over the positives of TP_ge / (TP_ge + FP_ge),
 * the positives / negatives scored not lower (float64); invalid[c] = labelled rows with a NaN score; *unlabelled = rows with a
 * label outside [0, C); *rows = the listed rows.  scratch_bytes: the cap of the key tables and the sort scratch (0: 256 MiB); the
 * classes run in batches that fit it, at least one at a time, with the same bits in every batching.  scores (may be NULL; room for
 * scores_cap floats, else refused): the [rows x C] f32 score rows in list order.
 * gcnhost_ranking_report, host only (host/ranking.h): auc[c] = u2 / (2 P N), defined (auc_defined[c] = 1) when P > 0 and N > 0;
 * ap[c] = ap_sum / P, defined when P > 0; an undefined value is 0, never NaN.  summary[5] = {macro_auc, macro_ap, weighted_auc,
 * weighted_ap, classes with an AUC}: the macro means run over the defined classes only, the weighted ones weigh them by P.
 * Refused: C < 1, a negative count, u2 outside [0, 2 P N], ap_sum outside [0, P]. */
int gcnhost_model_ranking(gcnhost_model *m, int split, const int *nodes, int n, size_t scratch_bytes, int64_t *u2, double *ap_sum, int64_t *pos,
                          int64_t *neg, int64_t *invalid, int64_t *unlabelled, int64_t *rows, float *scores, int64_t scores_cap);
int gcnhost_ranking_report(int num_classes, const int64_t *u2, const double *ap_sum, const int64_t *pos, const int64_t *neg, double *auc, double *ap,
                           int32_t *auc_defined, int32_t *ap_defined, double *summary);
/* Multi-label decision thresholds (beyond the reference; ModelQueries::tune_thresholds, kernels in csrc/thresholds.hip): one cut per
 * class on the logit in place of the training rule logit > 0.  Rule: class c is predicted for a row exactly when its logit z is not
 * NaN and z >= thr[c], compared on the order-preserving integer keys of gcnhip_rank_keys (-0.0 == +0.0; denormals as the numbers
 * they are).  Multi-label models, one rank, at most 256 classes; all hold gcnhost_model_predict's contract (the call synchronises
 * first, the training state is untouched).
 *
 * gcnhost_model_tune_thresholds: rows as gcnhost_model_evaluate takes them (split 1..3, or split == 0 with the `nodes` query).  Per
 * class c over the listed rows whose logit is not NaN, P positives and N negatives (pos / neg; invalid[c] = the NaN rows): the
 * candidates are the logits of the positives; at a cut TP / FP = the positives / negatives scored not lower, FN = P - TP, and in
 * float64, in this order, w = beta * beta, num = (1 + w) TP, den = num + w FN + FP, F = num / den.  thr[c] = the candidate with the
 * largest F, the highest one among equal F; tp / fp / fn [C] its counts, f[c] its F, defined[c] = 1.  P == 0: defined[c] = 0,
 * thr[c] = 0, tp = fn = 0, fp = the negatives scored >= 0, f = 0.  beta finite and > 0; at most 2^24 listed rows; scratch_bytes as
 * for gcnhost_model_ranking (the same batches, the same bits in every batching).  Only these O(C) numbers cross to the host.
 * *rows (may be NULL) = the listed rows.
 * gcnhost_model_predict_multilabel_thr / gcnhost_model_evaluate_thr: gcnhost_model_predict_multilabel and the multi-label
 * gcnhost_model_evaluate (counts [3 x output_dim] = TP, FP, FN) deciding by thr [n_thr]; prob stays the sigmoid.  Refused with a
 * message: n_thr != output_dim, a NaN threshold, more than one rank, a single-label model.
 * gcnhost_thresholds_read / _write, host only (host/thresholds.h): a text file, one line per class, the first token the threshold
 * as %.9g (exact for every float32), everything from '#' on ignored.  read: *num_classes > 0 on entry = the count the file must
 * hold, 0 = take it from the file; thr may be NULL (for the count).  write: pos .. f (all six, or all NULL) are appended to each
 * line as `# class c pos P neg N tp .. fp .. fn .. f ..`.  A NaN threshold is refused by both. */
int gcnhost_model_tune_thresholds(gcnhost_model *m, int split, const int *nodes, int n, double beta, size_t scratch_bytes, float *thr, int64_t *tp,
                                  int64_t *fp, int64_t *fn, double *f, int64_t *pos, int64_t *neg, int64_t *invalid, int32_t *defined, int64_t *rows);
int gcnhost_model_predict_multilabel_thr(gcnhost_model *m, const int *nodes, int n, const float *thr, int n_thr, uint32_t *bits, float *prob);
int gcnhost_model_evaluate_thr(gcnhost_model *m, int split, const int *nodes, int n, const float *thr, int n_thr, int64_t *counts, int64_t *rows_counted);
/* ---- unseen nodes: new rows attached to a trained graph (host/attach.h, host/queries.h; beyond the reference) ----
 * The dataset has num_nodes = N nodes; a call brings m new ones, new node i has id N + i and the stored row
 * [N + i, nbr_ids[nbr_ptr[i] : nbr_ptr[i + 1]] ...] — the self loop first, then its listed ids in listed order, each in
 * [0, N + m) (N + k: new node k of the same call); repeats, and N + i listed again, count as the loader counts them (degree =
 * stored row length); no existing row changes.  a(v, j) = 1 / sqrt(len(v) . len(j)), the product formed in 64 bits.
 * gcnhost_attach_rows, host only: g_indptr [N + 1] = the dataset's row pointers (its row lengths); out_ptr [m + 1], out_col /
 * out_coef [nbr_ptr[m] + m], out_len [m] (callers allocate).  mode 0: out_coef[e] = a(v, j) as gcnhip_graph_create stores it;
 * mode 1 (the factored model, whose tables carry 1 / sqrt(len) of their own row): out_coef[e] = (float)(1 / sqrt(len(v))).
 * Refused with a message: m < 0, nbr_ptr[0] != 0 or a decreasing nbr_ptr, an id outside [0, N + m), more than 2^31 - 1 stored entries.
 * gcnhost_model_predict_new: the logits of the new rows are what the reference's evaluation forward gives them on the augmented
 * dataset (the dataset nodes' rows as an evaluation forward forms them; the new rows influence no dataset node).  X_new is CSR
 * (x_indptr [m + 1], x_indices, x_values); x_indices == NULL: dense rows of input_dim values.  Single-label model: pred [m],
 * prob [m], logp (may be NULL) [m x output_dim] as gcnhost_model_predict returns them, at the model's temperature; thr must be
 * NULL.  Multi-label model: bits [m x ceil(output_dim / 32)], prob (may be NULL) [m x output_dim] = sigmoid(z), decided by
 * z > 0 or, with thr [n_thr = output_dim], as gcnhost_model_predict_multilabel_thr decides.  Training state is untouched and
 * nothing is cached between calls.  Refused with a message before any launch: what gcnhost_attach_rows refuses, a malformed
 * X_new, more than one rank, bf16 tables, a hidden width above 256, more than 64 (single-label) / 256 (multi-label) classes. */
int gcnhost_attach_rows(int num_nodes, const int *g_indptr, int m, const int64_t *nbr_ptr, const int *nbr_ids, int mode, int32_t *out_ptr,
                        int32_t *out_col, float *out_coef, int32_t *out_len);
int gcnhost_model_predict_new(gcnhost_model *m, const int *x_indptr, const int *x_indices, const float *x_values, int n_new, const int64_t *nbr_ptr,
                              const int *nbr_ids, const float *thr, int n_thr, int32_t *pred, float *prob, float *logp, uint32_t *bits);
/* ---- Monte Carlo dropout (ModelQueries::mc_dropout, host/queries.h; csrc/mcdropout.hip has the definition; beyond the reference) ----
 * Per-node uncertainty from `samples` forwards with dropout on: sample s in [first_sample, first_sample + samples) is the model's
 * training forward with the epoch word s, the rate *p (p == NULL: the model's dropout) and the seed *seed (seed == NULL: the model's
 * seed ^ KEY_MC_DROPOUT; the model's own seed with first_sample = e draws the masks of training epoch e).  Rows as
 * gcnhost_model_evaluate takes them: the nodes of `split` (1 train, 2 validation, 3 test), or with split == 0 the `nodes` query (n
 * dataset ids, repeats allowed; NULL: every row).  *rows = the rows listed.  A call with every array NULL checks the arguments,
 * writes *rows and launches nothing (a split's rows are the model's to count); otherwise capacity must be *rows (samples_logp is
 * laid out by it; capacity >= 1 will do for an empty list).  By list position, each array may be NULL: pred
 * int32 [rows] = argmax of the mean softmax row (lowest class on a tie), confidence = its mean probability, entropy (predictive),
 * expected_entropy, mutual_information = max(0, entropy - expected_entropy), variation_ratio = 1 - (largest vote count) / samples,
 * all f32 [rows] formed in float64 on the device; mean_prob f32 [rows x C]; votes int32 [rows x C]; samples_logp f32 [samples x
 * rows x C] = the per-sample log-softmax rows at the model's temperature.  *seed_used / *p_used: what the samples were drawn with.
 * Training state is untouched (the metrics ring, the current split, the logits, the captured epoch graph, Adam's state, the epoch
 * word, the mask bits).  Refused with a message before any launch: a multi-label model, more than 64 classes, more than one rank,
 * bf16 tables, a hidden width above 256, samples outside 1..1024, p outside [0, 1), first_sample + samples > 2^32, a split outside
 * 0..3, a node id outside the graph. */
int gcnhost_model_mc_dropout(gcnhost_model *m, int split, const int *nodes, int n, int samples, const float *p, const uint64_t *seed, uint64_t first_sample,
                             int64_t capacity, int32_t *pred, float *confidence, float *entropy, float *expected_entropy, float *mutual_information,
                             float *variation_ratio, float *mean_prob, int32_t *votes, float *samples_logp, uint64_t *seed_used, float *p_used,
                             int64_t *rows);
int gcnhost_thresholds_read(const char *path, int *num_classes, float *thr);
int gcnhost_thresholds_write(const char *path, int num_classes, const float *thr, const int64_t *pos, const int64_t *neg, const int64_t *tp,
                             const int64_t *fp, const int64_t *fn, const double *f);
/* Node embeddings (ModelQueries, host/queries.h; kernels in csrc/embed.hip): the hidden matrix H1 = ReLU(A^.X.W1) of one evaluation
 * forward with the current weights (no dropout), as variable 3 stores it (a factored model keeps dinv[r] on row r; cosine scores
 * and normalised rows do not depend on it), queried on the device.  Ids are DATASET node ids.  predict's contract: training state
 * is not touched.  One rank, a hidden width of at most 256, single- or multi-label; metric: 0 = dot product, 1 = cosine.  Refused
 * with a message before any launch: several ranks, a wider hidden layer, k outside 1..64, another metric, a node id outside the graph.
 * gcnhost_model_embed: out [n x hidden] = the rows of the n listed nodes (repeats allowed; nodes == NULL: every node in id
 *   order, out [num_nodes x hidden]), gathered on the device; normalize != 0: each row divided by its norm (a zero row stays zero).
 * gcnhost_model_similar: for each listed node (NULL: every node) the k best nodes by the metric, best first, equal scores by
 *   ascending id, without the node itself when exclude_self != 0: out_id [n x k] int32, out_score [n x k] f32; -1 / -inf where the
 *   graph has fewer candidates.
 * gcnhost_model_score_pairs: out[i] = the score of nodes (src[i], dst[i]). */
int gcnhost_model_embed(gcnhost_model *m, const int *nodes, int n, float *out, int normalize);
int gcnhost_model_similar(gcnhost_model *m, const int *nodes, int n, int k, int metric, int exclude_self, int32_t *out_id, float *out_score);
int gcnhost_model_score_pairs(gcnhost_model *m, const int *src, const int *dst, int n_pairs, int metric, float *out);
/* k-means on the hidden layer (ModelQueries::kmeans, host/queries.h; kernels in csrc/kmeans.hip): the rows gcnhost_model_embed
 * exports, grouped on the device.  Rows: the nodes of `split` (1 train, 2 validation, 3 test) in ascending id, or with split == 0
 * the `nodes` query (n dataset ids in the order given, repeats allowed; NULL: every node in id order).  normalize != 0: unit
 * rows (a factored model's stored row carries 1 / sqrt(deg)); 0: the stored rows.  init: 0 = k-means++ seeding on the stream
 * (*seed, NULL: the model's seed) ^ KEY_KMEANS; 1 = init_pos [k] list positions; 2 = init_centers [k x hidden].  Each of
 * at most `iters` iterations is one assignment and one update; it stops when an assignment moved nothing.  scratch_bytes: the
 * update's device scratch (0: one batch; less: more launches, the same bits).  Outputs, each may be NULL: assign / dist2 (laid out
 * for `capacity` rows, at least the rows listed), centers [k x hidden], sizes [k], seed_pos [k] (init 0), history [iters x 2] =
 * (moved, inertia) per iteration run, contingency [k x num_classes] against the dataset's labels (single-label models, at most
 * 64 classes), info [4] = {rows listed, iterations run, converged, rows the table skipped}, *inertia (the last), *seed_used.
 * embed's contract: training state is not touched.  Refused with a message before any launch: several ranks, a hidden width
 * above 256, bf16 tables, k outside 1..256 or above the rows listed, iters < 1, a bad split, init, position or node id.
 * gcnhost_cluster_report (host/kmeans.h; no GPU): summary [9] = {purity, homogeneity, completeness, V-measure, NMI (arithmetic
 * mean), ARI, H(classes), H(clusters), rows} of a table counts [k x num_classes] in float64; empty rows and columns are
 * allowed, one cluster or one class gives the conventional values, never NaN. */
int gcnhost_model_kmeans(gcnhost_model *m, int k, int split, const int *nodes, int n, int iters, int normalize, int init, const int *init_pos,
                         const float *init_centers, const uint64_t *seed, size_t scratch_bytes, int64_t capacity, int32_t *assign, float *dist2,
                         float *centers, int32_t *sizes, int32_t *seed_pos, double *history, int64_t *contingency, int64_t *info, double *inertia,
                         uint64_t *seed_used);
int gcnhost_cluster_report(int k, int num_classes, const int64_t *counts, double *summary);
/* Silhouette widths of a labelling of the hidden layer (ModelQueries::silhouette, host/queries.h; kernels and definitions in
 * csrc/silhouette.hip): for every listed row a = its mean Euclidean distance to the other points of its label, b = the lowest
 * mean distance to the points of another label, neighbor = that label, s = (b - a) / max(a, b).  Rows as for
 * gcnhost_model_kmeans, a repeat being a point of its own.  labels: int32 by LIST POSITION (what gcnhost_model_kmeans writes as
 * assign for the same arguments); `capacity` is their number and the length the per-row outputs are laid out for: it must
 * equal the rows listed.  A label outside [0, k) takes its position out: s = a = b = NaN, neighbor = -1.  normalize as for
 * gcnhost_model_kmeans.  scratch_bytes: the cap on the sums' device scratch (0: 256 MiB; less: more launches, the same bits).
 * Outputs, each may be NULL: s / a / b float64 [capacity], neighbor int32 [capacity], cluster_mean float64 [k] (0 for an empty
 * label), sizes int32 [k], info [5] = {rows listed, points, excluded, non-empty labels, defined (at least two of them)},
 * *score = the mean of s over the points.  With fewer than two non-empty labels every s is 0 and every neighbor -1; nothing is
 * NaN or inf for a point.  embed's contract: training state is not touched, nothing is cached.  Refused with a message before
 * any launch: several ranks, bf16 tables, a hidden width above 256, k outside 1..256, a bad split or node id, labels of
 * another length than the list. */
int gcnhost_model_silhouette(gcnhost_model *m, int split, const int *nodes, int n, const int32_t *labels, int k, int normalize, size_t scratch_bytes,
                             int64_t capacity, double *s, double *a, double *b, int32_t *neighbor, double *cluster_mean, int32_t *sizes,
                             int64_t *info, double *score);
/* Principal components of the hidden layer (ModelQueries::pca_fit / pca_project, host/queries.h; sums in csrc/pca.hip; the
 * eigenproblem in host/pca.h).  Rows as for gcnhost_model_kmeans, repeats counted as often as listed.
 * gcnhost_sym_eigen (no GPU): S [h x h] float64, 1 <= h <= 256, finite and symmetric bit for bit (else -1 with a message);
 *   lambda [h] descending; V [h x h], V[a * h + j] = entry a of the unit vector of lambda[j], its entry of largest magnitude positive
 *   (the lowest index on equal magnitude).  Cyclic Jacobi.
 * gcnhost_pca_from_scatter (no GPU): from the scatter matrix of `rows` >= 2 centred rows — eigenvalues [h] = max(lambda, 0)
 *   descending, components [h x h] with ROW j = component j, explained [3 x h] = {lambda / (rows - 1) | lambda_j / sum(lambda), 0
 *   when the sum is 0 | sqrt(lambda)}, *rank = the number of lambda_j > h . 2^-52 . lambda_1, and with whiten != 0 scale [k] =
 *   1 / sqrt(lambda_j / (rows - 1)), 0 past the rank.  Never NaN or inf.  mean (may be NULL) is checked to be finite.  Each
 *   output may be NULL.
 * gcnhost_model_pca_fit: one evaluation forward, with center != 0 the float64 mean, the float64 scatter matrix on the device,
 *   h + h . h doubles to the host, the eigenproblem there, and with coords the projection of the listed rows onto the leading k
 *   components on the device: coords [rows x k] f32 (laid out for `capacity` rows, at least the rows listed).  mean [h] (zeros without center), scatter [h x h], eigenvalues, components,
 *   explained, scale as above, each may be NULL; info [3] = {rows, rank, k}.  scratch_bytes: the sums' device scratch (0: one
 *   launch; less: more launches, the same bits).
 * gcnhost_model_pca_project: a fit's arrays (width, k, mean [width] or NULL, components [k x width] rows, scale [k] or NULL)
 *   applied to the `nodes` query (NULL: every node) at the current weights: out [n x k].  Nothing is cached.
 * embed's contract: training state is not touched.  Refused with a message before any launch: several ranks, bf16 tables, a
 * hidden width above 256, k outside 1..hidden, fewer than 2 rows listed, a bad split or node id, a fit of another width or one
 * that is not finite. */
int gcnhost_sym_eigen(const double *S, int h, double *lambda, double *V);
int gcnhost_pca_from_scatter(const double *S, const double *mean, int64_t rows, int h, int k, int whiten, double *eigenvalues, double *components,
                             double *explained, double *scale, int *rank);
int gcnhost_model_pca_fit(gcnhost_model *m, int k, int split, const int *nodes, int n, int normalize, int center, int whiten, size_t scratch_bytes,
                          int64_t capacity, double *mean, double *scatter, double *eigenvalues, double *components, double *explained, double *scale,
                          float *coords, int64_t *info);
int gcnhost_model_pca_project(gcnhost_model *m, int width, int k, const double *mean, const double *components, const double *scale, int normalize,
                              const int *nodes, int n, float *out);
/* Label structure of the graph (ModelQueries::neighbor_agreement / structure, host/queries.h; kernels and definitions in
 * csrc/structure.hip; measures in host/structure.h).  Arrays are in DATASET node order.  Rows: the nodes of `split` (1 train,
 * 2 validation, 3 test) in ascending id, or with split == 0 the `nodes` query (n dataset ids in the order given, repeats counted
 * as often as listed; NULL: every node in id order).
 * gcnhost_model_neighbor_agreement: labels int32 [n_labels = num_nodes], any labelling with x known when 0 <= x < num_classes <= 64;
 *   no weights, no forward, single- and multi-label models alike.  deg / same / known (each may be NULL; laid out for `capacity`
 *   rows, at least the rows listed) by list position, mix [C x C] (may be NULL), class_rows [C], totals [8] (int64; the kernel
 *   file lists them), info [2] = {rows listed, positions outside the adjacency}.
 * gcnhost_model_structure: the agreement of the dataset's labels (deg / same / known, mix_truth, class_rows_truth, totals_truth)
 *   and, with predicted != 0, one evaluation forward, the agreement of the predicted classes (mix_pred, class_rows_pred,
 *   totals_pred) and strata [32 x (bins + 1) x 2] = (rows, rows predicted right) by degree bucket and by the bucket of the
 *   TRUTH's agreement; info [3] = {rows listed, positions outside the adjacency, listed rows without a label}.  C is the model's.
 * predict's contract: training state is not touched.  Refused with a message before any launch: several ranks, more than 64
 * classes, bins outside 1..32, a bad split or node id, a label array of another length, and with predicted a multi-label model.
 * gcnhost_structure_metrics (host/structure.h; no GPU): from mix [C x C], class_rows [C], totals [8] (may be NULL) — summary [8] =
 *   {edge_homophily, node_homophily, adjusted_homophily, class_insensitive_homophily, edges, rows with a labelled neighbour,
 *   labelled rows, strata rows}, class_homophily [C], compatibility [C x C]; from strata (may be NULL, then bins is ignored) —
 *   by_degree [32 x 5] and by_agreement [(bins + 1) x 5], rows of {lo, hi, rows, correct, accuracy}.  Each output may be NULL.
 *   A zero denominator gives 0, never NaN; a negative count is an error.
 * gcnhost_structure_write / _read: the text report gcn-hip writes for GCN_STRUCTURE (the integers, and derived from them the
 *   metrics and the two tables).  The reader's arrays are laid out for 64 classes and 32 bins. */
int gcnhost_model_neighbor_agreement(gcnhost_model *m, const int32_t *labels, int64_t n_labels, int num_classes, int split, const int *nodes, int n,
                                     int64_t capacity, int32_t *deg, int32_t *same, int32_t *known, int64_t *mix, int64_t *class_rows, int64_t *totals,
                                     int64_t *info);
int gcnhost_model_structure(gcnhost_model *m, int split, const int *nodes, int n, int bins, int predicted, int64_t capacity, int32_t *deg, int32_t *same,
                            int32_t *known, int64_t *mix_truth, int64_t *class_rows_truth, int64_t *totals_truth, int64_t *mix_pred,
                            int64_t *class_rows_pred, int64_t *totals_pred, int64_t *strata, int64_t *info);
int gcnhost_structure_metrics(int num_classes, const int64_t *mix, const int64_t *class_rows, const int64_t *totals, int bins, const int64_t *strata,
                              double *summary, double *class_homophily, double *compatibility, double *by_degree, double *by_agreement);
int gcnhost_structure_write(const char *path, int num_classes, int bins, const int64_t *totals_truth, const int64_t *totals_pred,
                            const int64_t *class_rows_truth, const int64_t *class_rows_pred, const int64_t *mix_truth, const int64_t *mix_pred,
                            const int64_t *strata);
int gcnhost_structure_read(const char *path, int *num_classes, int *bins, int64_t *totals_truth, int64_t *totals_pred, int64_t *class_rows_truth,
                           int64_t *class_rows_pred, int64_t *mix_truth, int64_t *mix_pred, int64_t *strata);
/* Reach of the labels (ModelQueries::label_distance / components / reach, host/queries.h; kernels and definitions in
 * csrc/reach.hip; measures in host/reach.h).  Arrays are in DATASET node order.  Rows: the nodes of `split` (1 train, 2 validation,
 * 3 test) in ascending id, or with split == 0 the `nodes` query (n dataset ids in the order given, repeats counted as often as
 * listed; NULL: every node in id order).  Sources (the marks of components): the nodes of the splits in source_mask (bit s = split
 * s; 2 = the training split), or with source_mask == 0 the n_sources ids of source_nodes.  One rank; single- and multi-label
 * models alike (gcnhost_model_reach with predicted != 0: single-label only).  Per-position arrays are laid out for `capacity`
 * rows, at least the rows listed; each may be NULL.  nearest and component are dataset ids; a tie between sources at the same
 * distance goes to the lowest local row (the dataset id unless the model was given a node order).
 * gcnhost_model_label_distance: dist / nearest [rows] (nearest NULL: not computed), level_counts [level_capacity] (rows per
 *   distance, zero past the last level), info [5] = {rows listed, rows that became sources, source positions outside the graph,
 *   listed rows no source reaches (within max_hops; 0: no limit), levels}.
 * gcnhost_model_components: component / size [rows] = the smallest node of the row's weak component and its number of nodes,
 *   totals [6] = {rows, components, largest, components without a source, rows in those, source rows}, info [2] = {rows listed,
 *   rounds}.
 * gcnhost_model_reach: with predicted != 0 one evaluation forward; the traversal; the components; strata [(hops + 2) x 4] = per
 *   distance bucket (b < hops: distance b; hops: further; hops + 1: unreachable) {rows, labelled, predicted right, nearest
 *   source has the row's label}; totals [6]; level_counts; info [7] = {rows listed, sources, skipped, listed rows without a
 *   label, listed rows unreachable, levels, rounds}.
 * predict's contract: training state is not touched.  Refused with a message before any launch: several ranks, a bad split, source
 * mask or node id, max_hops < 0, hops outside 1..32, and with predicted a multi-label model.
 * gcnhost_reach_metrics (host/reach.h; no GPU): by_distance [(hops + 2) x 6] and groups [3 x 6] (inside the receptive field =
 *   buckets 0 .. layers, outside it, all), rows of {rows, labelled, correct, nearest_correct, accuracy, nearest_label_accuracy};
 *   summary [2] = {unreachable, unreachable share}.  0 <= layers < hops.  Each output may be NULL.  A zero denominator gives 0,
 *   never NaN; a negative or inconsistent count is an error.
 * gcnhost_reach_write / _read: the text report gcn-hip writes for GCN_REACH; info [3] = {sources, unlabelled, rounds}; the reader
 *   copies at most level_capacity level counts and tells their number in *n_levels. */
int gcnhost_model_label_distance(gcnhost_model *m, int source_mask, const int *source_nodes, int n_sources, int split, const int *nodes, int n,
                                 int max_hops, int64_t capacity, int32_t *dist, int32_t *nearest, int64_t *level_counts, int level_capacity,
                                 int64_t *info);
int gcnhost_model_components(gcnhost_model *m, int split, const int *nodes, int n, int source_mask, const int *source_nodes, int n_sources,
                             int64_t capacity, int32_t *component, int32_t *size, int64_t *totals, int64_t *info);
int gcnhost_model_reach(gcnhost_model *m, int split, const int *nodes, int n, int source_mask, const int *source_nodes, int n_sources, int hops,
                        int predicted, int64_t capacity, int32_t *dist, int32_t *nearest, int32_t *component, int64_t *strata, int64_t *totals,
                        int64_t *level_counts, int level_capacity, int64_t *info);
int gcnhost_reach_metrics(const int64_t *strata, int hops, int layers, double *by_distance, double *groups, double *summary);
int gcnhost_reach_write(const char *path, int hops, int layers, const int64_t *info, const int64_t *totals, const int64_t *level_counts,
                        int64_t n_levels, const int64_t *strata);
int gcnhost_reach_read(const char *path, int *hops, int *layers, int64_t *info, int64_t *totals, int64_t *level_counts, int64_t level_capacity,
                       int64_t *n_levels, int64_t *strata);
/* Explaining a logit (ModelQueries::explain / feature_importance, host/queries.h; kernels in csrc/explain.hip).  The network is
 * Z = A^ . (ReLU(A^ . X . W1) . W2) without bias: with the ReLU gates of a forward fixed, the logit of (node, class) is a plain sum
 * that splits exactly by the neighbour a term came through (one share per stored edge of the node's row, self loop included, a
 * repeated edge twice), by hidden unit [hidden] and by input feature column [F]; each split adds up to the logit (the feature
 * shares up to the first layer's own rounding).  Ids are DATASET node ids.  embed's contract: training state is not touched.
 * classes == NULL: each node's highest logit, lowest class on a tie.  feat_scratch_bytes: device scratch of the feature shares
 * (0: 64 MiB, the most it may be); larger queries run in batches with the same bits.  Refused with a message before any launch:
 * several ranks, a hidden width above 256, bf16 tables, a node id or class out of range; for the importance more than 256 classes
 * or a split without rows.
 * gcnhost_model_explain: a first call with nbr_ids == NULL writes only *nbr_total, the length of the neighbour lists of the query
 *   (as gcnhost_local_graph reports its sizes).  The second call fills out_class [n], logit [n], hidden [n x hidden], feat [n x F]
 *   (NULL: not computed), nbr_ptr [n + 1], nbr_ids / nbr_values [nbr_total]: the shares of query i are entries nbr_ptr[i] ..
 *   nbr_ptr[i + 1] - 1, in the stored order of the row.  nodes == NULL: every node in id order (n = num_nodes).
 * gcnhost_model_feature_importance: mean_abs [C x F] float64 = the mean of |feature share| over the nodes of `split` (1 train,
 *   2 validation, 3 test; 0: the `nodes` query) explained for their default class, per explained class; count [C] the nodes. */
int gcnhost_model_explain(gcnhost_model *m, const int *nodes, const int *classes, int n, size_t feat_scratch_bytes, int32_t *out_class,
                          float *logit, float *hidden, float *feat, int64_t *nbr_ptr, int32_t *nbr_ids, float *nbr_values, int64_t *nbr_total);
int gcnhost_model_feature_importance(gcnhost_model *m, int split, const int *nodes, int n, size_t feat_scratch_bytes, double *mean_abs,
                                     int64_t *count);
/* Per-class metrics from integer counts, host only (host/report.h): either confusion [C x C] (row = truth, column =
 * prediction) or tp / fp / fn [C] (the other form NULL).  Every output may be NULL: tp_fp_fn [3 x C] the counts used; support
 * (TP + FN), precision = TP / (TP + FP), recall = TP / (TP + FN), f1 = 2 TP / (2 TP + FP + FN) [C], float64, each 0 when
 * its denominator is 0; summary [3] = {macro_f1 (mean of f1 over all C classes), micro_f1 = 2 sum TP / (2 sum TP + sum FP +
 * sum FN), accuracy = trace / sum of the matrix (0 from vectors)}.  A negative count or C < 1 is an error. */
int gcnhost_class_report(int num_classes, const int64_t *confusion, const int64_t *tp, const int64_t *fp, const int64_t *fn,
                         int64_t *tp_fp_fn, double *support, double *precision, double *recall, double *f1, double *summary);
/* The multi-label truth file (host/labels.h), host only: one line per node, comma-separated class ids, empty for none.
 * *num_nodes > 0: the file must have that many lines; *num_classes > 0: every id must be below it (else C = largest id + 1).
 * Both receive the values used.  bits (may be NULL: check and report the sizes only) [num_nodes x ceil(C / 32)].  A wrong
 * line count, a bad token or a negative id is an error with a message naming the line. */
int gcnhost_labels_read(const char *path, int *num_nodes, int *num_classes, uint32_t *bits);
/* The weights file: "GCNW", format version, input / hidden / output widths (int32), W1 [F x h], W2 [h x C] (f32 row-major),
 * CRC-32; little-endian (host/weights.h).  save writes this model's W1, W2 (several ranks hold the same weights: one of them
 * writes).  load refuses a file whose widths differ from the model's (an error with a message, never a reshape) and goes
 * through gcnhost_model_set_weights.  Adam's moments and step count are not in the file: a loaded model that trains further
 * starts Adam afresh. */
int gcnhost_model_save_weights(gcnhost_model *m, const char *path);
int gcnhost_model_load_weights(gcnhost_model *m, const char *path);
/* the same file from the host alone (no GPU).  read: w1 == w2 == NULL reports the file's widths; otherwise the widths passed
 * in are those of the caller's buffers and must equal the file's.  A truncated or damaged file, a wrong magic or version is
 * an error (gcnhost_last_error). */
int gcnhost_weights_write(const char *path, int input_dim, int hidden_dim, int output_dim, const float *w1, const float *w2);
int gcnhost_weights_read(const char *path, int *input_dim, int *hidden_dim, int *output_dim, float *w1, float *w2);
/* device-event timer `id` (host/timer.h, ids of src/common/timer.h:5-20 plus 13 Adam, 14 comm,
 * 15 GraphSum at the hidden width): accumulated seconds and number of intervals */
int gcnhost_model_timer(gcnhost_model *m, int id, double *seconds, long *count);
int gcnhost_model_timers_reset(gcnhost_model *m);
/* switch the per-op timers on/off after construction (synchronises).  While on, run_epochs runs eagerly instead
 * of replaying its captured hipGraph: time the headline with them off, collect the breakdown in a separate pass */
int gcnhost_model_set_timers(gcnhost_model *m, int on);

/* the text loader (src/common/parser.cpp) — fills caller-visible arrays owned by the returned handle */
typedef struct gcnhost_dataset gcnhost_dataset;
int gcnhost_dataset_load(gcnhost_dataset **d, const char *root, const char *name, gcnhost_params *p);
int gcnhost_dataset_arrays(gcnhost_dataset *d, const int **g_indptr, const int **g_indices, int64_t *g_nnz,
                           const int **f_indptr, const int **f_indices, const float **f_val, int64_t *f_nnz,
                           const int **split, int64_t *n_split, const int **label, int64_t *n_label);
int gcnhost_dataset_save_binary(gcnhost_dataset *d, const gcnhost_params *p, const char *path);
int gcnhost_dataset_free(gcnhost_dataset *d);

/* one-rank RCCL round trip on `device` (communicator init, in-place all-gather, all-reduce,
 * destroy): checks that the RCCL this process loaded works before a multi-GPU job relies on it */
int gcnhost_rccl_selftest(int device);
/* the same with `world` ranks, one process per rank, all given the id rank 0 got from gcnhost_nccl_unique_id:
 * in-place all-gather of distinct blocks, all-reduce, the halo exchange (an ExchangePlan's send lists moved by grouped
 * ncclSend/ncclRecv, every table row checked), split communicator, alternating lanes — values checked */
int gcnhost_rccl_selftest_world(int device, int rank, int world, const char *nccl_id);
/* device time (microseconds, HIP events) per in-place all-gather of block_floats floats per rank and per all-reduce of
 * reduce_floats floats, back to back on the stream; with world == 1 the launch + kernel floor of a collective */
int gcnhost_rccl_collective_us(int device, int rank, int world, const char *nccl_id, long block_floats, long reduce_floats, int iters,
                               double *us_allgather, double *us_allreduce);
/* the halo round trip of that self-test through the host-staged transport (the callbacks of gcnhost_model_create) */
int gcnhost_halo_selftest_host(int device, int rank, int world, gcnhost_allgather_fn host_allgather,
                               gcnhost_allreduce_fn host_allreduce, void *host_user);

/* host-only helpers, callable without a GPU (CPU tests) */
int gcnhost_partition(const int *g_indptr, int n_rows, int world, int *start /* [world+1] */, int *rows_max);
/* rank's row block with columns rewritten to padded all-gather positions (what HipGCN feeds to
 * gcnhip_graph_create when world > 1).  Call once with NULL arrays for the sizes. */
int gcnhost_local_graph(const int *g_indptr, const int *g_indices, int n_rows, int world, int rank,
                        int *indptr, int *indices, int *col_deg, int *n_local, int *n_cols, int64_t *nnz_local);
/* How rank `rank` of `world` completes the tables an aggregation gathers from (host/partition.h): mode 0 decides
 * per graph between an all-gather of whole row blocks and a halo exchange of only the rows some local edge points
 * at (1 / 2 force one).  Gives the table layout, the per-peer send and receive lists and the rank's row block of the
 * adjacency with its columns rewritten to table rows — what HipGCN hands to gcnhip_graph_create.  Host only. */
typedef struct gcnhost_plan gcnhost_plan;
int gcnhost_plan_create(gcnhost_plan **p, const int *g_indptr, const int *g_indices, int n_rows, int world, int rank, int mode);
int gcnhost_plan_info(const gcnhost_plan *p, int *halo, int *n_local, int *table_rows, int *own_offset, int *rows_max,
                      double *halo_share, int64_t *nnz_local, int64_t *n_recv, int64_t *n_send);
/* recv_off/send_off: [world+1]; recv_rows: peer-local row ids per segment; send_rows: local row ids per destination;
 * table_global: [table_rows] global node id (-1 = padding); indptr/indices/col_deg: the local adjacency */
int gcnhost_plan_arrays(const gcnhost_plan *p, const int **recv_off, const int **recv_rows, const int **send_off, const int **send_rows,
                        const int **table_global, const int **indptr, const int **indices, const int **col_deg);
int gcnhost_plan_free(gcnhost_plan *p);
int gcnhost_glorot(float *w, int size, int in_size, int out_size, long seed, int skip_draws);
int gcnhost_host_masks(uint8_t *keep, int64_t n, float p, long seed, int64_t skip_draws);
/* Graph500 R-MAT graph (a,b,c = .57,.19,.19) of 2^scale nodes and edge_factor * 2^scale sampled pairs, symmetrised,
 * duplicates and self pairs dropped, in the layout the reference's loader produces (src/common/parser.cpp:20-46:
 * CSR with the self loop first, neighbours ascending).  BASELINE configs[4] = scale 22, edge_factor 16.  The arrays
 * are malloc'ed here; release them with gcnhost_free_array.  Deterministic in (scale, edge_factor, seed). */
int gcnhost_rmat_graph(int scale, int edge_factor, uint64_t seed, int **indptr, int **indices, int64_t *nnz);
void gcnhost_free_array(void *p);
/* The node order a `world`-rank model would renumber the dataset with (host/partition.h, choose_node_order): order[new] =
 * old (identity when the ids are kept), and the rows the neediest rank receives per exchange under the ids and under the
 * chosen order, next to what the padded all-gather moves.  Host only. */
int gcnhost_choose_node_order(const int *g_indptr, const int *g_indices, int n_rows, int world, int force, int *order, int *renumbered,
                              double *ids_share, int64_t *ids_recv_rows, double *new_share, int64_t *new_recv_rows, int64_t *allgather_rows);
/* Row groups for the aggregation's schedule found in the graph itself (Louvain local moving from singletons with a size
 * bound, asynchronous in a fixed node order, host/cluster.h): group[i] in 0 .. *n_groups-1, largest group first.  *useful == 0: the graph has no such
 * structure (everything collapsed into one group, or nothing merged) and HipGCN would not try the grouping.  What
 * HipGCN runs when the labels are not assortative on the graph (or GCNHOST_NO_LABEL_HINT is set); deterministic. */
int gcnhost_structure_groups(const int *g_indptr, const int *g_indices, int n_rows, int *group, int *n_groups, int *sweeps,
                             double *largest_share, int *useful);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
