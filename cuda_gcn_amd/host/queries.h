// queries.h — what a caller asks of a trained model (beyond the reference, which only prints accuracy): prediction, per-class
// evaluation, label propagation and Correct & Smooth, temperature scaling, node embeddings, explanations, conformal prediction
// sets, ranking metrics, multi-label decision thresholds, prediction for nodes the dataset did not hold, Monte Carlo dropout, k-means on the embeddings, the label structure of the graph, the reach of the labels.  ModelQueries owns every device buffer and every piece of host state these calls need, in an arena of its own on the model's main context: nothing is allocated until the
// first query, and HipGCN::release() frees all of it by destroying this one object.
//
// It holds a HipGCN & and is a friend of it.  What it uses, and all it uses:
//   reads   params, opt_.multilabel, env (context, comm), n_local, row_start(), node_order_ (query_rows' inverse map; node_id()
//           elsewhere), data->split, data->label, graph, logits_gs (null test only), variables[6]->ld, d_truth[], split_rows[],
//           d_split_list[], split_local_n[], split_count[], d_ml_truth, ml_wpr, variables[3] (data, ld), node_id(), and for
//           explanations variables[2] / [5] (data, ld), factored_, flags, feat, feat_agg, eval_modules[0]->hidden_not_stored; for
//           predict_new also variables[1] / [4] (data, ld), eval_modules.empty(), env.seed, env.d_epoch; for mc_dropout
//           params.dropout, env.seed, feat, graph, factored_, flags, variables[1] / [3] / [4] (ld only), variables[2] / [5]
//   calls   sync(), forward_hooked(), forward_hidden_only(), forward_class_products()
// It writes no member of HipGCN.  One object it reads is changed by a query all the same: mc_dropout's stochastic gcnhip_spmm_fwd
// redraws the dropout-bit array of the feature object (and its layout flag), which the training backward reads.  That is harmless
// only because every training pass runs its own forward — which draws them again — before its backward; a query is made between
// passes (sync() first), never between a forward and its backward (tests/test_mc_dropout_gpu.py, "between epochs").
#pragma once
#include <cstdint>
#include <functional>
#include <vector>
#include "device_arena.h"

class HipGCN;

class ModelQueries {
public:
    explicit ModelQueries(HipGCN &model);
    ~ModelQueries() { arena.free_all(); }

    // Prediction: an evaluation forward with the current weights — no dropout, the model's usual evaluation order
    // (aggregate-first when that is on) — whose logit aggregation carries the prediction epilogue (gcnhip_graphsum_predict) on
    // the requested rows.  nodes: n DATASET node ids, each a row of this rank (repeats allowed); NULL: every row of this rank, in
    // the order of local rows (HipGCN::node_id() names them).  pred[i] = argmax of node i's logits (lowest class on a tie),
    // prob[i] = its softmax probability, logp (may be NULL) [n x C] = the log-softmax rows.  Several GPUs: a collective (the
    // logit aggregation's exchange) — every rank calls it, each with its own nodes.  Training state is not touched: the metrics
    // ring, the current split, the logits (variable 6) and the captured epoch graph are left as they were; a train_epoch()
    // after it has the same bits as one without it.  Synchronises.
    void predict(const int *nodes, int n, int32_t *pred, float *prob, float *logp);
    // Multi-label prediction, the same contract as predict() (dataset ids, NULL = every row of this rank, a collective, training
    // state untouched, synchronises): one evaluation forward whose logits go to scratch (not variable 6), then
    // gcnhip_bce_predict_rows.  bits [n x ceil(C / 32)]: bit (c & 31) of word c >> 5 = (z_c > 0); prob (may be NULL) [n x C] =
    // sigmoid(z).  Only on a multi-label model (predict() only on a single-label one).
    void predict_multilabel(const int *nodes, int n, uint32_t *bits, float *prob);
    // The same call deciding by one cut per class (tune_thresholds below; csrc/thresholds.hip has the rule): thr [n_thr], bit c =
    // (z_c is not NaN and z_c >= thr[c], compared on the integer keys), gcnhip_bce_predict_rows_thr; prob stays sigmoid(z).
    // Refused with a message before any launch: n_thr != C, a NaN threshold, more than one rank, more than 256 classes.
    void predict_multilabel(const int *nodes, int n, const float *thr, int n_thr, uint32_t *bits, float *prob);
    // Per-class evaluation: one evaluation forward with the current weights (no dropout) over a set of rows, and integer counts
    // per class formed on the GPU behind it.  Rows: the nodes of `split` (1 train, 2 validation, 3 test — eval's codes) on this
    // rank, `nodes` then ignored; or, with split == 0, the `nodes` query with predict()'s conventions (n dataset ids, each a row
    // of this rank, repeats counted as often as listed; NULL: every row of this rank).
    // Single-label model: the logit aggregation runs gcnhip_graphsum_predict on those rows only, then gcnhip_confusion_rows;
    // counts [C x C], counts[t * C + p] = rows with truth t predicted as p; *unlabelled = rows whose truth is outside [0, C)
    // (not in the matrix), *rows_counted = rows in the matrix.  Multi-label model: predict_multilabel's forward (logits to
    // scratch), then gcnhip_bce_class_counts_rows; counts [3 x C] = TP, FP, FN per class (z > 0 predicts the class),
    // *rows_counted = the rows, *unlabelled = 0.  Several GPUs: a collective like predict(); each rank counts its own rows, the
    // counts are summed exactly over the ranks and every rank returns the same totals.  Only the counts cross to the host.
    // Training state is not touched, as with predict().  Synchronises.  More than 64 (single-label) or 256 (multi-label)
    // classes: an error.  host/report.h derives precision / recall / F1 from the counts.
    void evaluate(int split, const int *nodes, int n, int64_t *counts, int64_t *rows_counted, int64_t *unlabelled);
    // evaluate() of a multi-label model with one cut per class in place of z > 0 (gcnhip_bce_class_counts_rows_thr): counts
    // [3 x C] = TP, FP, FN.  Refused as predict_multilabel with thresholds is, and on a single-label model.
    void evaluate(int split, const int *nodes, int n, const float *thr, int n_thr, int64_t *counts, int64_t *rows_counted);
    // Label propagation and Correct & Smooth (Huang et al., 2020): the graph and the known labels used at inference time.  Every
    // iteration is one gcnhip_graphsum_blend launch through the model's adjacency with its per-edge coefficients, ping-ponging
    // two of four [local rows x ld] f32 tables (allocated on first use; ld by the row rule of variable 6).  Arrays are in
    // DATASET node order.  predict()'s contract: the call starts with sync(); the metrics ring, the current split, variable 6
    // and the captured epoch graph are untouched.  Refused with a message before any launch: more than one rank (every
    // iteration would need a table exchange), alpha outside [0, 1], iters < 0, a width outside 1..64, and for the two label
    // schemes a multi-label model or more than 64 classes.  splits_mask: bit s = the labelled nodes of split s are known
    // (2 = the training split).
    //   propagate: Y_{k+1} = clamp(alpha . A^ . Y_k + (1 - alpha) . y0, lo, hi), Y_0 = y0 [num_nodes x dim]; out = Y_iters, pred
    //   (may be NULL) its row argmax (lowest column on a tie).  Needs neither labels nor trained weights.
    //   label_propagation: propagate from the one-hot rows of the known nodes (zero rows elsewhere), clamp [0, 1].
    //   correct_and_smooth: one hooked evaluation forward leaves the log-softmax rows on the device; gcnhip_cs_error_rows,
    //   iters_correct blends clamped to [-1, 1], gcnhip_cs_correct_rows, iters_smooth blends clamped to [0, 1], the last of which
    //   writes pred — the only array that must cross to the host; g (may be NULL) is copied when asked for.
    void propagate(const float *y0, int dim, float alpha, int iters, float lo, float hi, float *out, int32_t *pred);
    void label_propagation(float alpha, int iters, int splits_mask, int32_t *pred, float *y);
    void correct_and_smooth(float alpha_correct, int iters_correct, float alpha_smooth, int iters_smooth, int splits_mask, int32_t *pred, float *g);
    // Temperature scaling and calibration error (Guo et al., 2017): are predict()'s probabilities to be trusted, and one scalar T
    // that repairs them — softmax(z / T) with T fitted on a held-out split.  All three work on the log-softmax rows predict()'s
    // hooked forward leaves on the device (log_softmax(z / T) = log_softmax(log_softmax(z) / T)) with the row-local kernels of
    // csrc/calib.hip, and hold predict()'s contract: the call starts with sync(); the metrics ring, the current split,
    // variable 6 and the captured epoch graph are untouched.  Rows: the labelled nodes of `split` (1 train, 2 validation,
    // 3 test), or with split == 0 the `nodes` query scored against the dataset's labels, as evaluate() takes them.
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
    //   within the 40 steps); stops when |delta beta| <= 1e-6 beta or after 40 steps.  at_bound: the result sits on an end of
    //   [0.01, 100] (a split the model classifies perfectly: the NLL falls in beta without end).  With bins > 0 the reliability
    //   counts of the same rows at T = 1 and at the fitted T are formed by two more launches on the rows already there:
    //   count / correct / conf_sum [2 x bins].  calibrate does not set the temperature.
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
    // Node embeddings: the hidden matrix H1 = ReLU(A^.X.W1) of an evaluation forward with the current weights (no dropout), as
    // variable 3 stores it — on a factored model (HipGCN::factored()) row r carries the factor dinv[r], which cosine scores and
    // normalised rows do not see — queried where it lies.  The csrc/embed.hip kernels do the work; ids are DATASET node ids
    // everywhere, and ties of similar() are broken by dataset id (row_id = node_id()).  predict()'s contract: the call starts
    // with sync(); the metrics ring, the current split, variable 6 and the captured epoch graph are untouched; variable 3 is
    // rewritten, as by every forward, and h1_from_fused_eval stays truthful.  Single- and multi-label models alike.  Every call
    // recomputes the hidden layer (an aggregate-first model: its one product, HipGCN::forward_hidden_only; else a whole hooked
    // forward with the logits redirected to scratch) and the norms: nothing is cached, so nothing can go stale when weights
    // change.  Refused with a message before any launch: more than one rank (the table would need an exchange), a hidden width
    // above 256, k outside 1..64, a metric other than METRIC_DOT / METRIC_COSINE, a node id outside the graph.
    //   embed: out [n x hidden] = the rows of `nodes` (n dataset ids, repeats allowed; NULL: every node in id order, n ignored),
    //   gathered on the device so that only n x hidden floats cross; normalize: each row times 1 / its norm (a zero row stays zero).
    //   similar: per queried node (NULL: every node) the k best nodes of the graph by METRIC_DOT (the f32 dot product) or
    //   METRIC_COSINE, best first, equal scores by ascending id, without the node itself when exclude_self: out_id / out_score
    //   [n x k]; slots past the candidates hold -1 / -inf.  The per-chunk lists go through a scratch block of at most 64 MiB:
    //   more queries than it holds are answered in batches.
    //   score_pairs: out[i] = the score of nodes (src[i], dst[i]); src[i] == dst[i] is allowed.
    enum Metric { METRIC_DOT = 0, METRIC_COSINE = 1 };
    void embed(const int *nodes, int n, float *out, bool normalize);
    void similar(const int *nodes, int n, int k, int metric, bool exclude_self, int32_t *out_id, float *out_score);
    void score_pairs(const int *src, const int *dst, int n_pairs, int metric, float *out);
    // Explaining a logit: the network is Z = A^ . (ReLU(A^ . X . W1) . W2) without bias, so with the ReLU gates of a forward fixed
    // the logit of (node v, class c) is a plain sum, split here without approximation by the neighbour a term came through, by
    // hidden unit and by input feature column (csrc/explain.hip; include/gcnhip_driver.h has the formulas).  embed()'s contract:
    // the call starts with sync(); the hidden layer is recomputed through embed_forward with nothing cached; the metrics ring, the
    // current split, variable 6 and the captured epoch graph are untouched; variable 3 is rewritten, as by every forward.  The
    // gates are variable 3's own (H1 > 0), the results the reference's quantities on factored and HIPGCN_EDGE_COEF models alike.
    // Ids are DATASET node ids, also those of the neighbours.  classes == NULL: the explained class of a node is its highest
    // logit, lowest class on a tie (single- and multi-label), taken from the logits of the query's own forward (the evaluation
    // forward with its logits redirected to scratch; an aggregate-first model whose fused launch keeps the hidden layer in
    // registers then stores it by its one product).  The features path is gcnhip_explain_features_agg when the model has A^.X
    // (feat_agg), else gcnhip_explain_features_walk on its feature object; its scratch is feat_scratch_bytes (0: 64 MiB) at most,
    // larger queries run in batches and give the same bits.  Refused with a message before any launch: more than one rank, a
    // hidden width above 256, bf16 tables, a node id or class out of range; for feature_importance more than 256 classes or a
    // split without rows.
    //   explain: n queries (nodes NULL: every node in id order).  explain_size tells the length of the neighbour lists (the sum
    //   of the queried rows' stored lengths, self loops and repeated edges included) without touching the device beyond one
    //   copy of the row pointers.  out_class [n], logit [n], hidden [n x h], feat [n x F] (NULL: not computed), nbr_ptr [n + 1],
    //   nbr_ids / nbr_values [nbr_ptr[n]]: the stored edges of the node's row in stored order.
    //   feature_importance: over the nodes of `split` (1..3), or with split == 0 the `nodes` query, each explained for its
    //   default class: mean_abs [C x F] = the mean of |feat| per explained class (float64, accumulated on the device in query
    //   order; a class without nodes: zeros), count [C].
    int64_t explain_size(const int *nodes, int n);
    void explain(const int *nodes, const int *classes, int n, size_t feat_scratch_bytes, int32_t *out_class, float *logit, float *hidden, float *feat,
                 int64_t *nbr_ptr, int32_t *nbr_ids, float *nbr_values);
    void feature_importance(int split, const int *nodes, int n, size_t feat_scratch_bytes, double *mean_abs, int64_t *count);
    // Split conformal prediction (LAC: Sadinle et al., 2019; APS / RAPS: Romano et al., 2020, Angelopoulos et al., 2021; the
    // neighbourhood diffusion of the scores: Zargarbashi et al., 2023): calibration says whether the probabilities can be trusted
    // on average, this gives a guarantee per node — a SET of classes that holds the true one with probability >= 1 - alpha,
    // whatever the model, from one threshold (or one per class) fitted on a held-out split.  Both calls work on the log-softmax
    // rows predict()'s hooked forward leaves on the device with the row-local kernels of csrc/conformal.hip (formulas there),
    // at beta = 1 / temperature(), and hold predict()'s contract: the call starts with sync(); the metrics ring, the current
    // split, variable 6 and the captured epoch graph are untouched.  Rows: as calibration() takes them (the nodes of `split`, or
    // with split == 0 the `nodes` query scored against the dataset's labels).  The score table [local rows x smooth_row_ld(C)]
    // is indexed by local row; with diffusion d in (0, 1] the forward and the scores cover every row and one
    // gcnhip_graphsum_blend launch forms S' = d . A^ . S + (1 - d) . S (no clamp) into a second table; d == 0 launches no blend.
    // Refused with a message before any launch: a multi-label model, more than 64 classes, more than one rank, alpha outside
    // (0, 1), a method other than CONFORMAL_LAC / CONFORMAL_APS, lam < 0, k_reg < 0, diffusion outside [0, 1]; for the fit a
    // split without labelled rows; for the sets a NaN threshold, or a fit made at another temperature than the model's
    // current one (the guarantee is for the scores the threshold was fitted on).
    //   conformal_fit: gcnhip_conformal_true_scores on the listed rows, n floats to the host (the quantile is NOT selected on
    //   the device: 93 KB for Reddit's validation split), host/conformal.h's rule.  Not per_class: thresh[c] is the one
    //   threshold and n_cal[c] the number of scored rows, for every c < C; per_class: per label.  scores (may be NULL): the
    //   downloaded scores in list order, -1 for a row without a label in [0, C).
    //   conformal_sets: one gcnhip_conformal_sets_rows launch.  bits [n x ceil(C / 32)] and size [n] (by list position; either may
    //   be NULL) and counts [4 + 3 C + 1] = {rows, labelled rows, covered, empty sets | size_hist [C + 1] | class_support [C] |
    //   class_covered [C]}.  With bits == size == NULL only the counts cross to the host: the coverage report.
    enum ConformalMethod { CONFORMAL_LAC = 0, CONFORMAL_APS = 1 };
    struct Conformal {
        int method = CONFORMAL_APS;
        float lam = 0.f;
        int k_reg = 0;
        float diffusion = 0.f, temperature = 1.f;
        double alpha = 0.1;
        bool per_class = false;
        float thresh[64] = {};
        int64_t n_cal[64] = {};
    };
    Conformal conformal_fit(int split, const int *nodes, int n, double alpha, int method, float lam, int k_reg, float diffusion, bool per_class,
                            std::vector<float> *scores);
    void conformal_sets(const Conformal &fit, int split, const int *nodes, int n, uint32_t *bits, int32_t *size, int64_t *counts);
    // Ranking metrics: per-class ROC-AUC and average precision, the threshold-free scores of multi-label and imbalanced tasks
    // (csrc/ranking.hip: keys, a segmented sort, binary searches; formulas there and in host/ranking.h).  Rows as evaluate()
    // takes them (the nodes of `split`, or with split == 0 the `nodes` query scored against the dataset's labels, repeats
    // counted as often as listed).  predict()'s contract: the call starts with sync(); the metrics ring, the current split,
    // variable 6 and the captured epoch graph are untouched.  One forward: a multi-label model's logits go to scratch and are
    // scored as they are (monotone in the sigmoid, which would saturate into ties); a single-label model is scored one-vs-rest
    // on the log-softmax rows at the current temperature — exactly predict()'s logp: at T != 1 gcnhip_calib_scale_rows runs
    // on every queried row once.  A row whose label is outside [0, C) is in no class's counts (*unlabelled); a NaN score is in
    // neither P nor N of its class (invalid[c]).  The classes run in batches whose two key tables and sort scratch (4 x 4
    // bytes per listed row and class) fit scratch_bytes (0: 256 MiB), at least one class per batch; every batching gives the
    // same bits.  u2 [C] (int64, exact), ap_sum [C] (float64), pos / neg / invalid [C] and *unlabelled are all that crosses
    // to the host — 5 C + 1 numbers — unless scores != NULL: then also the [n x C] f32 score rows in list order, gathered on
    // the device (ROC / PR curves, tests).  Returns the number of listed rows.  Refused with a message before any launch:
    // more than one rank (the sort would need a gather), more than 64 (single-label) or 256 (multi-label) classes, a split
    // outside 0..3, more than 2^24 listed rows.
    int64_t ranking(int split, const int *nodes, int n, size_t scratch_bytes, int64_t *u2, double *ap_sum, int64_t *pos, int64_t *neg, int64_t *invalid,
                    int64_t *unlabelled, std::vector<float> *scores);

    // Multi-label decision thresholds: per class the cut on the logit with the largest F-beta over the listed rows — the last
    // step on data with rare classes, where the training rule z > 0 is seldom the best cut (csrc/thresholds.hip: the rule, the
    // candidates, the float64 expression of F and why every reduction order gives the same bits).  ranking()'s path on a
    // multi-label model up to the sorted key columns: rows as evaluate() takes them, one forward whose logits go to scratch,
    // the classes in ranking()'s batches under the same scratch cap; per batch gcnhip_rank_keys, one sort of both tables and
    // one gcnhip_threshold_scan.  thr [C] f32, tp / fp / fn [C] at the cut, f [C] (float64), pos / neg / invalid [C],
    // defined [C] (0: a class without a positive among the rows — thr 0, F 0) are all that crosses to the host; every batching
    // gives the same bits.  Returns the number of listed rows.  predict()'s contract: the call starts with sync(); the metrics
    // ring, the current split, variable 6 and the captured epoch graph are untouched.  Refused with a message before any
    // launch: a single-label model, more than 256 classes, more than one rank, a split outside 0..3, beta not finite or <= 0,
    // more than 2^24 listed rows.  host/thresholds.h reads and writes the thresholds file.
    int64_t tune_thresholds(int split, const int *nodes, int n, double beta, size_t scratch_bytes, float *thr, int64_t *tp, int64_t *fp, int64_t *fn,
                            double *f, int64_t *pos, int64_t *neg, int64_t *invalid, int32_t *defined);

    // Unseen nodes: classify n_new nodes that were not in the dataset the model was built from — each arrives with its
    // feature row and a list of nodes it links to — without rebuilding the dataset, the adjacency object, its schedule or A^.X.
    // The definition is the loader's rule (host/attach.h): new node i has id N + i and the stored row [N + i, its listed ids...],
    // the ids in [0, N + n_new) (N + k: new node k of the same call), repeats counted as often as listed; the row is appended,
    // no existing row changes, existing nodes do not list it back.  With a(v, j) = 1 / sqrt(len(v) . len(j)), T = [X; X_new] . W1
    // and the dataset nodes' rows exactly as an evaluation forward forms them:
    //   h_v = ReLU(sum_{j in row(v)} a(v, j) T_j),  P_v = h_v . W2,  z_v = sum_{j in row(v)} a(v, j) P_j   for each new v,
    //   P_j = H1_j . W2 of the evaluation forward for a dataset node j: the new rows influence no dataset node.
    // So the logits are what the reference's evaluation forward gives those rows on the augmented dataset.
    // X_new is CSR (x_indptr [n_new + 1], x_indices, x_values); x_indices == NULL: dense rows of input_dim values each.
    // Steps: sync(); HipGCN::forward_class_products (variable 4 = H1.W2 of every dataset node, carrying dinv of its row on a
    // factored model); T of the dataset nodes — variable 1 as that forward wrote it, or on an aggregate-first model one
    // gcnhip_spmm_fwd on the feature object into scratch (its values carry dinv on a factored model, so X_new's are scaled by
    // dinv of the new rows on the host); gcnhip_feat_create + gcnhip_spmm_fwd for X_new; gcnhip_attach_gather with ReLU;
    // gcnhip_matmul_fwd; gcnhip_attach_gather with the predict epilogue at beta = 1 / temperature().  The coefficient stream is
    // a(v, j) per edge on a HIPGCN_EDGE_COEF model; on a factored one dinv(v)^2 for the hidden gather (its result then carries
    // dinv(v), as variable 3 does) and dinv(v) for the class gather.
    // Single-label: pred [n_new], prob [n_new], logp (may be NULL) [n_new x C], as predict() returns them; thr must be NULL.
    // Multi-label: the second gather stores the logits and gcnhip_bce_predict_rows (thr [n_thr = C]: _thr, refused as
    // predict_multilabel refuses) decides: bits [n_new x ceil(C / 32)], prob (may be NULL) [n_new x C] = sigmoid(z).
    // The device scratch is the arena's (the feature object of X_new is the library's own and is destroyed before the call
    // returns); nothing is cached between calls, so nothing can go stale when weights change.  predict()'s contract: the metrics
    // ring, the current split, variable 6 and the captured epoch graph are untouched; variables 1, 3, 4 are rewritten, as by
    // every forward.  Refused with a message before any launch: more than one rank, bf16 tables, a hidden width above 256, more
    // than 64 (single-label) or 256 (multi-label) classes, a malformed X_new (pointers, a column outside the model's input
    // width, dense rows of another width), and everything gcn_attach_rows refuses (a bad id, nbr_ptr, n_new < 0).
    void predict_new(const int *x_indptr, const int *x_indices, const float *x_values, int n_new, const int64_t *nbr_ptr, const int *nbr_ids,
                     const float *thr, int n_thr, int32_t *pred, float *prob, float *logp, uint32_t *bits);

    // Monte Carlo dropout (Gal & Ghahramani, 2016): how sure the model itself is about one node.  S forwards with dropout on,
    // the softmax rows averaged, the predictive entropy split into its expected part and the mutual information between
    // prediction and weights (BALD).  csrc/mcdropout.hip has the definition: sample s in [first_sample, first_sample + samples)
    // is the training forward with the epoch word s, rate p (NULL: params.dropout) and the keys seed ^ KEY_INPUT_DROPOUT /
    // seed ^ KEY_HIDDEN_DROPOUT (seed NULL: env.seed ^ KEY_MC_DROPOUT, so that by default no sample repeats a training epoch's
    // masks; seed = env.seed and first_sample = e draw the masks of training epoch e).  Rows as evaluate() takes them (the nodes of
    // `split`, or with split == 0 the `nodes` query, repeats allowed, NULL: every row).  Per sample: gcnhip_spmm_fwd on the
    // model's feature object with p_drop = p, gcnhip_graphsum_ex with the ReLU + dropout epilogue (training, no pos_bits, no
    // keep_mask) over every row, gcnhip_matmul_fwd, gcnhip_graphsum_predict on the query's row subset, gcnhip_calib_scale_rows
    // when temperature() != 1, gcnhip_mc_accumulate_rows; then one gcnhip_mc_finalize_rows.  The coefficient form is the training
    // forward's own: scaling 2 / 1 on a factored model (the feature values carry dinv), 0 on an HIPGCN_EDGE_COEF one.
    // SCRATCH: T / H / H.W2 are tables of the query's own arena (laid out as variables 1, 3, 4); no variable of the model is
    // written.  The epoch words are a small device array of the arena.  predict()'s contract: the call starts with sync(); the
    // metrics ring, the current split, variable 6, the captured epoch graph, Adam's state, env.d_epoch and the model's mask bits
    // (d_pos_bits) are untouched (the feature object's dropout bits are redrawn: see the head of this file).
    // Outputs by list position, each may be NULL: pred, confidence, entropy, expected_entropy, mutual_information,
    // variation_ratio [n]; mean_prob, votes [n x C]; samples_logp [samples x n x C], the per-sample log-softmax rows gathered on
    // the device in list order.  Returns the rows listed and what was used.  Refused with a message before any launch: a
    // multi-label model, more than 64 classes, more than one rank, bf16 tables, a hidden width above 256, samples outside
    // 1..1024, p outside [0, 1), first_sample + samples > 2^32, a split outside 0..3, a node id outside the graph.
    static constexpr int MC_SAMPLES_MAX = 1024;
    struct McDropout {
        uint64_t seed = 0;
        float p = 0.f;
        int samples = 0;
        uint64_t first_sample = 0;
        int64_t rows = 0;
    };
    // the refusals alone, and the number of rows the query lists (a caller sizes its arrays by it); touches no device state
    int64_t mc_dropout_rows(int split, const int *nodes, int n, int samples, const float *p, uint64_t first_sample);
    McDropout mc_dropout(int split, const int *nodes, int n, int samples, const float *p, const uint64_t *seed, uint64_t first_sample, int32_t *pred,
                         float *confidence, float *entropy, float *expected_entropy, float *mutual_information, float *variation_ratio,
                         float *mean_prob, int32_t *votes, float *samples_logp);

    // k-means on the hidden layer (Lloyd, 1982; seeding: Arthur & Vassilvitskii, 2007): the rows embed() exports, grouped where
    // they lie (csrc/kmeans.hip has the definitions; host/kmeans.cpp the loop).  Rows: the nodes of `split` (1..3) in ascending
    // dataset id, or with split == 0 the `nodes` query (dataset ids in the order given, repeats allowed; NULL: every node in id
    // order) — list order is part of the definition of the update's sums.  Steps: sync(); embed_forward (variable 3 rewritten, as
    // by every forward; with `normalize` its inverse norms, so that the rows clustered are unit rows: a factored model's stored
    // row carries 1 / sqrt(deg), see row_scale(); without it the clustering is of the stored rows); the initial centres —
    // KMEANS_INIT_PLUSPLUS: gcnhip_kmeans_seed on the stream seed ^ KEY_KMEANS (seed NULL: env.seed); KMEANS_INIT_POSITIONS:
    // the rows at k list positions; KMEANS_INIT_CENTERS: k x hidden floats — and their norms (gcnhip_kmeans_update on no rows);
    // then gcnhip_kmeans_assign / gcnhip_kmeans_update until nothing moved or `iters` assignments were made: the four bytes of
    // `moved` are all that is read back per iteration.  Every assignment is followed by its update, so the centres returned are
    // the means of the returned assignment (at a fixed point also the centres it was made to: the same members in the same
    // order give the same bits), and dist2 is measured to the centres the assignment was made to.  Outputs (each may be NULL):
    // assign / dist2 [rows] by list position, centers [k x hidden], sizes [k], seed_pos [k] (list positions; KMEANS_INIT_PLUSPLUS only), history [iters x 2] =
    // (moved, inertia of that assignment) per iteration run, contingency [k x C] (single-label models, at most 64 classes:
    // gcnhip_contingency_rows against the dataset's labels) with *skipped.  predict()'s contract: the metrics ring, the current
    // split, variable 6 and the captured epoch graph are untouched.  Refused with a message before any launch: more than one
    // rank, a hidden width above 256, bf16 tables, k outside 1..256 or above the listed rows, iters < 1, a split outside 0..3,
    // an init position outside the list, a node id outside the graph.
    enum KMeansInit { KMEANS_INIT_PLUSPLUS = 0, KMEANS_INIT_POSITIONS = 1, KMEANS_INIT_CENTERS = 2 };
    struct KMeans {
        int k = 0, iters_run = 0;
        bool converged = false;
        int64_t rows = 0, skipped = 0;
        double inertia = 0;
        uint64_t seed = 0;
    };
    // the refusals alone, and the number of rows the query lists (a caller sizes its arrays by it); touches no device state
    int64_t kmeans_rows(int k, int split, const int *nodes, int n, int iters, int init, const int *init_pos, const float *init_centers);
    KMeans kmeans(int k, int split, const int *nodes, int n, int iters, bool normalize, int init, const int *init_pos, const float *init_centers,
                  const uint64_t *seed, size_t scratch_bytes, int32_t *assign, float *dist2, float *centers, int32_t *sizes, int32_t *seed_pos,
                  double *history, int64_t *contingency);

    // Silhouette widths of a labelling of the hidden layer (Rousseeuw, 1987; csrc/silhouette.hip has the definitions and the order
    // of the sums; host/silhouette_query.cpp the body): how well every listed node sits in its group compared with the next-best
    // group, in the Euclidean geometry of the rows embed() exports.  Rows as kmeans lists them: the nodes of `split` (1..3) in
    // ascending dataset id, or with split == 0 the `nodes` query (dataset ids in the order given, a repeat is a point of its own;
    // NULL: every node in id order).  labels [n_labels] by LIST POSITION — what kmeans() returns as assign for the same arguments —
    // a label outside [0, k) takes its position out of the points (s = a = b = NaN, neighbor = -1, counted in `excluded`).
    // Steps: sync(); embed_forward (variable 3 rewritten, as by every forward; with `normalize` its inverse norms); the list and
    // the labels up; one gcnhip_silhouette_sums with the scratch capped at scratch_bytes (0: SILHOUETTE_SCRATCH_DEFAULT; never
    // below the plan's minimum — fewer bytes, more launches, the same bits); one gcnhip_silhouette_rows.  Outputs, each may be
    // NULL: s / a / b (float64) and neighbor (int32) [rows] by list position, cluster_mean [k] (the mean of s over the points of a
    // label, 0 for an empty one), sizes [k].  score = the mean of s over the points (0 without points).  Nothing is cached.
    // predict()'s contract: the metrics ring, the current split, variable 6 and the captured epoch graph are untouched.  Refused
    // with a message before any launch: more than one rank, bf16 tables, a hidden width above 256, k outside 1..256, a split
    // outside 0..3, a node id outside the graph, labels of another length than the list.
    struct Silhouette {
        int64_t rows = 0, points = 0, excluded = 0;
        int nonempty = 0;
        bool defined = false;                                  // at least two non-empty labels
        double score = 0;
    };
    static constexpr size_t SILHOUETTE_SCRATCH_DEFAULT = (size_t)256 << 20;
    // the refusals alone, and the number of rows the query lists; touches no device state
    int64_t silhouette_rows(int k, int split, const int *nodes, int n, const int32_t *labels, int64_t n_labels, std::vector<int> *rows = nullptr);
    Silhouette silhouette(int split, const int *nodes, int n, const int32_t *labels, int64_t n_labels, int k, bool normalize, size_t scratch_bytes,
                          double *s, double *a, double *b, int32_t *neighbor, double *cluster_mean, int32_t *sizes);

    // Principal components of the hidden layer (Pearson, 1901; Hotelling, 1933): the rows embed() exports, reduced where they lie
    // (csrc/pca.hip has the definitions of the sums; host/pca.h the eigenproblem and what is derived from it; host/pca_query.cpp
    // the bodies).  Rows as kmeans lists them: the nodes of `split` (1..3) in ascending dataset id, or with split == 0 the
    // `nodes` query (dataset ids in the order given, repeats counted as often as listed; NULL: every node in id order) — list
    // order is part of the definition of the sums.
    //   pca_fit: sync(); embed_forward (variable 3 rewritten, as by every forward; with `normalize` its inverse norms); with
    //   `center` one gcnhip_pca_mean; one gcnhip_pca_scatter; h + h . h doubles to the host; gcn_pca_from_scatter; with `coords`
    //   one gcnhip_pca_project of the listed rows onto the leading k components (with `whiten` scaled to unit sample variance, 0
    //   past the rank) and n . k floats to the host.  Outputs, each may be NULL: mean [h] (zeros without `center`), scatter
    //   [h x h], eigenvalues [h], components [h x h] (ROW j = component j), explained [3 x h] = {explained_variance |
    //   explained_variance_ratio | singular_values}, scale [k] (written with `whiten` only), coords [rows x k] by list position.
    //   pca_project: a fit's arrays — width, k, mean [width] (NULL: none), components [k x width] rows, scale [k] (NULL: none) —
    //   applied to the `nodes` query at the CURRENT weights: sync(), embed_forward, one gcnhip_pca_project.  Nothing is cached.
    // predict()'s contract: the metrics ring, the current split, variable 6 and the captured epoch graph are untouched.  Scratch
    // lives in the arena; nothing is allocated until first use.  Refused with a message before any launch: more than one rank,
    // bf16 tables, a hidden width above 256, k outside 1..hidden, fewer than 2 listed rows, a split outside 0..3, a node id outside
    // the graph; for pca_project a fit of another width or one that is not finite.
    struct Pca {
        int k = 0, rank = 0;
        int64_t rows = 0;
    };
    // the refusals alone, and the number of rows the query lists (a caller sizes its arrays by it); touches no device state
    int64_t pca_rows(int k, int split, const int *nodes, int n, std::vector<int> *rows = nullptr);   // rows: the local rows listed
    Pca pca_fit(int k, int split, const int *nodes, int n, bool normalize, bool center, bool whiten, size_t scratch_bytes, double *mean, double *scatter,
                double *eigenvalues, double *components, double *explained, double *scale, float *coords);
    int64_t pca_project(int width, int k, const double *mean, const double *components, const double *scale, bool normalize, const int *nodes, int n,
                        float *out);

    // Label structure of the graph (csrc/structure.hip has the definitions; host/structure_query.cpp the bodies; host/structure.h
    // turns the integers into homophily measures and strata tables): WHERE on the graph a labelling agrees with itself, and where
    // the model is right.  Arrays are in DATASET node order.  Rows: the nodes of `split` (1..3) in ascending dataset id, or with
    // split == 0 the `nodes` query (dataset ids in the order given, repeats counted as often as listed; NULL: every node in id
    // order); the mapping to local rows and back goes through query_rows and node_id().  The adjacency walked is the model's own
    // object with its stored rows (self loop included, as the loader made them).
    //   neighbor_agreement: `labels` is ANY int32 array [n_labels = num_nodes] — the dataset's labels, predict()'s output,
    //   cluster()'s assign — with x known when 0 <= x < num_classes <= 64.  It needs neither weights nor a forward and takes
    //   single- and multi-label models alike: sync(), the labels to local row order on the host and up, one gcnhip_nbr_agreement
    //   launch.  deg / same / known [rows] by list position (each may be NULL), mix [C x C] (may be NULL), class_rows [C],
    //   totals [8].
    //   structure: sync(); the agreement launch on the dataset's labels; with `predicted` one evaluation forward with the
    //   prediction epilogue over every row (forward_predict(NULL, false)), the agreement launch on the predictions, and one
    //   gcnhip_strata_counts launch with agreement measured on the TRUTH: strata [32 x (bins + 1) x 2].  Without `predicted` the
    //   three *_pred outputs and strata are left as they are.  deg / same / known: the truth's, by list position.
    // Only mix (twice), class_rows, totals and strata cross to the host, and with per-position outputs asked for three int32 per
    // list position.  predict()'s contract: the metrics ring, the current split, variable 6 and the captured epoch graph are
    // untouched; a train_epoch() after it has the same bits as one without it.  Scratch lives in the arena; nothing is allocated
    // until first use.  Refused with a message before any launch: more than one rank (column labels would need an exchange), more
    // than 64 classes, bins outside 1..32, a split outside 0..3, a node id outside the graph, a label array of another length
    // than num_nodes, and for structure with `predicted` a multi-label model.
    struct Structure {
        int64_t rows = 0, skipped = 0, unlabelled = 0;         // listed; outside the adjacency (none from a checked query); strata's
    };
    // the refusals alone, and the number of rows the query lists (a caller sizes its arrays by it); touches no device state
    int64_t structure_rows(const char *what, int num_classes, int bins, bool predicted, int split, const int *nodes, int n);
    Structure neighbor_agreement(const int32_t *labels, int64_t n_labels, int num_classes, int split, const int *nodes, int n, int32_t *deg,
                                 int32_t *same, int32_t *known, int64_t *mix, int64_t *class_rows, int64_t *totals);
    Structure structure(int split, const int *nodes, int n, int bins, bool predicted, int32_t *deg, int32_t *same, int32_t *known, int64_t *mix_truth,
                        int64_t *class_rows_truth, int64_t *totals_truth, int64_t *mix_pred, int64_t *class_rows_pred, int64_t *totals_pred,
                        int64_t *strata);

    // Reach of the labels (csrc/reach.hip has the definitions; host/reach_query.cpp the bodies; host/reach.h turns the strata into
    // accuracy by distance): HOW FAR every node is from the labelled nodes the model learns from, which nodes hang together, and
    // how the accuracy falls with that distance.  Arrays are in DATASET node order.  Rows: the nodes of `split` (1..3) in
    // ascending dataset id, or with split == 0 the `nodes` query (dataset ids in the order given, repeats counted as often as
    // listed; NULL: every node in id order).  SOURCES (and the marks of components): the nodes of the splits in `source_mask`
    // (bit s = split s, 2 = the training split), or with source_mask == 0 the n_sources dataset ids of `source_nodes` (repeats
    // allowed, none: no source).  The adjacency walked is the model's own object with its stored rows; the distance follows the
    // direction of an aggregation (row v gathers from the entries it lists), the components are weak.  One rank only, and there
    // a row is a node: the traversal's tie rule — the LOWEST ROW among the sources at the same distance — is by local row, which
    // without a forced node order is the dataset id; nearest and component are mapped to dataset ids through node_id().
    //   label_distance: sync(); one gcnhip_hop_distance over the whole graph (max_hops 0: no limit).  dist / nearest [rows] by list
    //   position (nearest may be NULL, and is then not computed: a row stops at its first hit); level_counts [capacity] as the
    //   kernel call fills it.
    //   components: sync(); gcnhip_components and gcnhip_component_counts with the sources as marks.  component / size [rows] by
    //   list position (each may be NULL): the component's smallest row as a dataset id, and its number of nodes; totals [6].
    //   reach: sync(); with `predicted` one evaluation forward with the prediction epilogue over every row (forward_predict(NULL,
    //   false)); the traversal from the sources without a hop limit, with nearest; the components with the sources as marks; one
    //   gcnhip_distance_strata over the listed rows against the dataset's labels: strata [(hops + 2) x 4].  dist / nearest /
    //   component [rows] by list position, each may be NULL.
    // Only the strata, the totals and the level counts cross to the host, and with per-position outputs asked for one int32 array
    // of every local row each.  predict()'s contract: the metrics ring, the current split, variable 6 and the captured epoch graph
    // are untouched; a train_epoch() after it has the same bits as one without it.  Scratch lives in the arena; nothing is
    // allocated until first use.  Single- and multi-label models alike, except reach with `predicted`.  Refused with a message
    // before any launch: more than one rank (the traversal would need an exchange per level), a split outside 0..3, a source mask
    // with other bits than 1..3, a node id outside the graph, max_hops < 0, hops outside 1..32, and for reach with `predicted` a
    // multi-label model.
    struct Reach {
        int64_t rows = 0, sources = 0, skipped = 0, unlabelled = 0, unreachable = 0;   // listed; rows that became sources; ...; listed with dist -1
        int levels = 0, rounds = 0;
    };
    // the refusals alone, and the number of rows the query lists (a caller sizes its arrays by it); touches no device state
    int64_t reach_rows(const char *what, int split, const int *nodes, int n, int source_mask, const int *source_nodes, int n_sources, int max_hops,
                       int hops, bool predicted);
    Reach label_distance(int source_mask, const int *source_nodes, int n_sources, int split, const int *nodes, int n, int max_hops, int32_t *dist,
                         int32_t *nearest, int64_t *level_counts, int capacity);
    Reach components(int split, const int *nodes, int n, int source_mask, const int *source_nodes, int n_sources, int32_t *component, int32_t *size,
                     int64_t *totals);
    Reach reach(int split, const int *nodes, int n, int source_mask, const int *source_nodes, int n_sources, int hops, bool predicted, int32_t *dist,
                int32_t *nearest, int32_t *component, int64_t *strata, int64_t *totals, int64_t *level_counts, int capacity);

private:
    HipGCN &m;
    DeviceArena arena;                                       // every device buffer of a query
    // Device scratch that grows and never shrinks: need(n) returns room for n elements (for one when n == 0: a rank without
    // rows), allocated on first use and again, contents not kept, when n exceeds the capacity.  An allocation that throws leaves
    // capacity 0 and NULL behind.  Zeroed: a new block is cleared (tables whose padding no launch writes but a download may read).
    template <class T, bool Zeroed = false>
    struct Scratch {
        DeviceArena *arena;
        T *p = nullptr;
        size_t cap = 0;
        T *need(size_t n) {
            if (n < 1) n = 1;
            if (n <= cap) return p;
            cap = 0;
            arena->release(p);
            p = nullptr;
            p = Zeroed ? arena->alloc_zeroed<T>(n) : arena->alloc<T>(n);
            cap = n;
            return p;
        }
    };
    // what a call needs of the model (require): the refusals every query shares, worded once
    enum Need { SINGLE_LABEL = 1, MULTI_LABEL = 2, CLASS_AGGREGATION = 4, AT_MOST_64 = 8, AT_MOST_256 = 16, ONE_RANK = 32 };
    void require(const char *what, int needs) const;

    // predict, evaluate, calibration, Correct & Smooth: predicted class and its probability per local row, the log-softmax rows
    // [local rows x C]; the last node query's row subset (registered on the adjacency, removed when the next query differs)
    Scratch<int32_t> d_pred{&arena};
    Scratch<float> d_prob{&arena}, d_logp{&arena};
    std::vector<uint32_t> pred_bits;
    gcnhip_rowset *pred_rows = nullptr;
    // predict_multilabel, evaluate: scratch logits [local rows x ld of Z]; the query's bits, probabilities and rows
    Scratch<float, true> d_ml_logits{&arena};
    Scratch<uint32_t> d_ml_bits{&arena};
    Scratch<float> d_ml_prob{&arena};
    Scratch<int32_t> d_ml_rows{&arena};
    // evaluate: the counts on the device (also the float limbs of their all-reduce), an uploaded row list; every local label,
    // uploaded once
    Scratch<int32_t> d_eval_counts{&arena}, d_eval_rows{&arena};
    int32_t *d_label_all = nullptr;
    // propagate / label_propagation / correct_and_smooth: four tables [local rows x ld] that grow together, the merged truth of
    // the known splits, sigma = {sum |E_0|, rows}
    Scratch<float, true> d_smooth[4] = {{&arena}, {&arena}, {&arena}, {&arena}};
    Scratch<int32_t> d_smooth_truth{&arena};
    Scratch<float> d_sigma{&arena};
    // calibration / calibrate: {nll sums [4] | conf_sum [2 x 64]} doubles and {count, correct} [2 x 2 x 64] ints on the device
    float temperature_ = 1.f;
    Scratch<double> d_calib_sums{&arena};
    Scratch<int32_t> d_calib_counts{&arena};
    // embed / similar / score_pairs: inverse norms [local rows]; the dataset id of every local row, uploaded once; the query's
    // rows (two lists for pairs), its float and int results, and the partial lists of the top-k product
    Scratch<float> d_emb_inv{&arena}, d_emb_out{&arena};
    Scratch<int32_t> d_emb_rows{&arena}, d_emb_ids{&arena};
    Scratch<unsigned char> d_emb_scratch{&arena};
    int32_t *d_node_ids = nullptr;
    static constexpr size_t EMBED_SCRATCH_CAP = (size_t)64 << 20;
    // explain / feature_importance: the row pointers of the adjacency (host, downloaded once: the graph never changes); the
    // query's rows, classes and scan; its outputs; the features batch; the importance sums
    std::vector<int> xp_indptr;
    Scratch<int32_t> d_xp_rows{&arena}, d_xp_cls{&arena}, d_xp_ptr{&arena}, d_xp_nbr_row{&arena}, d_xp_count{&arena};
    Scratch<float> d_xp_logit{&arena}, d_xp_hidden{&arena}, d_xp_nbr_val{&arena}, d_xp_feat{&arena}, d_xp_z{&arena};
    Scratch<double> d_xp_acc{&arena};
    // conformal_fit / conformal_sets: the score table and its diffused copy [local rows x ld]; the listed rows' true scores; the
    // thresholds [64]; the sets' bits, sizes and counts
    Scratch<float, true> d_cf_table[2] = {{&arena}, {&arena}};
    Scratch<float> d_cf_score{&arena}, d_cf_thresh{&arena};
    Scratch<uint32_t> d_cf_bits{&arena};
    Scratch<int32_t> d_cf_size{&arena}, d_cf_counts{&arena};
    // ranking: a batch's key tables and sort scratch; the counts {pos | neg | invalid [C] | unlabelled}; {ap_sum | u2} [2 C]; the
    // block partials of gcnhip_rank_stats; the gathered score rows; a query's rows listed once (the temperature rescale)
    static constexpr size_t RANKING_SCRATCH_DEFAULT = (size_t)256 << 20;
    static constexpr int RANKING_ROWS_MAX = 1 << 24;
    Scratch<uint32_t> d_rk_keys{&arena};
    Scratch<int32_t> d_rk_counts{&arena}, d_rk_once{&arena};
    Scratch<double> d_rk_sums{&arena}, d_rk_work{&arena};
    Scratch<float> d_rk_scores{&arena};
    // tune_thresholds: one block {f [C] | thr [C] | TP, FP, FN per batch | defined [C]}; the cuts a query or an evaluation decides by
    Scratch<double> d_th_fit{&arena};
    Scratch<float> d_th_cuts{&arena};
    // predict_new: T of the dataset nodes (aggregate-first models), T / H1 / H1.W2 / logits of the new rows; their stored rows
    // and the two coefficient streams; the results
    Scratch<float> d_nn_ta{&arena}, d_nn_tb{&arena}, d_nn_pb{&arena}, d_nn_z{&arena}, d_nn_coef{&arena}, d_nn_prob{&arena}, d_nn_logp{&arena};
    Scratch<float, true> d_nn_hb{&arena};
    Scratch<int32_t> d_nn_ptr{&arena}, d_nn_col{&arena}, d_nn_pred{&arena};
    Scratch<uint32_t> d_nn_bits{&arena};
    // mc_dropout: T / H / H.W2 of a sample [local rows x ld of variables 1 / 3 / 4]; the epoch words; the accumulators by list
    // position; the f32 results {confidence | entropy | expected | mutual information | variation ratio | mean_prob}; pred; the
    // gathered per-sample rows; a query's rows listed once (the temperature rescale)
    Scratch<float, true> d_mc_t{&arena}, d_mc_h{&arena}, d_mc_p{&arena};
    Scratch<uint32_t> d_mc_epoch{&arena};
    Scratch<double> d_mc_acc{&arena};
    Scratch<int32_t> d_mc_votes{&arena}, d_mc_pred{&arena}, d_mc_once{&arena};
    Scratch<float> d_mc_out{&arena}, d_mc_samples{&arena};
    // kmeans: the listed rows, centres and their norms, both assignments, distances, sizes, seed positions, {moved | skipped},
    // the inertia, the update's and the seeding's scratch, the cluster x class counts
    Scratch<int32_t> d_km_rows{&arena}, d_km_assign{&arena}, d_km_sizes{&arena}, d_km_pos{&arena}, d_km_flag{&arena}, d_km_counts{&arena};
    Scratch<float> d_km_centers{&arena}, d_km_cn{&arena}, d_km_dist{&arena};
    Scratch<double> d_km_inertia{&arena};
    Scratch<unsigned char> d_km_scratch{&arena};
    std::vector<int> kmeans_list(const char *what, int split, const int *nodes, int &n);
    // silhouette: {rows | labels | neighbor [n] | sizes [k] | counts [3]}, the sums [n x k], {s | a | b [n] | cluster_sum [k] |
    // total}, the sums' scratch
    Scratch<int32_t> d_sil_int{&arena};
    Scratch<double> d_sil_sums{&arena}, d_sil_out{&arena};
    Scratch<unsigned char> d_sil_scratch{&arena};
    // pca_fit / pca_project: the listed rows, the valid count, {mean [h] | scatter [h x h]}, {mean | basis [h x k] | scale [k]} of
    // a projection, its coordinates, the sums' scratch
    Scratch<int32_t> d_pca_rows{&arena}, d_pca_count{&arena};
    Scratch<double> d_pca_stats{&arena}, d_pca_basis{&arena};
    Scratch<float> d_pca_out{&arena};
    Scratch<unsigned char> d_pca_scratch{&arena};
    // neighbor_agreement / structure: the listed rows, the labels by local row (the last launch's), the per-position counts
    // {deg | same | known} of the truth and of the second labelling, {mix [C x C] | class_rows [C] | totals [8] | skipped} and
    // {strata | unlabelled} as int64
    Scratch<int32_t> d_st_rows{&arena}, d_st_lab{&arena}, d_st_per{&arena}, d_st_per2{&arena};
    Scratch<int64_t> d_st_counts{&arena}, d_st_strata{&arena};
    struct AgreementOut { int32_t *deg, *same, *known; int64_t *mix, *class_rows, *totals; };
    // one launch on `d_lab` (local rows) over the uploaded list and the copies to the host; returns the skipped positions
    int64_t agreement_launch(const int32_t *d_lab, int C, const int32_t *d_rows, int n, int32_t *d_per, const AgreementOut &out);

    // label_distance / components / reach: the listed rows, the source rows and their flag per row, dist / nearest / comp / size /
    // marked [local rows], {the kernels' scratch [64] | totals [6] | strata [(hops + 2) x 4] | unlabelled} as int64
    Scratch<int32_t> d_rc_rows{&arena}, d_rc_seeds{&arena}, d_rc_mark{&arena}, d_rc_dist{&arena}, d_rc_nearest{&arena}, d_rc_comp{&arena},
        d_rc_size{&arena}, d_rc_marked{&arena};
    Scratch<int64_t> d_rc_counts{&arena};
    std::vector<int> reach_sources(const char *what, int source_mask, const int *source_nodes, int n_sources);
    // the traversal from `sources` (local rows) into d_rc_dist (and d_rc_nearest); the components into d_rc_comp / _size / _marked
    void reach_traverse(const std::vector<int> &sources, int max_hops, bool want_nearest, int64_t *level_counts, int capacity, Reach &res);
    void reach_components(const std::vector<int> &sources, int64_t *totals, Reach &res);
    // one int32 per local row to the host, picked at the listed rows; as_node: rows >= 0 become dataset ids
    void reach_pick(const int32_t *d_per_row, const std::vector<int> &rows, bool as_node, int32_t *out);

    void query_rows(const char *what, const int *nodes, int n, std::vector<int> &rows);   // dataset ids -> local rows
    const gcnhip_rowset *query_subset(const std::vector<int> &rows);
    const int32_t *upload_rows(const std::vector<int> &rows);
    // the rows a split or a query names, as evaluate() lists them, and the truth they are scored against
    struct ScoredRows { const int32_t *d_list; int n; const int32_t *truth; const gcnhip_rowset *subset; };
    ScoredRows scored_rows(const char *what, int split, const int *nodes, int n);
    // the two hooked forwards: d_pred / d_prob (and d_logp when kept) of the subset's rows; their logits into d_ml_logits
    void forward_predict(const gcnhip_rowset *subset, bool keep_logp);
    void forward_redirect(const gcnhip_rowset *subset);
    // predict_multilabel and the multi-label evaluate, by z > 0 (thr == NULL) or by the cuts thr [C] (host)
    void predict_multilabel_rows(const int *nodes, int n, const float *thr, uint32_t *bits, float *prob);
    void evaluate_rows(int split, const int *nodes, int n, const float *thr, int64_t *counts, int64_t *rows_counted, int64_t *unlabelled);
    void thresholds_check(const char *what, const float *thr, int n_thr) const;
    const float *upload_cuts(const float *thr);
    // ranking and tune_thresholds: the classes in batches whose two key tables and sort scratch fit the cap; per batch
    // gcnhip_rank_keys and one sort of both tables, then stats(c0, S, pos_keys, neg_keys, stride, d_pos, d_neg, d_work) with
    // the batch's counts and a work block of S * 32 * 16 bytes.  Returns the counts {pos | neg | invalid [C] | unlabelled}.
    using BatchStats = std::function<void(int c0, int S, const uint32_t *pos_keys, const uint32_t *neg_keys, int64_t stride, const int32_t *d_pos,
                                          const int32_t *d_neg, void *d_work)>;
    const int32_t *sorted_class_batches(const ScoredRows &q, const float *table, int ld, size_t scratch_bytes, const BatchStats &stats);
    static int smooth_row_ld(int dim) { return dim <= 32 ? (dim + 3) / 4 * 4 : (dim + 15) / 16 * 16; }   // HipVariable's rule
    void smooth_check(const char *what, int needs, float alpha, int iters) const;
    const int32_t *smooth_truth(const char *what, int splits_mask, std::vector<int32_t> *host);
    float *smooth_iterate(const float *base, float *a, float *b, int ld, int dim, float alpha, int iters, float lo, float hi, int32_t *pred);
    void smooth_download(const float *table, int ld, int dim, float *out, int32_t *pred_from_rows);
    void smooth_pred_download(int32_t *pred);
    void calib_check(const char *what, float temperature, int bins) const;
    void embed_check(const char *what, int metric) const;
    std::vector<int> embed_query(const char *what, const int *nodes, int &n);            // dataset ids (NULL: all) -> local rows
    struct EmbedTable { const float *data; int ld, rows, dim; const float *inv_norm; };
    EmbedTable embed_forward(bool norms);                      // the hidden matrix where variable 3 keeps it (and its inverse norms)
    void explain_check(const char *what, bool default_classes) const;
    const std::vector<int> &explain_indptr();
    // the forward of an explanation: variable 3 rewritten; cls = the given classes (checked) or each row's highest logit
    // (d_rows: `rows` on the device)
    EmbedTable explain_forward(const char *what, const std::vector<int> &rows, const int32_t *d_rows, const int *classes, std::vector<int32_t> &cls);
    // the feature shares of n uploaded queries in batches of at most cap_bytes: copied to host_out [n x F] and / or added to the
    // importance sums
    void explain_features(const EmbedTable &t, const int32_t *d_rows, const int32_t *d_cls, int n, size_t cap_bytes, float *host_out, double *d_acc,
                          int32_t *d_count);
    void calib_bins_download(const ScoredRows &q, float beta, int bins, int slot, int64_t *count, int64_t *correct, double *conf_sum);
    void conformal_check(const char *what, int split, int n, double alpha, int method, float lam, int k_reg, float diffusion) const;
    // the forward, the scores launch and the blend of both calls; returns the table the rows are read from (row stride *ld)
    const float *conformal_table(const ScoredRows &q, int method, float lam, int k_reg, float diffusion, int *ld);
};
