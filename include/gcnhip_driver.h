/*
 * gcnhip_driver.h — entry points of libgcnhip.so beyond the 1:1 surface of gcnhip.h: the protocol of THIS repository's host
 * driver (cuda_gcn_amd/host: HipGCN and its Hip* modules).
 *
 * gcnhip.h holds one entry point per kernel-launching wrapper of the reference — what a maintainer binding the library
 * into the reference's own CUDA* modules calls.  Everything here is an optimisation of the same
 * operators that the host driver uses: fused epilogues (ReLU / dropout / mask bits / loss in the aggregation; ReLU and the
 * second product in the first-layer GEMM), operators restricted to row subsets or column sets, the factored
 * coefficients, split-K parts of the weight gradient, bf16 table storage, the fused backward of the class layer, and
 * the device-side bookkeeping of graph-replayed epochs (counters, metrics ring, capture).  Each declaration cites the
 * reference lines whose work it takes over; conventions (return codes, streams, layouts) are those of gcnhip.h.
 * tests/test_abi_cpu.py checks that the library exports every symbol of both headers.
 */
#ifndef GCNHIP_DRIVER_H
#define GCNHIP_DRIVER_H
#include "gcnhip.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct gcnhip_rowset gcnhip_rowset;   /* a registered subset of an adjacency object's rows */

/* Hint: the launches of this context are meant to run BESIDE another stream's kernels (HipGCN's validation lane next to
 * the training pass).  Ops that have a whole-chip persistent form (the dense first-layer GEMM: one 512-thread workgroup
 * with 150 KB of LDS per CU for the whole launch) then take their tiled form, which leaves wave slots and registers to the
 * neighbour: measured on the two-stream epoch, 294 epochs/s with the persistent form on the lane against 297 with tiles.
 * Results do not depend on the hint beyond the order of floating-point sums of the two forms (each within the tested bound). */
int gcnhip_ctx_set_corun(gcnhip_ctx *ctx, int on);
/* The compute units of the context's device: every launcher caps its grid by a multiple of this count. */
int gcnhip_ctx_compute_units(const gcnhip_ctx *ctx, int *count);
/* Read-back without stalling the producer: page-locked host memory and a device-to-host copy that is only ENQUEUED on
 * ctx's stream (wait for it with an event recorded behind it + gcnhip_event_sync).  HipGCN::run() uses them to
 * print epoch e's line while epochs e+1.. are already running: behind a group of epochs, the metrics rows of the group are
 * copied on the producing stream and an event recorded that the host waits on.  (The reference's CUDA path instead blocks
 * on a cudaMemcpy of the whole logits matrix per accuracy call, src/cuda/cuda_gcn.cu:100-120.) */
int gcnhip_host_alloc(void **ptr, size_t bytes);
int gcnhip_host_free(void *ptr);
int gcnhip_d2h_async(gcnhip_ctx *ctx, void *dst_pinned, const void *src, size_t bytes);
/* As above, with a locality hint: h_row_group[r] >= 0 names the community of row r (any small integer
 * key; the host passes the node's label).  Rows of one group are scheduled together — group-major, heavy rows
 * first inside a group — so the neighbour rows they share stay in the XCD's L2 while the group is processed.
 * Results are those of gcnhip_graph_create bit for bit: no node is renamed and the order of every row's own
 * sum is unchanged; only the order in which rows are computed differs.  NULL = no hint. */
int gcnhip_graph_create_grouped(gcnhip_ctx *ctx, gcnhip_graph **g, const int *h_indptr, const int *h_indices,
                                int n_rows, int n_cols, const int *h_col_deg, const int *h_row_group);
/* Replace the row schedule of a prepared adjacency (synchronises the context).  The aggregation computes one
 * row per wave; WHICH rows are in flight together decides what the caches hold and whether bandwidth-bound hub rows
 * overlap with the overhead-bound tail of short rows.  Every schedule gives bit-identical results.
 *   mode 0: descending degree (what gcnhip_graph_create builds)
 *   mode 1: h_row_group-major, descending degree inside a group (= gcnhip_graph_create_grouped)
 *   mode 2: descending-degree rank dealt round-robin into n_groups groups (every group has the same degree mix),
 *           group-major; measured on an R-MAT graph with a 1 GiB table: 6.9 -> 5.3 ms at d = 128
 * The host (HipGCN) times the candidates once per dataset and keeps the fastest. */
int gcnhip_graph_set_schedule(gcnhip_ctx *ctx, gcnhip_graph *g, int mode, const int *h_row_group, int n_groups);
/* Same operator when whole rows of `in` are known to be zero: bit j of in_row_bits (n_cols bits,
 * word j >> 5) == 0 promises that row j is all zero, and the kernel does not read it.  The backward
 * of the output layer is the case: dZ is zero for every node outside the training split
 * (module.cpp:129-133), so a third of Reddit's gathers (and 95 % of Cora's) are skipped with
 * identical results. */
int gcnhip_graphsum_rowmask(gcnhip_ctx *ctx, const gcnhip_graph *g, const float *in, int ld_in,
                            float *out, int ld_out, int dim, const uint32_t *in_row_bits);
/* ... and when only some rows of `out` are ever read: bit r of out_row_bits (n_rows bits) == 0 means row r is
 * not computed and its memory is left untouched.  The last aggregation of a forward is the case: the loss and the
 * accuracy read only rows whose node is in the scored split (CrossEntropyLoss::forward, module.cpp:131-133;
 * GCN::get_accuracy, gcn.cpp:86-88), i.e. 66 % of Reddit's rows in a training forward and 10 % in a validation
 * forward.  Every computed row is bit-identical to gcnhip_graphsum's.  Either mask may be NULL. */
int gcnhip_graphsum_masked(gcnhip_ctx *ctx, const gcnhip_graph *g, const float *in, int ld_in,
                           float *out, int ld_out, int dim, const uint32_t *in_row_bits, const uint32_t *out_row_bits);
/* The same for a subset that is known in advance (the three splits of a dataset): gcnhip_graph_add_rowset cuts a
 * compacted task list for the rows with bit r set in h_row_bits (host, n_rows bits) out of the object's row schedule
 * — no wave is launched for a row outside it (the device mask above launches every wave and retires the unwanted ones:
 * at 10 % wanted rows that is 4x slower than the compacted list).  The subset belongs to the object: it follows
 * gcnhip_graph_set_schedule and is freed by gcnhip_graph_destroy; passing it with any other adjacency object is an
 * argument error (-1).  Results as gcnhip_graphsum_masked. */
int gcnhip_graph_add_rowset(gcnhip_ctx *ctx, gcnhip_graph *g, const uint32_t *h_row_bits, gcnhip_rowset **rows);
int gcnhip_rowset_size(const gcnhip_rowset *rows, int *n_tasks);
int gcnhip_graphsum_rowset(gcnhip_ctx *ctx, const gcnhip_graph *g, const gcnhip_rowset *rows, const float *in, int ld_in,
                           float *out, int ld_out, int dim, const uint32_t *in_row_bits);
/* When the zero rows of an aggregation's input are known for good (the backward of the output layer: dZ is zero for every
 * node outside the training split, module.cpp:129-133), the edges that point at them can be left out of the operator
 * instead of being masked at every launch: gcnhip_graph_create_restricted builds a second adjacency object with the
 * edges of `parent` whose SOURCE row (column index) has bit j set in h_col_bits (host, n_cols bits), the parent's
 * coefficients (degrees of the full graph, module.cpp:91-93) and the parent's current row order.  Aggregating an input
 * that is zero outside the set through it gives the same sum with the zero terms absent (the remaining terms may be
 * added in a different order: within the f32 bound of the tests, not bit-identical to the masked launch).  At Reddit
 * scale the masked class-width backward takes 0.39 ms, the restricted operator 0.27 ms (a third of the edges gone and
 * no predicate on the loads).  The object is independent of the parent: destroy it with gcnhip_graph_destroy. */
int gcnhip_graph_create_restricted(gcnhip_ctx *ctx, gcnhip_graph **out, const gcnhip_graph *parent, const uint32_t *h_col_bits);
/* A second, independent object with the parent's edges, coefficients and CURRENT row order and its own task lists and split-row
 * scratch — for a second stream that aggregates through the same adjacency at the same time (HipGCN's validation lane).  Device
 * copies only: the host preparation of gcnhip_graph_create (per-row neighbour sort: 0.4 s at Reddit scale) is not repeated.
 * Row subsets are not copied: register them on the clone.  Synchronises the context. */
int gcnhip_graph_clone(gcnhip_ctx *ctx, gcnhip_graph **out, const gcnhip_graph *parent);
/* One PART of an aggregation whose edges were split over two operators with the same rows (both made by
 * gcnhip_graph_create_restricted from one parent with complementary column sets).  The row-partitioned epoch uses it
 * to start on the edges that point at this rank's own rows while the rows of the other ranks are still in flight on the
 * exchange stream, then adds the remaining edges (xGMI note):
 *     accumulate == 0:  out[r,:]  = sum over the operator's edges            (the first part)
 *     accumulate != 0:  out[r,:]  = out[r,:] + that sum                      (the second part; rows with no edge keep their value)
 * with every option of the other entry points: rows (NULL or a subset registered on THIS g), in_row_bits (NULL or as in
 * gcnhip_graphsum_rowmask), and relu_dropout != 0 = the epilogue of gcnhip_graphsum_relu_dropout applied AFTER the
 * addition, i.e. by the last part only.  The sum of a row is then (terms of part 1) + (terms of part 2): the same real
 * number as gcnhip_graphsum on the parent, associated differently — within the f32 bound of the tests, not bit-identical. */
int gcnhip_graphsum_part(gcnhip_ctx *ctx, const gcnhip_graph *g, const gcnhip_rowset *rows, const float *in, int ld_in,
                         float *out, int ld_out, int dim, const uint32_t *in_row_bits, int accumulate,
                         int relu_dropout, int training, float p, uint64_t seed, const uint32_t *d_epoch,
                         uint64_t elem_offset, const uint8_t *keep_mask);
/* Fused epilogue used by the first layer: GraphSum, then ReLU
 * (module.cpp:175-185), then Dropout (module.cpp:207-221) on the same rows.
 * training == 0: ReLU only.  The dropout decision for element (r, c) is
 * keep(seed, *d_epoch, elem_offset + r*dim + c) (see gcnhip_dropout_fwd), or
 * keep_mask[r*dim + c] != 0 when keep_mask != NULL.  No mask is stored:
 * backward recovers it as out > 0 (gcnhip_relu_dropout_bwd). */
int gcnhip_graphsum_relu_dropout(gcnhip_ctx *ctx, const gcnhip_graph *g, const float *in, int ld_in,
                                 float *out, int ld_out, int dim, int training, float p,
                                 uint64_t seed, const uint32_t *d_epoch, uint64_t elem_offset,
                                 const uint8_t *keep_mask);
/* The same, also leaving the mask its backward needs as ONE BIT per element: bit (c & 31) of
 * pos_bits[r * words_per_row + (c >> 5)] = (out[r, c] > 0) after ReLU and dropout (the reference keeps a bool array for the
 * ReLU and an int array for the Dropout, module.cpp:166-173, 196-205: 5 bytes per element).  The bits are assembled from
 * the lanes that store the row, so they cost no extra pass; gcnhip_matmul_bwd_fused_bits reads them instead of re-reading
 * the activations (119 MB per epoch at Reddit scale).  Needs dim % 32 == 0, 16-byte aligned rows and
 * words_per_row * 32 >= dim; rows of a registered subset are not supported (the hidden layer computes every row). */
int gcnhip_graphsum_relu_dropout_bits(gcnhip_ctx *ctx, const gcnhip_graph *g, const float *in, int ld_in,
                                      float *out, int ld_out, int dim, int training, float p,
                                      uint64_t seed, const uint32_t *d_epoch, uint64_t elem_offset,
                                      const uint8_t *keep_mask, uint32_t *pos_bits, int words_per_row);
/* ---- the factored operator (round 4) ------------------------------------------------------------------------------
 * A^ = D^-1/2 (A + I) D^-1/2.  The reference multiplies every gathered row by a per-EDGE coefficient
 * 1/sqrt(deg(src) deg(dst)) (module.cpp:91-93), and so do the entry points above — which makes the coefficient array a
 * second stream beside the indices: 94 MB per launch at Reddit scale, measured at 6 % (hidden width) to 10 % (class width)
 * of the launch (tools/gather_peak.py --coef; profiles/r04_gather_peak.json).  The same operator FACTORED needs no per-edge
 * number at all:  (A^ x)[r] = dinv[r] * sum_e (dinv[col(e)] * x[col(e)]),  dinv = 1/sqrt(deg).
 * gcnhip_graphsum_ex with scaling != 0 computes  out[r] = post[r] * sum_e in[col(e)]  where the CALLER has stored
 * dinv[col] * x[col] in `in` (every producer on the training path has a row-wise epilogue or a value array that takes the
 * factor for free: HipGCN, host/gcn.cpp "factored").  scaling: 0 = per-edge coefficients (identical to the entry points
 * above), 1 = post = dinv[row], 2 = post = dinv[row]^2 (= 1/deg: the result is already dinv-scaled for the NEXT
 * aggregation), 3 = no post factor (the consumer folds dinv[row] in, e.g. through a pre-scaled feature matrix).
 * Same real numbers as the reference's operator; each term carries two more f32 roundings (dinv[r] * (dinv[c] * x)
 * instead of coef * x), inside the summation-order bound the parity tests use.  f32 rows, 16-byte aligned.
 * The other fields are the options of gcnhip_graphsum_rowset / _rowmask / _part / _relu_dropout_bits, all optional. */
typedef struct {
    const gcnhip_rowset *rows;          /* NULL: every row */
    const uint32_t *in_row_bits;        /* NULL, or as gcnhip_graphsum_rowmask */
    int accumulate;                     /* as gcnhip_graphsum_part: out = out + sum (then post, then the epilogue) */
    int relu_dropout, training;         /* the fused epilogue of gcnhip_graphsum_relu_dropout */
    float p;
    uint64_t seed;
    const uint32_t *d_epoch;
    uint64_t elem_offset;
    const uint8_t *keep_mask;
    uint32_t *pos_bits;                 /* NULL, or as gcnhip_graphsum_relu_dropout_bits (needs relu_dropout) */
    int words_per_row;
    int scaling;                        /* see above */
    const struct gcnhip_gs_loss *loss;  /* NULL, or the loss epilogue below (round 5) */
} gcnhip_gs_opts;
/* Loss epilogue of the aggregation that produces the logits (round 5; CrossEntropyLoss::forward, src/seq/module.cpp:124-161,
 * and GCN::get_accuracy, gcn.cpp:83-96, inside the launch that computes Z = A^.Z0).  After its shuffle reduce a wave holds
 * the whole logit row (dim <= 64) in one lane group: max, sum of exp (left to right, the reference's order), the row's loss
 * term, the accuracy test and — training — the gradient row (softmax - onehot) / count [* grad_row_scale[r]] are computed
 * there; the launch writes `out` (the logits) as always, the gradient row, and row_terms[2r] = loss term, row_terms[2r+1] =
 * 1.f when no logit is above the true one.  gcnhip_xent_from_row_terms then adds the terms of a row list in the order
 * gcnhip_xent_fwd_rows adds them: same bits as that entry point on the stored logits, without reading the logits again.
 * Rows with truth < 0 get a zero gradient row and zero terms.  Needs f32 rows, 16-byte aligned, dim <= 64, no relu_dropout. */
typedef struct gcnhip_gs_loss {
    const int32_t *truth;               /* [rows of out] */
    float *grad; int ld_grad;           /* gradient rows (training != 0) */
    int training, count;                /* as gcnhip_xent_fwd_rows (count > 0) */
    const float *grad_row_scale;        /* NULL, or as gcnhip_xent_fwd_rows_scaled */
    float *row_terms;                   /* [2 * rows of out] */
} gcnhip_gs_loss;
int gcnhip_graphsum_ex(gcnhip_ctx *ctx, const gcnhip_graph *g, const gcnhip_gs_opts *opts, const float *in, int ld_in,
                       float *out, int ld_out, int dim);
/* Prediction epilogue of the aggregation that produces the logits: for every computed row r (all rows, or the rows of
 * `rows`) the same launch that sums the row writes
 *   pred[r] (int32) = the column of the largest logit — on a tie the LOWEST column, numpy.argmax's rule.  The reference's
 *                     accuracy test (GCN::get_accuracy, src/seq/gcn.cpp:86-93) instead counts a row as correct when no logit
 *                     is above the true one, i.e. a tie with the true class counts for it wherever the true class sits;
 *   prob[r] (f32)   = the softmax probability of that class, 1 / sum_j exp(z_j - max): the max and the left-to-right sum
 *                     of the loss epilogue above (gcnhip_gs_loss), so the sum has the bits of CrossEntropyLoss's;
 *   logp[r * ld_logp + c] (optional, may be NULL) = (z_c - max) - log(sum), the whole log-softmax row.
 * pred and prob have n_rows entries (rows outside `rows` are left untouched).  The gathered table is either f32 rows
 * `in` (16-byte aligned, ld_in % 4 == 0; scaling as in gcnhip_graphsum_ex, the factored path) or a bf16 table `in_bf16`
 * (as gcnhip_graphsum_bf16; scaling must be 0) — exactly one of the two.  out (may be NULL: the logits are not stored)
 * receives the logits themselves, bit-identical to gcnhip_graphsum_ex / gcnhip_graphsum_bf16 on the same operands.
 * dim <= 64 (the row then sits in one wave).  Separate kernels: no existing launch changes. */
int gcnhip_graphsum_predict(gcnhip_ctx *ctx, const gcnhip_graph *g, const gcnhip_rowset *rows, const float *in, const uint16_t *in_bf16,
                            int ld_in, float *out, int ld_out, int dim, int scaling, int32_t *pred, float *prob, float *logp, int ld_logp);
/* ---- label propagation and Correct & Smooth (beyond the reference: the graph and the known labels used at inference time) ----
 * Blend epilogue of the class-width aggregation, one step of either scheme:
 *   out[r, j] = min(max(alpha * sum_e coef(e) * in[col(e), j] + beta * base[r, j], lo), hi)      for every row r, j < dim
 *   pred[r]   = argmax_j out[r, j], the LOWEST j on a tie (numpy.argmax's rule); only when pred != NULL ([n_rows] int32)
 * The gather is gcnhip_graphsum_predict's (same task list, lane groups, edge order, reduction tree, split-row scratch; rows
 * longer than the split length are summed in segment order by a finalize launch that applies the same epilogue) with the
 * per-edge coefficients of the object, never the factored form: the iterate stays in one form from launch to launch.
 * f32 rows only: 1 <= dim <= 64, every ld % 4 == 0 and >= dim, 16-byte aligned tables; anything else returns -1 with a message
 * (gcnhip_last_error), never a wrong answer.  `in` has n_cols rows, base and out n_rows.  out must not be `in` (other waves
 * are still gathering it: refused); base may be `in` or any other table.  Columns [dim, ld_out) of out are not written, those
 * of base not read.  lo = -INFINITY / hi = +INFINITY: no clamp.  Deterministic (no float atomics: two launches give the same
 * bits); neither allocates nor synchronises. */
int gcnhip_graphsum_blend(gcnhip_ctx *ctx, const gcnhip_graph *g, const float *in, int ld_in, const float *base, int ld_base,
                          float *out, int ld_out, int dim, float alpha, float beta, float lo, float hi, int32_t *pred);
/* The row-local steps of Correct & Smooth (smooth.hip; a wave per row, lane j on class j: 1 <= num_classes <= 64, rows of any
 * stride).  logp: log-softmax rows as gcnhip_graphsum_predict writes them; truth: an array as gcnhip_set_truth makes (-1 outside
 * the split); all tables have n_table rows.
 * gcnhip_cs_error_rows zeroes e (n_table x ld_e floats, on ctx's stream), then for each of the n_listed rows r = d_rows[i]
 * (distinct; d_rows == NULL: rows 0 .. n_listed - 1) whose truth[r] is in [0, C) writes e[r, j] = [j == truth[r]] - expf(logp[r, j])
 * and leaves d_sigma[2] = {sum of |e| over those rows, their number}; rows with another truth, or an id outside the table,
 * contribute nothing.  The sum is deterministic (block partials added in block order by a one-block finalize launch).
 * gcnhip_cs_correct_rows: for every row r, s = (d_sigma[0] / d_sigma[1]) / sum_j |e_hat[r, j]|, replaced by 1 unless s <= 1000
 * (a zero row, inf and NaN included); g0[r, :] = the one-hot row of truth[r] where that is in [0, C), else
 * expf(logp[r, :]) + s * e_hat[r, :].  g0 must not be e_hat.  Columns past num_classes are not written. */
int gcnhip_cs_error_rows(gcnhip_ctx *ctx, const float *logp, int ld_logp, const int32_t *truth, int n_table, const int32_t *d_rows,
                         int n_listed, int num_classes, float *e, int ld_e, float *d_sigma);
int gcnhip_cs_correct_rows(gcnhip_ctx *ctx, const float *logp, int ld_logp, const float *e_hat, int ld_e, const int32_t *truth, int n_table,
                           int num_classes, const float *d_sigma, float *g0, int ld_g);
/* ---- temperature scaling and calibration error (calib.hip; beyond the reference: are the softmax probabilities to be trusted?) ----
 * Row-local passes over log-softmax rows as gcnhip_graphsum_predict writes them: a wave per row, lane j on class j
 * (1 <= num_classes <= 64, rows of any stride >= num_classes).  With l_j = logp[r, j], beta = 1 / T (0 < beta <= GCNHIP_BETA_MAX, below) and
 * p = softmax(beta . l), formed with the row maximum subtracted; entries with p_j == 0 contribute nothing (a column at -1e4
 * gives no NaN).  The listed rows are d_rows[i], i < n, or 0 .. n - 1 when d_rows == NULL (then n <= n_table); ids outside
 * [0, n_table) and, where truth is an argument, rows whose truth[r] is outside [0, C) are skipped.  Per-row values are f32;
 * sums over rows are doubles formed in a fixed order (rows in row order per wave, block partials in block order by a one-block
 * finalize launch; no float or double atomics), so two launches give the same bits.  No launch allocates or synchronises.
 * Anything else returns -1 with a message (gcnhip_last_error).
 * The domain of beta, here and in gcnhip_conformal_scores and gcnhip_attach_gather: 0 < beta <= GCNHIP_BETA_MAX = 8e37, anything
 * else (NaN included) is refused.  The kernels round s_j = beta . l_j BEFORE they take the row maximum; the largest entry of a
 * log-softmax row of at most 64 classes is at least -ln 64 = -4.16, so its product stays finite as long as beta <=
 * FLT_MAX / ln 64 = 3.4028e38 / 4.1589 = 8.18e37 — 8e37 leaves 2 % for the rounding of the row itself.  Above that every s_j of a
 * constant row is -inf, the maximum is -inf and s_j - max is NaN.  Up to the limit every output on a finite log-softmax row is
 * NaN-free: an entry whose product overflows to -inf has e_j = 0 (scaled row -inf, a true class there: nll = +inf).
 * gcnhip_calib_nll_rows: d_out[4] = {sum nll_r, sum g_r, sum h_r, rows counted}: nll_r = lse(beta . l) - beta . l_t,
 *   g_r = mu - l_t with mu = sum_j p_j l_j (d nll / d beta), h_r = sum_j p_j (l_j - mu)^2 >= 0 (d2 nll / d beta2, the centred sum).
 * gcnhip_calib_bins_rows (1 <= bins <= 64): per counted row conf = max_j p_j, pred = the largest l_j (lowest column on a tie),
 *   bin b = clamp(ceil(conf . bins) - 1, 0, bins - 1) — the (b / B, (b + 1) / B] rule of Guo et al.; d_count[b] rows, d_correct[b]
 *   those with pred == truth (int32, zeroed on the stream first, integer adds), d_conf_sum[b] the sum of conf (double).
 * gcnhip_calib_scale_rows: out_logp[r, :] = beta . l - lse(beta . l) for every listed row inside the table (no truth), and
 *   d_prob[r] = expf(max_j out_logp[r, j]) when d_prob != NULL.  out_logp may be logp (a wave holds its row before it stores);
 *   the listed rows must then be distinct. */
#define GCNHIP_BETA_MAX 8e37f
int gcnhip_calib_nll_rows(gcnhip_ctx *ctx, const float *logp, int ld, const int32_t *truth, int n_table, const int32_t *d_rows, int n,
                          int num_classes, float beta, double *d_out);
int gcnhip_calib_bins_rows(gcnhip_ctx *ctx, const float *logp, int ld, const int32_t *truth, int n_table, const int32_t *d_rows, int n,
                           int num_classes, float beta, int bins, int32_t *d_count, int32_t *d_correct, double *d_conf_sum);
int gcnhip_calib_scale_rows(gcnhip_ctx *ctx, const float *logp, int ld, int n_table, const int32_t *d_rows, int n, int num_classes, float beta,
                            float *out_logp, int ld_out, float *d_prob);
/* ---- Monte Carlo dropout (mcdropout.hip; beyond the reference: per-node uncertainty from S stochastic forwards) ----
 * The conventions of the calibration kernels above: a wave per listed row, lane j on class j (1 <= num_classes <= 64, rows of any
 * stride >= num_classes), fp contract(off), rows listed as d_rows[i], i < n, or 0 .. n - 1 when d_rows == NULL (then n <= n_table);
 * no atomics, so the bits depend on the sample sequence alone; no launch allocates or synchronises; anything refused returns -1
 * with a message naming the entry point (gcnhip_last_error).  The accumulators are indexed by LIST POSITION i (a row listed
 * twice has two independent ones): acc_f64 [n x (C + 1)] doubles, acc_votes [n x C] int32.
 * gcnhip_mc_accumulate_rows: one sample.  l = logp[d_rows[i], :] are log-softmax rows as gcnhip_graphsum_predict leaves them (after
 *   gcnhip_calib_scale_rows: the rows at T != 1, hence no beta here).  In float64: acc_f64[i (C + 1) + c] += exp(l_c);
 *   acc_f64[i (C + 1) + C] += - sum_c exp(l_c) . l_c (a class with exp(l_c) == 0 contributes 0, l_c = -inf included);
 *   acc_votes[i C + argmax_c l_c] += 1, the lowest class on a tie.  first != 0 stores instead of adding (no memset launch is
 *   needed).  An id outside [0, n_table) adds nothing (first != 0: zeros).
 * gcnhip_mc_finalize_rows: after `samples` >= 1 accumulations.  In float64 until the store: mean_prob[i, c] = acc / samples
 *   ([n x ld_mp], columns past C not written); pred[i] = its argmax, lowest class on a tie; confidence[i] = mean_prob[i, pred];
 *   entropy[i] = - sum_c mean_prob ln mean_prob (a zero contributes 0); expected_entropy[i] = acc[.., C] / samples;
 *   mutual_information[i] = max(0, entropy - expected_entropy); variation_ratio[i] = 1 - max_c votes[i, c] / samples.
 *   Outputs are f32 (int32 for pred), indexed by list position; any output pointer may be NULL. */
int gcnhip_mc_accumulate_rows(gcnhip_ctx *ctx, const float *logp, int ld, int n_table, const int32_t *d_rows, int n, int num_classes, int first,
                              double *acc_f64, int32_t *acc_votes);
int gcnhip_mc_finalize_rows(gcnhip_ctx *ctx, const double *acc_f64, const int32_t *acc_votes, int n, int num_classes, int samples, float *mean_prob,
                            int ld_mp, int32_t *pred, float *confidence, float *entropy, float *expected_entropy, float *mutual_information,
                            float *variation_ratio);
/* ---- split conformal prediction sets (conformal.hip; beyond the reference: a set of classes per node with a coverage guarantee) ----
 * The conventions of the calibration kernels above: a wave per row, lane j on class j (1 <= num_classes <= 64, rows of any stride
 * >= num_classes), fp contract(off), rows listed as d_rows[i], i < n, or 0 .. n - 1 when d_rows == NULL (then n <= n_table), ids
 * outside [0, n_table) skipped; no float atomics, so two launches give the same bits; no launch allocates or synchronises; anything
 * refused returns -1 with a message naming the entry point (gcnhip_last_error).  p = softmax(beta . l) of l = logp[r, :] as above.
 * rank_j = #{k : l_k > l_j, or l_k == l_j and k < j}, on the f32 inputs: exact, ties to the lower class as in predict.
 * gcnhip_conformal_scores: out[r, j] for every listed row r, j < num_classes (columns past it and unlisted rows are not written;
 *   out is indexed by table row so that gcnhip_graphsum_blend can gather it).  method 0 (LAC): 1 - p_j.  method 1 (APS,
 *   non-randomised, inclusive): cum_j + lam . max(0, rank_j + 1 - k_reg), cum_j = the sum of p_k over rank_k <= rank_j in one fixed
 *   tree of at most six additions per result, clamped to 1, and exactly 1.0f for the last-ranked class (a threshold >= 1 gives the
 *   full set whatever the last ulp of sum p); lam >= 0 and k_reg >= 0 are the RAPS penalty, lam = 0 plain APS.
 * gcnhip_conformal_true_scores: d_score[i] = table[r, truth[r]] for list position i, or -1.f when r is outside the table or
 *   truth[r] outside [0, num_classes) (scores are never negative); repeats are scored as often as listed.
 * gcnhip_conformal_sets_rows: class j is in the set of row r iff table[r, j] <= d_thresh[j] (d_thresh [num_classes]; +inf allowed,
 *   NaN is the caller's to refuse).  By list position: d_bits [n x ceil(num_classes / 32)] (bit (j & 31) of word j >> 5; zero for a
 *   skipped id) and d_size [n] (-1 for a skipped id); either may be NULL.  d_counts (may be NULL; int32 [4 + 3 C + 1], zeroed on the
 *   stream first, integer adds only) = {rows in the table, labelled rows, covered, empty sets | size_hist [C + 1] | class_support
 *   [C] | class_covered [C]}; truth may be NULL (then no row is labelled). */
int gcnhip_conformal_scores(gcnhip_ctx *ctx, const float *logp, int ld, int n_table, const int32_t *d_rows, int n, int num_classes, float beta,
                            int method, float lam, int k_reg, float *out, int ld_out);
int gcnhip_conformal_true_scores(gcnhip_ctx *ctx, const float *table, int ld, const int32_t *truth, int n_table, const int32_t *d_rows, int n,
                                 int num_classes, float *d_score);
int gcnhip_conformal_sets_rows(gcnhip_ctx *ctx, const float *table, int ld, int n_table, const int32_t *d_rows, int n, int num_classes,
                               const float *d_thresh, const int32_t *truth, uint32_t *d_bits, int32_t *d_size, int32_t *d_counts);
/* ---- ranking metrics (ranking.hip; beyond the reference: per-class ROC-AUC and average precision without a threshold) ----
 * Key: the order-preserving u32 image of an f32 score — -0.0 is +0.0 first; with b its bits, ~b when the sign bit is set, else
 * b | 0x80000000.  Non-NaN scores compare as their keys do; 0xFFFFFFFF is no score's key and is the padding sentinel; a NaN score
 * gets no key.  None of the entry points is part of a captured epoch; no float atomics, so two launches give the same bits; no
 * launch allocates or synchronises; anything refused returns -1 with a message naming the entry point (gcnhip_last_error).
 * gcnhip_rank_keys: table f32 [n_table x ld], the listed rows d_rows[i], i < n (NULL: rows 0 .. n - 1, then n <= n_table; repeats
 *   count as often as listed), the classes [c0, c1) of num_classes <= ld.  Truth is EITHER int32 per table row as gcnhip_set_truth
 *   makes it (class c's positives are the rows with truth == c, its negatives the other rows with a truth in [0, num_classes); a
 *   row with any other truth is in no class and counted in *d_unlabelled) OR multi-hot bit rows (bit (c & 31) of word
 *   truth_bits[r * words_per_row + (c >> 5)]; every row is labelled).  pos_keys / neg_keys u32 [(c1 - c0) x stride], stride >=
 *   max(n, 1): entry i of column c - c0 = the key of listed row i when it is a positive (resp. negative) of class c, else the
 *   sentinel; entries [n, stride) are not written.  d_pos / d_neg / d_invalid int32 [c1 - c0] (zeroed on the stream first, integer
 *   adds): positives, negatives, and labelled rows whose score is NaN (in neither).  d_unlabelled (may be NULL) int32 [1]: listed
 *   rows without a usable truth, an id outside [0, n_table) among them.  Reads and writes both coalesce (an LDS tile transposes).
 * gcnhip_sort_segments_u32: sorts `segments` runs of n keys ascending in place, run s at keys + s * stride; scratch: a table of the
 *   same extent (may be NULL when n <= GCNHIP_SORT_TILE).  The result always lands in keys.  Entries [n, stride) of a run are
 *   neither read nor written, in either table.  A bitonic network per tile of GCNHIP_SORT_TILE keys (256 threads, 16 keys each:
 *   strides below 16 in registers, below 1024 by cross-lane moves, above through LDS), then ceil(log2(n / GCNHIP_SORT_TILE))
 *   merge-path passes between the two tables.  0 <= n <= 2^24, segments >= 1, 64-bit offsets.  gcnhip_sort_tile() returns the tile.
 * gcnhip_rank_stats: sorted tables as above with the valid lengths d_pos[c] / d_neg[c] (clamped to [0, n]; the sentinel is never
 *   compared with).  For every class c < segments: d_u2[c] = sum over its positives of #{negatives with a smaller key} +
 *   #{negatives with a key not larger} (int64, exact), d_ap_sum[c] = sum over its positives of TP_ge / (TP_ge + FP_ge) with TP_ge /
 *   FP_ge the positives / negatives whose key is not smaller (float64; per thread in index order, then one fixed tree per block,
 *   then the blocks in order).  A class without positives gives zeros.  d_work: segments * GCNHIP_RANK_STATS_BLOCKS * 16 bytes,
 *   8-byte aligned. */
#define GCNHIP_SORT_TILE 4096
#define GCNHIP_RANK_STATS_BLOCKS 32
int gcnhip_sort_tile(void);
int gcnhip_rank_keys(gcnhip_ctx *ctx, const float *table, int ld, int n_table, const int32_t *d_rows, int n, int c0, int c1, int num_classes,
                     const int32_t *truth, const uint32_t *truth_bits, int words_per_row, uint32_t *pos_keys, uint32_t *neg_keys, int64_t stride,
                     int32_t *d_pos, int32_t *d_neg, int32_t *d_invalid, int32_t *d_unlabelled);
int gcnhip_sort_segments_u32(gcnhip_ctx *ctx, uint32_t *keys, uint32_t *scratch, int n, int segments, int64_t stride);
int gcnhip_rank_stats(gcnhip_ctx *ctx, const uint32_t *pos_keys, const uint32_t *neg_keys, int64_t stride, int n, int segments, const int32_t *d_pos,
                      const int32_t *d_neg, void *d_work, int64_t *d_u2, double *d_ap_sum);
/* ---- multi-label decision thresholds (thresholds.hip; beyond the reference: one cut per class instead of the training rule z > 0) ----
 * Rule: with a threshold t[c], class c is predicted for a row exactly when its logit z is not NaN and key(z) >= key(t[c]), key()
 * as above — z >= t[c] in exact real comparison (-0.0 == +0.0), made on the integer keys, so denormal logits and thresholds
 * behave the same whatever the float denormal mode.  A NaN threshold has no key: its class is predicted for no row.
 * gcnhip_threshold_scan: the sorted tables and valid lengths of gcnhip_rank_stats (d_pos[c] / d_neg[c] clamped to [0, n]).  For
 *   every class c < segments with P positives and N negatives the candidates are the keys k of its positives; at a cut TP =
 *   #{pos >= k}, FP = #{neg >= k}, FN = P - TP (exact integers), and in float64 without contraction w = beta * beta, num =
 *   (1.0 + w) * TP, den = num + w * FN + FP, F = num / den.  The winner has the largest F, among equal F the largest key.
 *   d_thr[c] = the float of the winning key, d_counts int32 [3 * segments] = {TP | FP | FN} at it, d_f[c] = its F, d_defined[c] =
 *   1.  P == 0: d_defined[c] = 0, d_thr[c] = 0.0f, TP = FN = 0, FP = #{neg >= key(0)}, F = 0.  The max over (F, key) commutes and
 *   associates: every reduction order gives the same bits, two launches give the same bits; no atomics.  Grid
 *   (GCNHIP_THRESHOLD_SCAN_BLOCKS, segments) and a fold launch.  d_work: segments * GCNHIP_THRESHOLD_SCAN_BLOCKS * 16 bytes,
 *   8-byte aligned (the work block of gcnhip_rank_stats serves).  Refused with a message: beta not finite or <= 0, n > 2^24,
 *   stride < max(n, 1), segments outside 1..65535, a misaligned work block. */
#define GCNHIP_THRESHOLD_SCAN_BLOCKS 32
int gcnhip_threshold_scan(gcnhip_ctx *ctx, const uint32_t *pos_keys, const uint32_t *neg_keys, int64_t stride, int n, int segments, const int32_t *d_pos,
                          const int32_t *d_neg, double beta, void *d_work, float *d_thr, int32_t *d_counts, double *d_f, int32_t *d_defined);
/* gcnhip_bce_predict_rows and gcnhip_bce_class_counts_rows (below) with the rule above in place of z > 0: thr f32 [num_classes] on
 * the device.  Arguments, layouts, limits (1 <= num_classes <= 256) and determinism are theirs; prob stays sigmoid(z_c).  Neither
 * reads thr on the host: a caller that must refuse a NaN threshold checks its own copy. */
int gcnhip_bce_predict_rows_thr(gcnhip_ctx *ctx, const float *logits, int ld, const int32_t *d_rows, int n_rows, int num_classes, const float *thr,
                                uint32_t *bits, int words_per_row, float *prob, int ld_prob);
int gcnhip_bce_class_counts_rows_thr(gcnhip_ctx *ctx, const float *logits, int ld, const uint32_t *truth_bits, int words_per_row, const int32_t *d_rows,
                                     int n, int num_classes, const float *thr, int32_t *counts);
/* ---- node embeddings (embed.hip; beyond the reference: what a GCN learns, taken out without leaving the device) ----
 * All entry points read an f32 table [n_table x ld] with 1 <= dim <= 256 and dim <= ld, rows of any stride and alignment;
 * columns [dim, ld) are never read as values.  Score of rows (q, c): their f32 dot product (inv_norm == NULL, metric "dot"),
 * else (dot . inv_norm[q]) . inv_norm[c] (metric "cosine").  No launch allocates or synchronises; two launches give the same
 * bits; anything else returns -1 with a message (gcnhip_last_error).
 * gcnhip_embed_inv_norms: inv_norm[r] = 1 / sqrt(sum_j x_rj^2) in f32; an all-zero row (ReLU makes them) gives exactly 0.
 * gcnhip_topk_rows: for each of the nq listed query rows (q_rows: device int32, repeats allowed; a row outside the table gets
 *   the empty answer) the k best of all n_table candidate rows, without the query's own row when exclude_self != 0.  Order:
 *   score descending, on equal scores the smaller id first, id = row_id[c] (row_id == NULL: c itself) — a total order, so the
 *   answer does not depend on how the candidates are cut into chunks.  out_id [nq x k] int32 holds ids, out_score [nq x k] f32;
 *   1 <= k <= 64; with fewer than k candidates the remaining slots are -1 / -inf.  chunk_rows: candidate rows per workgroup,
 *   0 = the library's choice (gcnhip_topk_plan reports it).  The per-chunk lists go through `scratch`, device memory of the
 *   caller: gcnhip_topk_plan's *scratch_bytes holds every query at once; with less, down to *scratch_bytes_min (one tile of 64
 *   queries), the queries are answered in batches of as many tiles as fit — more launches, the same bits.  launches: 3 = the
 *   product launch and the merge launch (the answer); 1 or 2 = only the one or the other, for timing them apart.
 * gcnhip_pair_scores: out[i] = score(src[i], dst[i]) for n_pairs listed row pairs (device int32; src[i] == dst[i] allowed); a
 *   row outside the table gives NaN.
 * gcnhip_embed_rows: out[i, :dim] = table[d_rows[i], :dim], times inv_norm[d_rows[i]] when inv_norm != NULL (d_rows == NULL:
 *   row i, n <= n_table); the export gather, so that only the asked rows cross to the host. */
int gcnhip_embed_inv_norms(gcnhip_ctx *ctx, const float *table, int ld, int n_table, int dim, float *inv_norm);
int gcnhip_topk_plan(int n_table, int nq, int k, int chunk_rows, int *chunk_rows_used, int *n_chunks, size_t *scratch_bytes,
                     size_t *scratch_bytes_min);
int gcnhip_topk_rows(gcnhip_ctx *ctx, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *row_id,
                     const int32_t *q_rows, int nq, int k, int exclude_self, int chunk_rows, void *scratch, size_t scratch_bytes,
                     int launches, int32_t *out_id, float *out_score);
int gcnhip_pair_scores(gcnhip_ctx *ctx, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *src,
                       const int32_t *dst, int n_pairs, float *out);
int gcnhip_embed_rows(gcnhip_ctx *ctx, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *d_rows,
                      int n, float *out, int ld_out);
/* ---- k-means on the rows of a table (kmeans.hip; beyond the reference: grouping what a GCN learns, where it lies) ----
 * The table contract of the embedding calls.  d_rows: a device int32 list of n rows, repeats allowed, NULL: rows 0 .. n - 1
 * (then n <= n_table); a list position whose row is outside the table takes no part.  The row used is x^ = x . inv_norm[r]
 * (inv_norm == NULL: x).  centers: f32 [k x ldm], 1 <= k <= 256, dim <= ldm; cn[c]: f32 squared norm of centre c.  No launch
 * allocates or synchronises, none uses a float atomic; every output's bits are a function of the arguments' contents alone
 * (not of launch geometry, scratch size or batching); anything else returns -1 with a message (gcnhip_last_error).
 * gcnhip_kmeans_plan: the bytes of device scratch gcnhip_kmeans_update takes (*update_bytes: one batch; down to
 *   *update_bytes_min: more launches, the same bits) and gcnhip_kmeans_seed needs (*seed_bytes); each may be NULL.
 * gcnhip_kmeans_assign: d(i, c) = cn[c] - 2 . (dot_f32(T[r], M[c]) . inv_norm[r]) on the exact-f32 MFMA; assign[i] = argmin_c d,
 *   the lowest c on equal d; dist2[i] = max(0, |x^|^2 + d(i, assign[i])) with |x^|^2 = (sumsq_f32(T[r]) . inv_norm[r]) . inv_norm[r];
 *   *moved (device int32) = positions with assign[i] != prev[i] (prev == NULL: n).  A row outside the table: assign -1, dist2 NaN.
 *   cn is an INPUT (gcnhip_kmeans_update writes it).  The table is read once whatever k is.
 * gcnhip_kmeans_update: members of centre c = the positions with assign == c whose row is in the table, in ascending position.
 *   sum[c, j] = float64 sum over them of (double)(x[r, j] . inv_norm[r]) (the product rounded to f32 first), added member by
 *   member inside segments of 128 members and segment by segment; centers[c, j] = (float)(sum / count); an empty centre keeps
 *   its row.  sizes[c] int32; cn[c] = (float)(the float64 sum over j, in order, of centers[c, j]^2), of kept rows too (n == 0:
 *   the norms of the given centres); *inertia (device double, may be NULL) = the sum of dist2 over the members (dist2 NULL: 0),
 *   per 1024 positions by a fixed tree, then over those partials by a fixed tree.
 * gcnhip_kmeans_seed: k-means++ by an exponential race.  w(i, t) = word 0 of Philox4x32-10(counter {i, 0, t, 0x6B6D2B2B}, key
 *   {lo32, hi32 of stream_seed}).  seed_pos[0] = (uint64(w(0, 0)) . n) >> 32; step t = 1 .. k - 1: d2min[i] = min(d2min[i],
 *   sum_j (x^_ij - M[t - 1, j])^2) in f32 by differences; key_i = -log((w(i, t) + 0.5) . 2^-32) / d2min[i] in float64, +inf where
 *   d2min == 0; seed_pos[t] = the position of the smallest key, the lowest position on a tie; every key +inf: the lowest
 *   position whose row is in the table.  centers[t] = the chosen row, scaled.  All k steps are enqueued back to back.
 * gcnhip_contingency_rows: counts [k x num_classes] int32, counts[a * C + y] = positions with assign[i] = a and truth[r] = y
 *   (truth: [n_truth] by row, r = d_rows[i] or i); *skipped = positions with a negative assignment, a row outside [0, n_truth)
 *   or a truth outside [0, C).  num_classes <= 64. */
int gcnhip_kmeans_plan(int n, int k, int dim, size_t *update_bytes, size_t *update_bytes_min, size_t *seed_bytes);
int gcnhip_kmeans_assign(gcnhip_ctx *ctx, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *d_rows,
                         int n, const float *centers, int ldm, const float *cn, int k, const int32_t *prev, int32_t *assign, float *dist2,
                         int32_t *moved);
int gcnhip_kmeans_update(gcnhip_ctx *ctx, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *d_rows,
                         int n, const int32_t *assign, const float *dist2, int k, float *centers, int ldm, int32_t *sizes, float *cn,
                         double *inertia, void *scratch, size_t scratch_bytes);
int gcnhip_kmeans_seed(gcnhip_ctx *ctx, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *d_rows,
                       int n, int k, uint64_t stream_seed, float *centers, int ldm, int32_t *seed_pos, void *scratch, size_t scratch_bytes);
int gcnhip_contingency_rows(gcnhip_ctx *ctx, const int32_t *assign, const int32_t *truth, int n_truth, const int32_t *d_rows, int n, int k,
                            int num_classes, int32_t *counts, int32_t *skipped);
/* ---- silhouette widths of a labelling of a table's rows (silhouette.hip; beyond the reference: how well a grouping fits) ----
 * The table contract and the row lists of the k-means calls.  labels: device int32 [n] by list position.  The POINTS are the
 * positions with a label in [0, k), 1 <= k <= 256, and a row in the table; two positions that name one row are two points.
 * d(i, j) = sqrtf(max(0, (xn_i + xn_j) - 2 . dot_f32(x^_i, x^_j))) with x^ = x . inv_norm[r] rounded to f32 (inv_norm == NULL: x),
 * xn = (sumsq_f32(T[r]) . inv_norm[r]) . inv_norm[r] as gcnhip_kmeans_assign forms it, the dot on the exact-f32 MFMA, sqrtf
 * correctly rounded.  No launch allocates or synchronises, none uses a float atomic; every output's bits are a function of the
 * arguments' contents alone (not of launch geometry, scratch size or batching); anything else returns -1 with a message.
 * gcnhip_silhouette_plan: the bytes of device scratch gcnhip_silhouette_sums takes for every position in one batch (*bytes) and
 *   the least it works with (*bytes_min: batches of 64 positions, more launches, the same bits); each may be NULL.  No GPU.
 * gcnhip_silhouette_sums: sums [n x k] float64, sums[i . k + c] = S(i, c) = the sum of d(i, j) over the points j of label c, the
 *   pair (i, i) left out by POSITION.  The members of a label are taken in ascending position, in segments of 512 members; inside
 *   a segment in tiles of 64: of a tile, member m goes to partial (m mod 16) / 4, each partial a float64 chain in ascending m
 *   that runs on through the segment's tiles; the segment's sum is (p0 + p1) + (p2 + p3); the segments of a label are added in
 *   order from +0.  The row of a position that is no point is written as 0.  sizes [k] int32: the points of every label.
 * gcnhip_silhouette_rows: row-local, from sums and sizes.  With A = labels[i]: a[i] = S(i, A) / (n_A - 1), 0 when n_A = 1;
 *   b[i] = the least S(i, c) / n_c over c != A with n_c > 0, neighbor[i] that c, the lowest on equal means; s[i] = (b - a) /
 *   max(a, b), 0 when n_A = 1 or max(a, b) = 0 — each ONE float64 expression.  Fewer than two non-empty labels: b = 0, s = 0,
 *   neighbor = -1.  A position that is no point: s = a = b = NaN, neighbor = -1.  cluster_sum [k] and *total (device float64):
 *   the sums of s over the points of a label and over all points; thread t of 256 adds positions t, t + 256, .. in order, then a
 *   fixed tree.  counts (device int32 [3]) = {points, positions that are no point, non-empty labels}. */
int gcnhip_silhouette_plan(int n, int k, int dim, size_t *bytes, size_t *bytes_min);
int gcnhip_silhouette_sums(gcnhip_ctx *ctx, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *d_rows,
                           int n, const int32_t *labels, int k, double *sums, int32_t *sizes, void *scratch, size_t scratch_bytes);
int gcnhip_silhouette_rows(gcnhip_ctx *ctx, const double *sums, const int32_t *labels, const int32_t *sizes, const int32_t *d_rows,
                           int n_table, int n, int k, double *s, double *a, double *b, int32_t *neighbor, double *cluster_sum,
                           double *total, int32_t *counts);
/* ---- principal components of the rows of a table (pca.hip; beyond the reference: the coordinates of what a GCN learns) ----
 * The table contract and the row lists of the k-means calls: a list position whose row is outside the table is skipped and
 * leaves a NaN row in a projection.  x_i[a] = T[r][a] . inv_norm[r] rounded to f32 (inv_norm == NULL: T[r][a]).  No launch
 * allocates or synchronises, none uses a float atomic; every output's bits are a function of the arguments' contents alone.
 * The list is cut into parts of 1024 positions; a part's partial is accumulated in ascending position, the partials are added
 * from +0 in ascending part order; a call handles as many parts per launch as its scratch holds.
 * gcnhip_pca_plan: *bytes_full = max(ceil(n / 1024), 1) . T . 2048 and *bytes_min = T . 2048 bytes of device scratch for either
 *   call below, T = t (t + 1) / 2, t = ceil(dim / 16); each may be NULL.
 * gcnhip_pca_mean: mean[a] (device float64 [dim]) = (the float64 sum of (double)x_i[a] over the valid positions) / count;
 *   *count (device int32) = the valid positions; count == 0 gives NaN.
 * gcnhip_pca_scatter: scatter (device float64 [dim x dim]), S[a][b] = sum_i c_ia . c_ib with c_ia = (double)x_i[a] - mean[a]
 *   (mean == NULL: x, the uncentred Gram matrix), products and sums in float64 on the f64 MFMA, four consecutive positions per
 *   instruction.  Tile pairs on or above the diagonal are computed and mirrored: S is symmetric bit for bit.
 * gcnhip_pca_project: out[i][j] (f32 [n x ldy]) = (float)(scale[j] . sum_a c_ia . basis[a . ldv + j]) for j < k <= dim, one
 *   float64 fma chain in ascending a; basis: device float64 [dim x ldv]; scale: device float64 [k] or NULL (no factor). */
int gcnhip_pca_plan(int n, int dim, size_t *bytes_full, size_t *bytes_min);
int gcnhip_pca_mean(gcnhip_ctx *ctx, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *d_rows, int n,
                    double *mean, int32_t *count, void *scratch, size_t scratch_bytes);
int gcnhip_pca_scatter(gcnhip_ctx *ctx, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *d_rows,
                       int n, const double *mean, double *scatter, void *scratch, size_t scratch_bytes);
int gcnhip_pca_project(gcnhip_ctx *ctx, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *d_rows,
                       int n, const double *mean, const double *basis, int ldv, int k, const double *scale, float *out, int ldy);
/* ---- label structure of the graph (structure.hip; beyond the reference: WHERE on the graph a labelling agrees with itself) ----
 * g: an adjacency object with its stored rows (self loop included, repeated entries counted as often as stored, one-way entries
 * allowed).  lab: device int32, one entry per COLUMN of g; label x is known when 0 <= x < num_classes, 1 <= num_classes <= 64.
 * d_rows: a device int32 list of n rows, repeats counted as often as listed, NULL: position i is row i; a position whose row is
 * outside [0, n_rows) counts in *skipped and nowhere else.  For position i with row v and its non-loop entries u (u != v):
 * deg[i] = their number; with lab[v] known, known[i] = those with lab[u] known, same[i] = those of them with lab[u] == lab[v],
 * mix[lab[v] * C + lab[u]] += 1 for each of them and class_rows[lab[v]] += 1; with lab[v] unknown known[i] = same[i] = 0.
 * deg / same / known: int32 [n] by list position, each may be NULL; mix: int64 [C x C], may be NULL; class_rows: int64 [C];
 * totals: int64 [8] = {listed rows in range, labelled rows, rows with known > 0, sum deg, sum known, sum same, self entries seen,
 * ratio_sum}, ratio_sum = the sum over rows with known > 0 of floor(same . 2^32 / known) in 64-bit integers (node homophily =
 * ratio_sum / 2^32 / rows with known > 0); skipped: one int64.  All device memory; the call zeroes them itself, allocates
 * nothing, synchronises nothing, and adds with integer atomics only: the same bits from every launch.
 * gcnhip_nbr_agreement_ex: the same launch with the lane group per row (0: by the mean stored row length; 4, 16, 64) and the
 * number of walked entries after which a wave empties its workgroup's LDS histogram (0: 2^26, the largest allowed) given.
 * gcnhip_strata_counts: pred and truth are indexed by ROW ([n_truth]), deg / same / known by list position.  db = 0 when
 * deg <= 0, else 1 + floor(log2 deg); ab = bins when known <= 0, else min(bins - 1, floor(same . bins / known)) in 64-bit
 * integers; strata: int64 [32 x (bins + 1) x 2], strata[(db * (bins + 1) + ab) * 2 + {0, 1}] = the positions whose truth is
 * known and, of them, those with pred == truth; *unlabelled = the positions whose truth is outside [0, num_classes); a position
 * whose row is outside [0, n_truth) counts nowhere.  1 <= bins <= 32.
 * Refused with -1 and a message (gcnhip_last_error) before any launch: a NULL required pointer, n < 0, num_classes outside
 * 1..64, bins outside 1..32. */
int gcnhip_nbr_agreement(gcnhip_ctx *ctx, const gcnhip_graph *g, const int32_t *lab, int num_classes, const int32_t *d_rows, int n,
                         int32_t *deg, int32_t *same, int32_t *known, int64_t *mix, int64_t *class_rows, int64_t *totals, int64_t *skipped);
int gcnhip_nbr_agreement_ex(gcnhip_ctx *ctx, const gcnhip_graph *g, const int32_t *lab, int num_classes, const int32_t *d_rows, int n,
                            int32_t *deg, int32_t *same, int32_t *known, int64_t *mix, int64_t *class_rows, int64_t *totals, int64_t *skipped,
                            int group, int64_t flush_every);
int gcnhip_strata_counts(gcnhip_ctx *ctx, const int32_t *deg, const int32_t *same, const int32_t *known, const int32_t *pred,
                         const int32_t *truth, int n_truth, const int32_t *d_rows, int n, int num_classes, int bins, int64_t *strata,
                         int64_t *unlabelled);
/* ---- reach of a seed set and connected components (reach.hip; beyond the reference: HOW FAR a row is from what it learns from) ----
 * g: a SQUARE adjacency object with its stored rows (one-way, repeated and unsorted entries allowed; an entry outside the graph is
 * passed over).  All integer work: the same bits from every launch, lane group and batching.
 * gcnhip_hop_distance: d_seeds: a device int32 list of n_seeds rows, repeats allowed; a seed outside [0, n_rows) counts in *skipped
 * and nowhere else.  dist: device int32 [n_rows]: 0 for a seed, else 1 + min dist[u] over the stored entries u != v of ROW v (row v
 * gathers from the entries it lists; no transpose is used), -1 when no seed reaches v or none within max_hops (0: no limit).
 * nearest: device int32 [n_rows], may be NULL: the lowest row index among the seeds at distance dist[v] from v, -1 with dist -1.
 * scratch: device int64 [GCNHIP_REACH_SCRATCH].  HOST outputs: *levels = the largest distance assigned, level_counts[d] = the rows
 * with distance d for d < capacity (the rest of [0, capacity) zero; may be NULL with capacity 0), *skipped.  One level is one
 * launch; no launch waits on another workgroup.  UNLIKE most entry points here the call SYNCHRONISES the context's stream: once
 * after the seeding and once per levels_per_sync level launches, to read the counters of newly reached rows and stop at the first
 * empty level (launches behind it change nothing).  It allocates nothing.
 * gcnhip_hop_distance_ex: the same with the lane group per row (0: by the mean stored row length; 4, 16, 64) and levels_per_sync
 * (1..64; the plain call uses 8) given.
 * gcnhip_components: comp: device int32 [n_rows] = the smallest row index in the row's WEAKLY connected component (every stored
 * entry u != v joins u and v, whichever row stores it).  Min-label hooking with atomicMin and pointer jumping; the call ends after
 * a round whose hooking pass found equal labels on every stored entry.  *rounds (host) = the rounds run, that one included.
 * scratch as above.  SYNCHRONISES the stream once per round (4 bytes read back); allocates nothing.
 * gcnhip_component_counts: comp and mark (int32 flag per row, NULL: no row is marked) [n_rows]; size / marked: device int32
 * [n_rows], size[r] = rows with comp == r, marked[r] = those with mark != 0; totals: device int64 [6] = {rows with comp in range,
 * components, largest size, components without a marked row, rows in those components, marked rows}.  Zeroes its outputs,
 * allocates nothing, synchronises nothing.
 * gcnhip_distance_strata: dist, nearest (may be NULL), pred (may be NULL), truth: device int32 [n_rows], indexed by ROW; d_rows: n
 * positions (NULL: position i is row i), a row outside [0, n_rows) counts nowhere.  Bucket b = dist for 0 <= dist < hops, hops
 * for dist >= hops, hops + 1 for dist < 0.  strata: device int64 [(hops + 2) x 4], per bucket {positions listed, those whose truth
 * is known (0 <= truth < num_classes), of those pred == truth, of those the nearest row has a known truth equal to theirs};
 * *unlabelled (device int64) = the listed positions without a known truth.  Zeroes its outputs, allocates nothing, synchronises
 * nothing.
 * Refused with -1 and a message (gcnhip_last_error) before any launch: a NULL required pointer, a negative count, a non-square
 * object, a lane group other than 0 / 4 / 16 / 64, levels_per_sync outside 1..64, hops outside 1..32, num_classes < 1. */
#define GCNHIP_REACH_SCRATCH 64
int gcnhip_hop_distance(gcnhip_ctx *ctx, const gcnhip_graph *g, const int32_t *d_seeds, int n_seeds, int max_hops, int32_t *dist,
                        int32_t *nearest, int64_t *scratch, int *levels, int64_t *level_counts, int capacity, int64_t *skipped);
int gcnhip_hop_distance_ex(gcnhip_ctx *ctx, const gcnhip_graph *g, const int32_t *d_seeds, int n_seeds, int max_hops, int32_t *dist,
                           int32_t *nearest, int64_t *scratch, int *levels, int64_t *level_counts, int capacity, int64_t *skipped, int group,
                           int levels_per_sync);
int gcnhip_components(gcnhip_ctx *ctx, const gcnhip_graph *g, int32_t *comp, int64_t *scratch, int *rounds);
int gcnhip_component_counts(gcnhip_ctx *ctx, const int32_t *comp, const int32_t *mark, int n_rows, int32_t *size, int32_t *marked,
                            int64_t *totals);
int gcnhip_distance_strata(gcnhip_ctx *ctx, const int32_t *dist, const int32_t *nearest, const int32_t *pred, const int32_t *truth,
                           int n_rows, const int32_t *d_rows, int n, int num_classes, int hops, int64_t *strata, int64_t *unlabelled);
/* ---- explaining a logit (explain.hip; beyond the reference: WHY the model answers what it answers) ----
 * The network is Z = A^ . (ReLU(A^ . X . W1) . W2) without bias, so with the ReLU gates of a forward fixed a logit is a plain sum
 * that splits without approximation ("gradient x input" is a decomposition here).  One query = a row v of the adjacency object and
 * a class c; e_1 .. e_d are the stored edges of row v in stored order (gcnhip_graph_arrays), u_i = col(e_i), a_i = A^[v, u_i],
 * g_i[k] = (H1[u_i, k] > 0) read from the table passed in, S = A^ . X:
 *   logit   z      = sum_i a_i sum_k H1[u_i, k] W2[k, c]
 *   nbr_i          = a_i sum_k H1[u_i, k] W2[k, c]                      one per stored edge (a repeated edge: two entries)
 *   hid_k          = W2[k, c] sum_i a_i H1[u_i, k]                      [h]
 *   feat_f         = sum_i a_i sum_k g_i[k] W2[k, c] W1[f, k] S[u_i, f] [F]
 * All take device lists q_row / q_class [nq] (repeats allowed), an f32 H1 table [g->n_cols x ld_h1] with 1 <= h <= 256 (any stride
 * and alignment; columns [h, ld) are never read as values), W2 [h x C] with its own stride, W1 [F x h], and `scaling` with
 * gcnhip_graphsum_ex's meaning: 0 = plain tables, a_i = coef[e_i]; 1 = the factored form, where row r of H1 / S / the feature
 * object carries dinv[r] and a_i . H1[u_i] = dinv_row[v] . H1'[u_i], a_i . S[u_i] = dinv_row[v] . S'[u_i], a_i . A^[u_i, w] . x(w) =
 * dinv_row[v] . dinv2_row[u_i] . X'[w].  The query lists are copied to the host and checked first (this synchronises the stream):
 * a row outside the object or a class outside [0, C) is an argument error (-1, gcnhip_last_error) before any launch.  No float
 * atomics, no allocation inside a launch; two launches give the same bits, and the result of a query does not depend on which
 * other queries are in the launch.
 * gcnhip_explain_hops: one launch writes logit [nq], hidden [nq x ld_out] (columns < h) and the neighbour shares: nbr_val[nbr_ptr[q]
 *   + i] = nbr_i, nbr_row[nbr_ptr[q] + i] = u_i.  nbr_ptr [nq] is the exclusive scan of the queried rows' lengths, made by the caller
 *   and checked against the object (nbr_capacity = entries of nbr_row / nbr_val).  Any degree.
 * gcnhip_explain_features_agg: feat [nq x ld_f] from dense rows of S [g->n_cols x ld_s]: per query the product [F x d] . [d x h] of
 *   gathered S rows with the gated rows r_i[k] = a_i g_i[k] W2[k, c], folded row-wise with W1 — 2 d F h flops, d F 4 gathered bytes.
 * gcnhip_explain_features_walk: the same numbers from a feature object in CSR (sparse, or dense) by the two-hop walk i -> w in
 *   row(u_i) -> non-zeros (f, x), adding a_i A^[u_i, w] x . (W1[f, :] . r_i) in that order, one lane adding; needs a square adjacency
 *   object and at most 40 896 feature columns (a neighbour's inner sum sits in LDS: the sum is d + D additions deep, as _agg's).
 * gcnhip_explain_abs_colsum: acc[q_class[q] * F + f] += |feat[q, f]| in float64 with the rows taken in order, count[class] += 1
 *   (int32); batches accumulate in call order; the caller zeroes acc and count.  1 <= C <= 256. */
int gcnhip_explain_hops(gcnhip_ctx *ctx, const gcnhip_graph *g, const int32_t *q_row, const int32_t *q_class, int nq, const float *h1,
                        int ld_h1, int h, const float *w2, int ld_w2, int num_classes, int scaling, float *logit, float *hidden,
                        int ld_out, const int32_t *nbr_ptr, int32_t *nbr_row, float *nbr_val, int64_t nbr_capacity);
int gcnhip_explain_features_agg(gcnhip_ctx *ctx, const gcnhip_graph *g, const int32_t *q_row, const int32_t *q_class, int nq,
                                const float *h1, int ld_h1, int h, const float *w2, int ld_w2, int num_classes, const float *w1,
                                int ld_w1, int n_features, const float *s, int ld_s, int scaling, float *feat, int ld_f);
int gcnhip_explain_features_walk(gcnhip_ctx *ctx, const gcnhip_graph *g, const gcnhip_feat *x, const int32_t *q_row,
                                 const int32_t *q_class, int nq, const float *h1, int ld_h1, int h, const float *w2, int ld_w2,
                                 int num_classes, const float *w1, int ld_w1, int scaling, float *feat, int ld_f);
int gcnhip_explain_abs_colsum(gcnhip_ctx *ctx, const float *feat, int ld_f, const int32_t *q_class, int nq, int n_features,
                              int num_classes, double *acc, int32_t *count);
/* ---- new nodes attached to a trained graph (attach.hip; beyond the reference, which scores only the nodes it was built with) ----
 * A gather for m rows that are not rows of an adjacency object, from two f32 tables read where they lie:
 *   out[i, 0:dim] = epilogue( sum_{e in [d_ptr[i], d_ptr[i+1])} d_coef[e] * row(d_col[e]) ),   i < m
 *   row(c) = table_a[c, :] for c < n_a,   table_b[c - n_a, :] for n_a <= c < n_a + m
 * d_ptr [m + 1], d_col / d_coef [d_ptr[m]] are device arrays; the tables have row strides of their own (ld_a, ld_b >= dim, any
 * alignment: rows that are 16-byte aligned in both tables are read in 16-byte pieces, others 4 bytes at a time, with the same
 * bits); 1 <= dim <= 256; out [m x ld_out] must be neither table.  A row without edges is a zero row.
 * epilogue 0: none.  1: ReLU (v > 0 ? v : 0).  2: predict (dim <= 64 only, otherwise -1 and a message) — d_pred[i] = the column
 * of the largest sum, the LOWEST on a tie; d_prob[i] = its softmax probability; d_logp (may be NULL) [i * ld_logp + c] = the
 * log-softmax row of beta . z, all three by the statements of gcnhip_graphsum_predict, followed at beta != 1 by those of
 * gcnhip_calib_scale_rows on that row (a model temperature T is beta = 1 / T, 0 < beta <= GCNHIP_BETA_MAX; the sum of the rescaled row runs
 * left to right here and in a shuffle tree there, so the two agree within the rounding of one sum, not bit for bit); out may
 * then be NULL, else it receives the logits z themselves.
 * The order of a row's sum depends on that row's own edge list and on dim alone (attach.hip has it): not on m, the row's
 * position or the other rows, so a row has the same bits alone, in any batch and on every launch.  No atomics.  The launch
 * allocates nothing, does not synchronise and TRUSTS d_col to be in [0, n_a + m): the host validates (gcnhost_attach_rows). */
int gcnhip_attach_gather(gcnhip_ctx *ctx, const int32_t *d_ptr, const int32_t *d_col, const float *d_coef, int m, const float *table_a,
                         int ld_a, int n_a, const float *table_b, int ld_b, int dim, int epilogue, float *out, int ld_out, int32_t *d_pred,
                         float *d_prob, float *d_logp, int ld_logp, float beta);
/* Unregister a row subset made by gcnhip_graph_add_rowset (synchronises the context's stream, frees its task lists): for
 * subsets made at call time, such as the node queries of a prediction. */
int gcnhip_graph_remove_rowset(gcnhip_ctx *ctx, gcnhip_graph *g, gcnhip_rowset *rows);
/* device pointers of the factor arrays of a prepared adjacency: dinv / dinv^2 per row ([n_rows]) and per column ([n_cols]);
 * degrees are those of the full graph also for objects made by gcnhip_graph_create_restricted */
int gcnhip_graph_scales(const gcnhip_graph *g, const float **d_dinv_row, const float **d_dinv2_row,
                        const float **d_dinv_col, const float **d_dinv2_col);
/* values of row r of a feature object *= d_row_scale[r] (all of its internal copies; synchronises): X -> D^-1/2 X */
int gcnhip_feat_scale_rows(gcnhip_ctx *ctx, gcnhip_feat *f, const float *d_row_scale);

/* Aggregate-first evaluation.  Without dropout the first layer is linear in X: ReLU(A^.(X.W1)) = ReLU((A^.X).W1)
 * (src/seq/gcn.cpp:23-41 with Dropout skipped, module.cpp:208), and A^.X does not change from epoch to epoch.
 * This builds the feature object of A^.X once (dense X only; x has g->n_cols rows — every column of g); an
 * evaluation forward then runs gcnhip_spmm_fwd_relu on it and needs NO hidden-width aggregation (and, with
 * several GPUs, no exchange before the hidden layer).  Same result up to the rounding of a reassociated f32 sum.
 * Training cannot use it: its X~ changes with every epoch's dropout decisions. */
int gcnhip_feat_create_aggregated(gcnhip_ctx *ctx, gcnhip_feat **f, gcnhip_graph *g, const gcnhip_feat *x);
/* forward without dropout, ReLU (module.cpp:175-185, keep = x > 0) applied when the result is stored */
int gcnhip_spmm_fwd_relu(gcnhip_ctx *ctx, const gcnhip_feat *f, const float *vals, const float *w, int ld_w,
                         float *out, int ld_out, int p);
/* Evaluation forward of BOTH layers' products in one launch (round 5): z0[m x p2] = ReLU(X . w)[m x p] . w2[p x p2], the hidden
 * matrix never stored (SparseMatmul::forward + ReLU + Matmul::forward, module.cpp:47-61, 175-185, 11-22, for a forward whose
 * hidden activations nobody reads afterwards: GCN::eval with the aggregate-first feature object).  The first product is
 * computed transposed on the bf16 pipe (three-plane splits, as gcnhip_spmm_fwd does at p = 128), which leaves a row's features
 * in one lane's accumulators — the operand layout of the second product.  Available for a dense X, p = 128, p2 <= 64,
 * 16-byte aligned rows of z0 and option gemm_bf16x3 != 0; otherwise returns GCNHIP_NOT_AVAILABLE (nothing launched: call
 * gcnhip_spmm_fwd_relu and gcnhip_matmul_fwd instead).  Results inside the f32 summation bound of the two-call form, not its bits. */
#define GCNHIP_NOT_AVAILABLE (-2)
int gcnhip_spmm_fwd_relu_matmul(gcnhip_ctx *ctx, const gcnhip_feat *f, const float *vals, const float *w, int ld_w, int p,
                                const float *w2, int ld_w2, int p2, float *z0, int ld_z0);
/* The dense weight gradient (dense X, p > 64) is a split-K product: n_splits row ranges of rows_per_split rows each
 * write a partial [n_cols x p] slab, and an ordered sum of the slabs gives dW (no atomics: the same bits every run).
 * The three steps are also callable one by one, so that a caller whose dOut arrives in row blocks (the hidden layer's
 * backward aggregation, computed block by block on another stream) can start on the first blocks while the rest is
 * still being produced:  _plan reports the ranges (n_splits == 0: this shape does not take the split-K path, use
 * gcnhip_spmm_bwd);  _part computes splits [split_begin, split_end) into the context's slabs — rows
 * [split_begin * rows_per_split, min(n_rows, split_end * rows_per_split)) of X and dOut are all it reads;
 * make_decisions != 0 (re)generates the input-dropout decisions first, once per backward (0: the decisions a forward or an
 * earlier part made with the same p_drop / seed / epoch / nnz_offset are still in the feature object; their bit layout is the
 * library's own — flat or a word per row and 32 columns, by kernel family — and a part that needs the other one re-derives it
 * from the same arguments);  _finish sums the slabs of the same context.  gcnhip_spmm_bwd is exactly _part(0, n_splits, 1) + _finish. */
int gcnhip_spmm_bwd_plan(const gcnhip_ctx *ctx, const gcnhip_feat *f, int p, int *rows_per_split, int *n_splits);
int gcnhip_spmm_bwd_part(gcnhip_ctx *ctx, const gcnhip_feat *f, const float *vals, const float *dout, int ld_dout, int p,
                         float p_drop, uint64_t seed, const uint32_t *d_epoch, uint64_t nnz_offset, const uint8_t *keep_mask,
                         int split_begin, int split_end, int make_decisions);
int gcnhip_spmm_bwd_finish(gcnhip_ctx *ctx, const gcnhip_feat *f, float *dw, int ld_dw, int p);

/* ---- opt-in storage format: bfloat16 gathered tables (beyond the reference) ----------
 * gcnhip_f32_to_bf16 rounds rows of f32 to bf16 (nearest even; NaN kept) into a table with row stride ld_dst
 * (multiple of 8, 16-byte aligned; columns dim..ld_dst-1 are written as zero).  gcnhip_graphsum_bf16 is
 * GraphSum reading that table: coef, the running sum and `out` are f32, so the ONLY difference to
 * gcnhip_graphsum* is the rounding of the gathered values — on a table that holds bf16-representable numbers
 * the two agree bit for bit.  A row of d values is 2d bytes: half the cache lines per edge.
 * in_row_bits (optional) as in gcnhip_graphsum_rowmask, out_rows (optional) as in gcnhip_graphsum_rowset; relu_dropout != 0 selects the fused epilogue of
 * gcnhip_graphsum_relu_dropout with the arguments that follow. */
int gcnhip_f32_to_bf16(gcnhip_ctx *ctx, const float *src, int ld_src, uint16_t *dst, int ld_dst, int64_t rows, int dim);
int gcnhip_graphsum_bf16(gcnhip_ctx *ctx, const gcnhip_graph *g, const uint16_t *in_bf16, int ld_in,
                         float *out, int ld_out, int dim, const uint32_t *in_row_bits, const gcnhip_rowset *out_rows,
                         int relu_dropout, int training, float p, uint64_t seed, const uint32_t *d_epoch,
                         uint64_t elem_offset, const uint8_t *keep_mask);

/* da only, with the ReLU+Dropout backward fused into the store:
 * da[i,j] = (h[i,j] > 0) ? scale * (dc . b^T)[i,j] : 0, h = the forward output
 * of gcnhip_graphsum_relu_dropout (module.cpp:187-194, 223-233). */
int gcnhip_matmul_bwd_fused(gcnhip_ctx *ctx, const float *a, int lda, const float *b, int ldb,
                            const float *dc, int lddc, float *da, int ldda, float *db, int lddb,
                            int m, int n, int p, float relu_dropout_scale);
/* ... with the mask taken from the bits gcnhip_graphsum_relu_dropout_bits left (same result bit for bit: the bit IS h > 0) */
int gcnhip_matmul_bwd_fused_bits(gcnhip_ctx *ctx, const float *a, int lda, const float *b, int ldb,
                                 const float *dc, int lddc, float *da, int ldda, float *db, int lddb,
                                 int m, int n, int p, float relu_dropout_scale, const uint32_t *pos_bits, int words_per_row);

/* every form of the fused backward in one call, plus an optional factor per row of da:  db = a^T . dc when db != NULL;
 * da[r,:] = mask . (relu_dropout_scale * d_da_row_scale[r]) . (dc . b^T)[r,:], mask = pos_bits when given (a may then be
 * NULL if db is NULL too), else a > 0; d_da_row_scale == NULL: factor 1 */
int gcnhip_matmul_bwd_ex(gcnhip_ctx *ctx, const float *a, int lda, const float *b, int ldb,
                         const float *dc, int lddc, float *da, int ldda, float *db, int lddb,
                         int m, int n, int p, float relu_dropout_scale, const uint32_t *pos_bits, int words_per_row,
                         const float *d_da_row_scale);

/* Multi-GPU form of the same backward.  dH1 = mask . (dZ0 . W2^T) is cheap to recompute and 128 floats wide,
 * while its inputs are 48 floats (dZ0) and 1 bit per element (mask = H1 > 0): ranks all-gather those and each
 * rebuilds dH1 for every row.  gcnhip_pack_positive writes bit (c & 31) of bits[r*words_per_row + (c >> 5)] =
 * (h[r,c] > 0); gcnhip_matmul_bwd_da_bits computes da[m x n] = bit ? scale * (dc . b^T) : 0 for all m rows. */
int gcnhip_pack_positive(gcnhip_ctx *ctx, const float *h, int ld, int n_rows, int dim, uint32_t *bits, int words_per_row);
int gcnhip_matmul_bwd_da_bits(gcnhip_ctx *ctx, const float *b, int ldb, const float *dc, int lddc,
                              float *da, int ldda, int m, int n, int p,
                              const uint32_t *h_pos_bits, int words_per_row, float scale);

/* Row packing for the halo exchange (new: the reference is single-GPU).  dst[i, 0:ld_words] = src[d_rows[i], 0:ld_words]
 * for i < n; rows are arrays of 4-byte words that are moved, not interpreted (f32 rows, bf16 rows, mask words). */
int gcnhip_gather_rows(gcnhip_ctx *ctx, const float *src, int ld_words, const int *d_rows, int n, float *dst);

/* backward of the fused ReLU+Dropout: grad[i] = h[i] > 0 ? scale * grad[i] : 0 */
int gcnhip_relu_dropout_bwd(gcnhip_ctx *ctx, float *grad, int ld_grad, const float *h, int ld_h,
                            int n_rows, int dim, float scale);

/* The same over a list of rows known to be labelled (d_rows[n_listed], ascending row ids of one split; count = the
 * split's size over all ranks): only those rows of logits are read and only those rows of grad are written — the
 * caller guarantees that every other row of grad is already zero (it is after allocation, and stays so because the
 * training split never changes).  Losses are added in list order per wave, so the result equals gcnhip_xent_fwd's
 * to rounding, not bit for bit. */
int gcnhip_xent_fwd_rows(gcnhip_ctx *ctx, float *logits, int ld, float *grad, int ld_grad,
                         const int32_t *truth, const int32_t *d_rows, int n_listed, int num_classes, int training,
                         int count, int shift_in_place, float *d_result, int32_t *d_result_i);
/* ... with row r of grad multiplied by d_grad_row_scale[r] (NULL: as above) — the factored aggregation's input dinv . dZ */
int gcnhip_xent_fwd_rows_scaled(gcnhip_ctx *ctx, float *logits, int ld, float *grad, int ld_grad,
                                const int32_t *truth, const int32_t *d_rows, int n_listed, int num_classes, int training,
                                int count, int shift_in_place, float *d_result, int32_t *d_result_i, const float *d_grad_row_scale);
/* The end of gcnhip_xent_fwd_rows from the per-row terms a loss epilogue left (gcnhip_gs_loss above): d_result / d_result_i
 * exactly as gcnhip_xent_fwd_rows(_scaled) would have written them from the stored logits (same per-lane order, same block
 * partials, same final reduction — bit for bit), an armed metrics record included. */
int gcnhip_xent_from_row_terms(gcnhip_ctx *ctx, const float *d_row_terms, const int32_t *truth, const int32_t *d_rows, int n_listed,
                               float *d_result, int32_t *d_result_i);
/* ---- multi-label (beyond the reference, which is single-label) ----------------------------------------------------
 * Per-class sigmoid cross-entropy over a list of rows (bce.hip).  Truth: multi-hot bit rows, bit (c & 31) of word
 * truth_bits[r * words_per_row + (c >> 5)] = class c of row r, words_per_row >= ceil(C / 32).  For every listed row r and
 * class c (y in {0, 1}): the term max(z, 0) - z y + log(1 + exp(-|z|)) (finite for every finite z); when training,
 * grad[r, c] = (sigmoid(z) - y) / (count * C), times d_grad_row_scale[r] when given (the factored form), and no other row
 * of grad is written; the counts TP (z > 0, y = 1), FP (z > 0, y = 0), FN (z <= 0, y = 1).  count = listed rows over all
 * ranks (> 0 when training).  d_result[4] = {sum of terms, n_listed * C, 2 TP, 2 TP + FP + FN} — every entry additive
 * across ranks, so an all-reduce of the four floats is enough: loss = [0] / [1], micro-F1 = [2] / [3] (0 when [3] is 0).
 * d_result_i (may be NULL) [4] = {TP, FP, FN, n_listed}, exact.  The sums are deterministic (block partials added in
 * block order: two launches give the same bits).  An armed gcnhip_metrics_record_with_next_loss is honoured: the ring row
 * receives d_result's four floats.  1 <= num_classes <= 256, else -1.  Graph-capturable. */
int gcnhip_bce_fwd_rows(gcnhip_ctx *ctx, const float *logits, int ld, float *grad, int ld_grad,
                        const uint32_t *truth_bits, int words_per_row, const int32_t *d_rows, int n_listed,
                        int num_classes, int training, int count, const float *d_grad_row_scale,
                        float *d_result, int32_t *d_result_i);
/* Predicted class sets of n_rows rows (d_rows[i], or row i when d_rows is NULL) of a logit table: bits[i * words_per_row
 * + (c >> 5)] bit (c & 31) = (z_c > 0), the rule of the counts above (bits past C are 0); prob (may be NULL)
 * [i * ld_prob + c] = sigmoid(z_c).  1 <= num_classes <= 256. */
int gcnhip_bce_predict_rows(gcnhip_ctx *ctx, const float *logits, int ld, const int32_t *d_rows, int n_rows, int num_classes,
                            uint32_t *bits, int words_per_row, float *prob, int ld_prob);
/* ---- class-weighted losses (xent.hip, bce.hip: the W = true kernels; beyond the reference, whose loss weighs every row equally) -------------------
 * Weighted softmax cross-entropy over a row list: the arguments of gcnhip_xent_fwd_rows_scaled plus d_class_weight [C]
 * (finite, >= 0) and weight_sum.  For each listed row r with truth t in [0, C) and w = d_class_weight[t]: the term
 * w * (log sum exp(z - max) - (z_t - max)); when training, grad[r, j] = w * (p_j - [j == t]) / weight_sum, times
 * d_grad_row_scale[r] when given, where weight_sum = sum of w[truth] over the scored split's rows of ALL ranks (the caller
 * knows it: labels and splits never change) and must be > 0.  Accuracy is not weighted.  d_result[4] = {sum of w * term,
 * sum of w over this call's rows, correct, total} — every entry additive across ranks; loss = [0] / [1], the weighted mean of
 * torch's cross_entropy(weight=, reduction="mean").  d_result_i (may be NULL) [2] = {correct, total}.  A listed row whose
 * truth is outside [0, C) has no weight: zero gradient row, in no count.  Same grids, lane -> row assignment and order of
 * additions as gcnhip_xent_fwd_rows_scaled: with every weight 1.0f the gradient and all of d_result / d_result_i have that
 * entry point's bits.  Deterministic (block partials added in block order by a finalize launch, which also writes an armed
 * gcnhip_metrics_record_with_next_loss row).  1 <= num_classes <= 256, else -1 with a message.  Graph-capturable. */
int gcnhip_wxent_fwd_rows(gcnhip_ctx *ctx, float *logits, int ld, float *grad, int ld_grad,
                          const int32_t *truth, const int32_t *d_rows, int n_listed, int num_classes, int training,
                          int count, int shift_in_place, float *d_result, int32_t *d_result_i, const float *d_grad_row_scale,
                          const float *d_class_weight, float weight_sum);
/* gcnhip_bce_fwd_rows with a weight on the positive term of every class, d_pos_weight [C] (finite, >= 0): the term
 * pw_c * y * softplus(-z) + (1 - y) * softplus(z), softplus(x) = max(x, 0) + log1p(exp(-|x|)); when training, grad[r, c] =
 * (y ? -pw_c * sigmoid(-z) : sigmoid(z)) / (count * C) [* d_grad_row_scale[r]].  Normaliser, TP / FP / FN, d_result,
 * d_result_i, limits, determinism and the armed metrics row exactly as gcnhip_bce_fwd_rows: torch's
 * binary_cross_entropy_with_logits(pos_weight=, reduction="mean"). */
int gcnhip_wbce_fwd_rows(gcnhip_ctx *ctx, const float *logits, int ld, float *grad, int ld_grad,
                         const uint32_t *truth_bits, int words_per_row, const int32_t *d_rows, int n_listed,
                         int num_classes, int training, int count, const float *d_grad_row_scale,
                         float *d_result, int32_t *d_result_i, const float *d_pos_weight);
/* ---- per-class evaluation counts (report.hip; beyond the reference, which reports one accuracy per split) -----------
 * Both entry points ZERO their outputs on ctx's stream and then count, so a call with n == 0 leaves zeros.  All counts are
 * integers and integer addition commutes and associates: the result depends neither on the order of the blocks nor on the
 * order in which their atomic adds arrive, and two launches on the same inputs give identical output.  Not part of any
 * captured epoch.
 *
 * Confusion matrix of a single-label model: for each of the n listed rows r = d_rows[i] (repeats count as often as they are
 * listed; d_rows == NULL: rows 0 .. n - 1), counts[t * C + p] += 1 with t = truth[r] (an array as gcnhip_set_truth makes) and
 * p = pred[r] (the array gcnhip_graphsum_predict writes); pred and truth have n_table entries.  *out_of_range = listed rows
 * that are NOT in the matrix: truth outside [0, C) (an unlabelled row, -1) — and, so that no input can index past the
 * matrix, a row id outside [0, n_table) or a prediction outside [0, C), which the producers above never write.
 * counts [C * C] and out_of_range [1] are int32 device arrays.  1 <= num_classes <= 64 (gcnhip_graphsum_predict's limit: the
 * block's matrix is 16 KB of LDS at most); a larger C returns -1 with a message (gcnhip_last_error). */
int gcnhip_confusion_rows(gcnhip_ctx *ctx, const int32_t *pred, const int32_t *truth, int n_table, const int32_t *d_rows, int n,
                          int num_classes, int32_t *counts, int32_t *out_of_range);
/* TP / FP / FN of every class of a multi-label model over n listed rows of a logit table (layouts, row list and limits of
 * gcnhip_bce_fwd_rows; d_rows == NULL: rows 0 .. n - 1): counts [3 * C] int32 = {TP[C], FP[C], FN[C]} with the rule the loss
 * kernel counts by — class c is predicted for a row when z_c > 0.  Their sums over the classes are d_result_i[0..2] of
 * gcnhip_bce_fwd_rows on the same inputs.  1 <= num_classes <= 256, else -1 with a message. */
int gcnhip_bce_class_counts_rows(gcnhip_ctx *ctx, const float *logits, int ld, const uint32_t *truth_bits, int words_per_row,
                                 const int32_t *d_rows, int n, int num_classes, int32_t *counts);
/* The same update, and the epoch word advanced behind it in the same launch (the block that finishes last, after every
 * block has read the word): *d_epoch_done = e, *d_epoch_counter = e + 1 with e the counter's value during the launch.
 * The training pass of epoch e + 1 then reads its epoch from d_epoch_counter without a launch of its own
 * (gcnhip_counter_add), while an evaluation of epoch e's weights names its metrics row through d_epoch_done.
 * d_epoch (the index into d_step_sizes) may be d_epoch_counter itself or NULL. */
int gcnhip_adam_step_advance(gcnhip_ctx *ctx, const gcnhip_adam_var *vars, int n_vars, float step_size,
                             const float *d_step_sizes, const uint32_t *d_epoch,
                             float beta1, float beta2, float eps, float weight_decay, float *d_sumsq,
                             uint32_t *d_epoch_counter, uint32_t *d_epoch_done);

/* ---- small device utilities for graph-replayed epochs -------------------------- */
int gcnhip_counter_add(gcnhip_ctx *ctx, uint32_t *d_counter, uint32_t inc);
/* metrics ring [capacity][4 slots][8 floats]: slot `slot_in_row` (0..3) of row `*d_epoch % capacity`
 * = {loss_sum, count, correct, total, sumsq, epoch, 0, 0}.  correct/total come from d_result_i when it is
 * non-NULL, else from d_result[2..3] (the all-reduced floats of a multi-GPU run). */
int gcnhip_metrics_record(gcnhip_ctx *ctx, float *d_ring, int capacity, int slot_in_row,
                          const uint32_t *d_epoch, const float *d_result, const int32_t *d_result_i,
                          const float *d_sumsq);
/* The same row, written by the NEXT gcnhip_xent_fwd / gcnhip_xent_fwd_rows launched on ctx, from that launch's own
 * final reduction (the block that finishes last adds the block partials in block order and then fills the row: no
 * launch for the final sum, none for the copy).  One-shot: the loss call disarms it.  For a run whose d_result needs
 * no all-reduce before it is reported (one GPU); correct/total are taken from the launch's counts, as
 * gcnhip_metrics_record does with d_result_i == NULL.  Reference: the four scalars CUDACrossEntropyLoss leaves for
 * GCN::train_epoch / eval to read back (src/cuda/cuda_module.cu, src/seq/gcn.cpp:107-128). */
int gcnhip_metrics_record_with_next_loss(gcnhip_ctx *ctx, float *d_ring, int capacity, int slot_in_row,
                                         const uint32_t *d_epoch, const float *d_sumsq);

/* ---- hipGraph capture of a launch sequence (small graphs are launch-bound: ~25 kernels of a few
 *      microseconds per epoch).  Everything the ops read that changes from epoch to epoch lives in
 *      device memory (epoch word, step-size table, metrics ring), so one captured epoch replays
 *      correctly any number of times.  Ops must have run once eagerly before (scratch is sized on
 *      first use). */
int gcnhip_capture_begin(gcnhip_ctx *ctx);
int gcnhip_capture_end(gcnhip_ctx *ctx, void **graph_exec);
int gcnhip_graph_launch(gcnhip_ctx *ctx, void *graph_exec);
int gcnhip_graph_exec_destroy(void *graph_exec);

#ifdef __cplusplus
}
#endif
#endif
