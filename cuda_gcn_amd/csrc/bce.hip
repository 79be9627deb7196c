// bce.hip — multi-label loss and prediction: per-class sigmoid cross-entropy over a list of rows, micro-F1 counts, and the
// predicted class sets as packed bits.  Beyond the reference, which is single-label (softmax, argmax accuracy).
//
// Layout: one wave64 per listed row, lane j on class j (j + 64, j + 128, j + 192 for wider rows: C <= 256 sits in four
// registers).  Nothing is reduced across a row: every (row, class) term is independent, so a lane adds its terms, counts
// its TP / FP / FN and writes its dZ entries without a shuffle; the wave and block sums happen once, at the end.  The next
// row's logits and truth word are loaded while this row's terms are computed (each row is a dependent chain rows[q] ->
// logits).  Reductions are deterministic: per-lane in row order, a fixed shuffle tree, block partials added in block
// order by a one-block finalize launch — the grid depends on n_rows alone, so two launches give the same bits.
//
// bce_fwd_kernel<true> (gcnhip_wbce_fwd_rows) is the same walk with a weight per class on the positive term and its gradient
// (pos_weight), which a lane holds in four registers for the whole launch: no LDS.
#include "common.h"
#include <stdlib.h>
#pragma clang fp contract(off)
#include "score_rules.h"                 // bce_sigmoid

constexpr int BCE_MAXC_REG = 4;          // 4 x 64 = 256 classes
constexpr int BCE_MAX_BLOCKS = 1024;     // part_i holds 3 ints per block: red_i[0, 3072)

struct BceArgs {
    const float *logits;
    float *grad;                // NULL: no gradient
    const uint32_t *truth;      // [row * wpr + word], bit (c & 31) of word c >> 5
    const int32_t *rows;        // NULL: rows 0 .. n_rows - 1
    const float *grad_row_scale;
    int ld, ld_grad, wpr, n_rows, C;
    float denom;                // count * C (the gradient's divisor)
    float *part_f;              // [blocks]
    int32_t *part_i;            // [blocks * 3] {TP, FP, FN}
    const float *pos_weight;    // W = true only: [C] (kept at the end: the offsets the unweighted kernel reads stay where they were)
};

template <bool W>
__global__ __launch_bounds__(256) void bce_fwd_kernel(BceArgs a) {
    __shared__ float sh_f[4];
    __shared__ int sh_i[12];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves_total = gridDim.x * 4;
    float loss = 0.f;
    int tp = 0, fp = 0, fn = 0;
    float pw[BCE_MAXC_REG];
    if constexpr (W) {
#pragma unroll
        for (int k = 0; k < BCE_MAXC_REG; k++) {
            const int j = lane + k * WAVE;
            pw[k] = j < a.C ? a.pos_weight[j] : 0.f;
        }
    }
    float nv[BCE_MAXC_REG];
    uint32_t nw[BCE_MAXC_REG];
    auto prefetch = [&](int q) {
        const int r = a.rows ? a.rows[q] : q;
        const float *lg = a.logits + (size_t)r * a.ld;
        const uint32_t *tw = a.truth + (size_t)r * a.wpr;
#pragma unroll
        for (int k = 0; k < BCE_MAXC_REG; k++) {
            const int j = lane + k * WAVE;
            nv[k] = j < a.C ? lg[j] : 0.f;
            nw[k] = j < a.C ? tw[j >> 5] : 0u;
        }
    };
    int q = blockIdx.x * 4 + wave;
    if (q < a.n_rows) prefetch(q);
    for (; q < a.n_rows; q += waves_total) {
        const int r = a.rows ? a.rows[q] : q;
        float v[BCE_MAXC_REG];
        uint32_t w[BCE_MAXC_REG];
#pragma unroll
        for (int k = 0; k < BCE_MAXC_REG; k++) { v[k] = nv[k]; w[k] = nw[k]; }
        if (q + waves_total < a.n_rows) prefetch(q + waves_total);
        float *gr = a.grad ? a.grad + (size_t)r * a.ld_grad : nullptr;
        const float gs = a.grad_row_scale && gr ? a.grad_row_scale[r] : 1.f;
#pragma unroll
        for (int k = 0; k < BCE_MAXC_REG; k++) {
            const int j = lane + k * WAVE;
            if (j >= a.C) continue;
            const float z = v[k];
            const bool y = (w[k] >> (j & 31)) & 1u;
            if constexpr (W) {
                // pw . y . softplus(-z) + (1 - y) . softplus(z), softplus(x) = max(x, 0) + log1p(exp(-|x|)): finite for every finite z
                const float l1p = log1pf(expf(-fabsf(z)));
                loss += y ? pw[k] * (fmaxf(-z, 0.f) + l1p) : fmaxf(z, 0.f) + l1p;
            } else {
                // max(z, 0) - z y + log(1 + exp(-|z|)): finite for every finite z
                loss += (fmaxf(z, 0.f) - (y ? z : 0.f)) + log1pf(expf(-fabsf(z)));
            }
            const bool pos = z > 0.f;
            tp += pos && y;
            fp += pos && !y;
            fn += !pos && y;
            if (gr) {
                // sigmoid(z) - 1 = -sigmoid(-z): no cancellation when y = 1 and z is large (float 1 - 4e-8 keeps one digit)
                const float g = (y ? -(W ? pw[k] * bce_sigmoid(-z) : bce_sigmoid(-z)) : bce_sigmoid(z)) / a.denom;
                gr[j] = a.grad_row_scale ? g * gs : g;
            }
        }
    }
    loss = wave_sum(loss); tp = wave_sum_i(tp); fp = wave_sum_i(fp); fn = wave_sum_i(fn);
    if (lane == 0) { sh_f[wave] = loss; sh_i[wave * 3] = tp; sh_i[wave * 3 + 1] = fp; sh_i[wave * 3 + 2] = fn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.part_f[blockIdx.x] = (sh_f[0] + sh_f[1]) + (sh_f[2] + sh_f[3]);
#pragma unroll
        for (int k = 0; k < 3; k++) a.part_i[blockIdx.x * 3 + k] = sh_i[k] + sh_i[3 + k] + sh_i[6 + k] + sh_i[9 + k];
    }
}

// fixed-order sum of the block partials; d_result = {loss_sum, n_rows * C, 2 TP, 2 TP + FP + FN} (additive across ranks:
// loss = [0] / [1], micro-F1 = [2] / [3]), d_result_i = {TP, FP, FN, n_rows}, and the metrics-ring row when one is armed
__global__ __launch_bounds__(256) void bce_finalize_kernel(const float *part_f, const int32_t *part_i, int n, int n_rows, int C,
                                                           float *res, int32_t *res_i, float *ring, int ring_capacity, int ring_slot,
                                                           const uint32_t *ring_epoch, const float *ring_sumsq) {
    __shared__ float shf[4];
    __shared__ int shi[12];
    float l = 0.f;
    int tp = 0, fp = 0, fn = 0;
    for (int i = threadIdx.x; i < n; i += 256) { l += part_f[i]; tp += part_i[3 * i]; fp += part_i[3 * i + 1]; fn += part_i[3 * i + 2]; }
    l = wave_sum(l); tp = wave_sum_i(tp); fp = wave_sum_i(fp); fn = wave_sum_i(fn);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { shf[w] = l; shi[3 * w] = tp; shi[3 * w + 1] = fp; shi[3 * w + 2] = fn; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int TP = shi[0] + shi[3] + shi[6] + shi[9], FP = shi[1] + shi[4] + shi[7] + shi[10], FN = shi[2] + shi[5] + shi[8] + shi[11];
    const float r[4] = {(shf[0] + shf[1]) + (shf[2] + shf[3]), (float)((double)n_rows * C), (float)(2.0 * TP), (float)(2.0 * TP + FP + FN)};
    if (res) { res[0] = r[0]; res[1] = r[1]; res[2] = r[2]; res[3] = r[3]; }
    if (res_i) { res_i[0] = TP; res_i[1] = FP; res_i[2] = FN; res_i[3] = n_rows; }
    ring_row_write({ring, ring_capacity, ring_slot, ring_epoch, ring_sumsq}, r[0], r[1], r[2], r[3]);
}

// one wave per listed row: bit c of the row's words = (z_c > 0), the rule the TP / FP / FN counts use; optional sigmoid row
__global__ __launch_bounds__(256) void bce_predict_kernel(const float *logits, int ld, const int32_t *rows, int n, int C,
                                                          uint32_t *bits, int wpr, float *prob, int ld_prob) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;                                   // whole waves leave together: the ballot below sees all 64 lanes
    const int r = rows ? rows[i] : i;
    const float *lg = logits + (size_t)r * ld;
    for (int k = 0; k * WAVE < C; k++) {
        const int j = lane + k * WAVE;
        const float z = j < C ? lg[j] : 0.f;
        const unsigned long long m = __ballot(j < C && z > 0.f);
        if (lane == 0) {
            if (2 * k < wpr) bits[(size_t)i * wpr + 2 * k] = (uint32_t)m;
            if (2 * k + 1 < wpr) bits[(size_t)i * wpr + 2 * k + 1] = (uint32_t)(m >> 32);
        }
        if (prob && j < C) prob[(size_t)i * ld_prob + j] = bce_sigmoid(z);
    }
}

// both entry points, after the checks that differ between them; d_pos_weight chooses the weighted kernel
static int bce_launch(gcnhip_ctx *c, const float *logits, int ld, float *grad, int ld_grad,
                      const uint32_t *truth_bits, int words_per_row, const int32_t *d_rows, int n_listed,
                      int num_classes, int training, int count, const float *d_grad_row_scale,
                      float *d_result, int32_t *d_result_i, const float *d_pos_weight) {
    if (words_per_row < (num_classes + 31) / 32 || n_listed < 0 || (n_listed > 0 && !d_rows)) return -1;
    if (training && (!grad || ld_grad < num_classes || count <= 0)) return -1;
    BceArgs a;
    a.logits = logits; a.grad = training ? grad : nullptr; a.truth = truth_bits; a.rows = d_rows;
    a.grad_row_scale = d_grad_row_scale; a.pos_weight = d_pos_weight;
    a.ld = ld; a.ld_grad = ld_grad; a.wpr = words_per_row; a.n_rows = n_listed; a.C = num_classes;
    a.denom = (float)((double)(count > 0 ? count : 1) * num_classes);
    int blocks = ceil_div(n_listed, 4 * 4);               // ~4 rows per wave on small inputs; the cap decides on large ones
    if (blocks > BCE_MAX_BLOCKS) blocks = BCE_MAX_BLOCKS;
    if (blocks < 1) blocks = 1;                           // a rank that owns no rows still reports zeros
    a.part_f = c->red_f + 2048;
    a.part_i = c->red_i;
    if (d_pos_weight) bce_fwd_kernel<true><<<blocks, 256, 0, c->stream>>>(a);
    else bce_fwd_kernel<false><<<blocks, 256, 0, c->stream>>>(a);
    GCNHIP_LAUNCH_CHECK();
    const RingRow g = ring_row_take(c);                   // gcnhip_metrics_record_with_next_loss: this launch writes the row
    bce_finalize_kernel<<<1, 256, 0, c->stream>>>(a.part_f, a.part_i, blocks, n_listed, num_classes, d_result, d_result_i,
                                                  g.ring, g.capacity, g.slot, g.epoch, g.sumsq);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

extern "C" {

int gcnhip_bce_fwd_rows(gcnhip_ctx *c, const float *logits, int ld, float *grad, int ld_grad,
                        const uint32_t *truth_bits, int words_per_row, const int32_t *d_rows, int n_listed,
                        int num_classes, int training, int count, const float *d_grad_row_scale,
                        float *d_result, int32_t *d_result_i) {
    if (!c || !logits || !truth_bits || !d_result || num_classes < 1 || num_classes > BCE_MAXC_REG * WAVE || ld < num_classes) return -1;
    return bce_launch(c, logits, ld, grad, ld_grad, truth_bits, words_per_row, d_rows, n_listed, num_classes, training, count,
                      d_grad_row_scale, d_result, d_result_i, nullptr);
}

int gcnhip_wbce_fwd_rows(gcnhip_ctx *c, const float *logits, int ld, float *grad, int ld_grad,
                         const uint32_t *truth_bits, int words_per_row, const int32_t *d_rows, int n_listed,
                         int num_classes, int training, int count, const float *d_grad_row_scale,
                         float *d_result, int32_t *d_result_i, const float *d_pos_weight) {
    if (!c || !logits || !truth_bits || !d_result || !d_pos_weight || num_classes < 1 || ld < num_classes) return -1;
    if (num_classes > BCE_MAXC_REG * WAVE) return gcnhip_fail("gcnhip_wbce_fwd_rows: more than 256 classes");
    return bce_launch(c, logits, ld, grad, ld_grad, truth_bits, words_per_row, d_rows, n_listed, num_classes, training, count,
                      d_grad_row_scale, d_result, d_result_i, d_pos_weight);
}

int gcnhip_bce_predict_rows(gcnhip_ctx *c, const float *logits, int ld, const int32_t *d_rows, int n_rows, int num_classes,
                            uint32_t *bits, int words_per_row, float *prob, int ld_prob) {
    if (!c || !logits || !bits || num_classes < 1 || num_classes > BCE_MAXC_REG * WAVE || ld < num_classes || n_rows < 0) return -1;
    if (words_per_row < (num_classes + 31) / 32 || (prob && ld_prob < num_classes)) return -1;
    if (n_rows == 0) return 0;
    bce_predict_kernel<<<ceil_div(n_rows, 4), 256, 0, c->stream>>>(logits, ld, d_rows, n_rows, num_classes, bits, words_per_row, prob, ld_prob);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

GCNHIP_DEFINE_PRELOAD(bce, bce_fwd_kernel<false>)
