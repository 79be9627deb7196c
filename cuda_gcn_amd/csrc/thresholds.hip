// thresholds.hip — multi-label decision thresholds: one cut per class fitted on score rows that stay on the device, and the
// row-local kernels that decide by such cuts instead of the training rule z > 0.  Beyond the reference, which is single-label.
// None of the launches is part of a captured epoch.
//
//   gcnhip_threshold_scan             the sorted key columns ranking.hip makes (gcnhip_rank_keys, gcnhip_sort_segments_u32) ->
//                                     per class the cut with the largest F-beta, its TP / FP / FN and its F
//   gcnhip_bce_predict_rows_thr       gcnhip_bce_predict_rows with a cut per class
//   gcnhip_bce_class_counts_rows_thr  gcnhip_bce_class_counts_rows with a cut per class
//
// Rule.  With a threshold t[c], class c is predicted for a row exactly when its logit z is not NaN and key(z) >= key(t[c]),
// key() the order-preserving u32 image of score_rules.h: z >= t[c] in exact real comparison, -0.0 == +0.0, and denormal logits
// and thresholds compared as the numbers they are whatever the float denormal mode, because the comparison is one of integers.
// A NaN threshold has no key: its class is predicted for no row.
//
// Fit.  For one class, P positives and N negatives (NaN scores in neither).  The candidates are the keys k of the positives:
// a cut at a key only negatives hold predicts the same positives as the next positive key above it and no fewer negatives.
// At a cut, TP = #{pos >= k}, FP = #{neg >= k}, FN = P - TP — exact integers; the positives' column is sorted, so at the first
// entry i that holds k, TP = P - i, and FP is one binary search among the negatives.  In float64 with contraction off:
//     w = beta * beta;  num = (1.0 + w) * TP;  den = num + w * FN + FP;  F = num / den          (den > 0: TP >= 1)
// The winner has the largest F, among equal F the largest key (the fewest predictions).  P == 0: defined = 0, threshold 0.0f,
// TP = FN = 0, FP = #{neg >= key(0)}, F = 0 — never NaN.
//
// Determinism.  TP, FP, FN are integers; F is one correctly rounded expression of them; the max over (F, key) in lexicographic
// order is commutative and associative, so the strided walk, the shuffle tree, the LDS step and the fold over the blocks give
// the same bits in any order.  No atomics.
#include "common.h"
#include <cmath>
#pragma clang fp contract(off)
#include "score_rules.h"

constexpr int THR_N_MAX = 1 << 24;
constexpr int THR_MAXC_REG = 4;            // 4 x 64 = 256 classes, the limit of gcnhip_bce_predict_rows
constexpr int THR_MAX_BLOCKS = 512;

namespace {

// (f, k) = max((f, k), (of, ok)), F first, then the key.  "No candidate" is (-1, 0): every F of a candidate is > 0.
__device__ __forceinline__ void thr_take(double &f, uint32_t &k, double of, uint32_t ok) {
    if (of > f || (of == f && ok > k)) { f = of; k = ok; }
}
__device__ __forceinline__ double thr_fbeta(double w, int tp, int fp, int fn) {
    const double num = (1.0 + w) * (double)tp;
    const double den = (num + w * (double)fn) + (double)fp;
    return num / den;
}
// the key a logit's key is compared with: a NaN threshold gets the sentinel, above every logit's key
__device__ __forceinline__ uint32_t thr_key(float t) {
    const uint32_t b = __float_as_uint(t);
    return (b & 0x7FFFFFFFu) > 0x7F800000u ? RANK_SENTINEL : rank_key(b);
}
__device__ __forceinline__ bool thr_predicts(float z, uint32_t tkey) {
    const uint32_t b = __float_as_uint(z);
    return (b & 0x7FFFFFFFu) <= 0x7F800000u && rank_key(b) >= tkey;
}

}  // namespace

// grid (GCNHIP_THRESHOLD_SCAN_BLOCKS, S): block bx of class c takes the positives bx . 256 + t, + blocks . 256, ...; one partial
// (F, key) per block
__global__ __launch_bounds__(256) void threshold_scan_kernel(const uint32_t *__restrict__ pos_keys, const uint32_t *__restrict__ neg_keys, int64_t stride,
                                                             int n, const int32_t *__restrict__ pos, const int32_t *__restrict__ neg, double w,
                                                             double *__restrict__ part_f, uint32_t *__restrict__ part_key) {
    __shared__ double sh_f[4];
    __shared__ uint32_t sh_k[4];
    const int c = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int P = pos[c], N = neg[c];
    P = P < 0 ? 0 : (P > n ? n : P);                           // the valid lengths come from the counts; no count can index past a column
    N = N < 0 ? 0 : (N > n ? n : N);
    const uint32_t *pk = pos_keys + (size_t)c * (size_t)stride, *nk = neg_keys + (size_t)c * (size_t)stride;
    double best = -1.0;
    uint32_t best_key = 0u;
    for (int i = blockIdx.x * 256 + t; i < P; i += gridDim.x * 256) {
        const uint32_t k = pk[i];
        if (i > 0 && pk[i - 1] == k) continue;                 // a candidate is scored once, where its key first stands: TP = P - i
        const int tp = P - i, fp = N - rank_lower_bound(nk, N, k);
        thr_take(best, best_key, thr_fbeta(w, tp, fp, P - tp), k);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double of = __shfl_xor(best, off, WAVE);
        const uint32_t ok = (uint32_t)__shfl_xor((int)best_key, off, WAVE);
        thr_take(best, best_key, of, ok);
    }
    if (lane == 0) { sh_f[wave] = best; sh_k[wave] = best_key; }
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int v = 1; v < 4; v++) thr_take(best, best_key, sh_f[v], sh_k[v]);
        part_f[(size_t)c * gridDim.x + blockIdx.x] = best;
        part_key[(size_t)c * gridDim.x + blockIdx.x] = best_key;
    }
}
// a thread per class: the winner of the block partials, the counts at its key, the key back to its float
__global__ __launch_bounds__(256) void threshold_fold_kernel(const uint32_t *__restrict__ pos_keys, const uint32_t *__restrict__ neg_keys, int64_t stride,
                                                             int n, const int32_t *__restrict__ pos, const int32_t *__restrict__ neg,
                                                             const double *__restrict__ part_f, const uint32_t *__restrict__ part_key, int S, int blocks,
                                                             float *__restrict__ thr, int32_t *__restrict__ counts, double *__restrict__ f,
                                                             int32_t *__restrict__ defined) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= S) return;
    int P = pos[c], N = neg[c];
    P = P < 0 ? 0 : (P > n ? n : P);
    N = N < 0 ? 0 : (N > n ? n : N);
    const uint32_t *pk = pos_keys + (size_t)c * (size_t)stride, *nk = neg_keys + (size_t)c * (size_t)stride;
    double best = -1.0;
    uint32_t best_key = 0u;
    for (int b = 0; b < blocks; b++) thr_take(best, best_key, part_f[(size_t)c * blocks + b], part_key[(size_t)c * blocks + b]);
    const bool found = P > 0 && best > 0.0;
    const uint32_t k = found ? best_key : 0x80000000u;         // no positive: the cut 0.0f
    const int tp = found ? P - rank_lower_bound(pk, P, k) : 0;
    thr[c] = __uint_as_float(rank_key_bits(k));
    counts[c] = tp;
    counts[S + c] = N - rank_lower_bound(nk, N, k);
    counts[2 * S + c] = found ? P - tp : 0;
    f[c] = found ? best : 0.0;
    defined[c] = found ? 1 : 0;
}

// bce_predict_kernel with a cut per class: one wave per listed row
__global__ __launch_bounds__(256) void bce_predict_thr_kernel(const float *logits, int ld, const int32_t *rows, int n, int C, const float *__restrict__ thr,
                                                              uint32_t *bits, int wpr, float *prob, int ld_prob) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;                                        // whole waves leave together: the ballot below sees all 64 lanes
    const int r = rows ? rows[i] : i;
    const float *lg = logits + (size_t)r * ld;
    for (int k = 0; k * WAVE < C; k++) {
        const int j = lane + k * WAVE;
        const float z = j < C ? lg[j] : 0.f;
        const uint32_t tkey = j < C ? thr_key(thr[j]) : RANK_SENTINEL;
        const unsigned long long m = __ballot(j < C && thr_predicts(z, tkey));
        if (lane == 0) {
            if (2 * k < wpr) bits[(size_t)i * wpr + 2 * k] = (uint32_t)m;
            if (2 * k + 1 < wpr) bits[(size_t)i * wpr + 2 * k + 1] = (uint32_t)(m >> 32);
        }
        if (prob && j < C) prob[(size_t)i * ld_prob + j] = bce_sigmoid(z);
    }
}

// bce_class_counts_kernel with a cut per class: a lane keeps the keys of the cuts of its (up to) four classes for the whole
// launch, next to their TP / FP / FN; the four waves of a block add in LDS, one atomic per class, count and block goes to global
// memory.  The next row is loaded while this one is counted.
__global__ __launch_bounds__(256) void bce_class_counts_thr_kernel(const float *__restrict__ logits, int ld, const uint32_t *__restrict__ truth, int wpr,
                                                                   const int32_t *__restrict__ rows, int n, int C, const float *__restrict__ thr,
                                                                   int32_t *counts) {
    __shared__ int sh[3 * THR_MAXC_REG * WAVE];
    for (int c = threadIdx.x; c < 3 * THR_MAXC_REG * WAVE; c += 256) sh[c] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves_total = gridDim.x * 4;
    int tp[THR_MAXC_REG] = {}, fp[THR_MAXC_REG] = {}, fn[THR_MAXC_REG] = {};
    uint32_t tk[THR_MAXC_REG];
#pragma unroll
    for (int k = 0; k < THR_MAXC_REG; k++) {
        const int j = lane + k * WAVE;
        tk[k] = j < C ? thr_key(thr[j]) : RANK_SENTINEL;
    }
    float nv[THR_MAXC_REG];
    uint32_t nw[THR_MAXC_REG];
    auto prefetch = [&](int q) {
        const int r = rows ? rows[q] : q;
        const float *lg = logits + (size_t)r * ld;
        const uint32_t *tw = truth + (size_t)r * wpr;
#pragma unroll
        for (int k = 0; k < THR_MAXC_REG; k++) {
            const int j = lane + k * WAVE;
            nv[k] = j < C ? lg[j] : 0.f;
            nw[k] = j < C ? tw[j >> 5] : 0u;
        }
    };
    int q = blockIdx.x * 4 + wave;
    if (q < n) prefetch(q);
    for (; q < n; q += waves_total) {
        float v[THR_MAXC_REG];
        uint32_t w[THR_MAXC_REG];
#pragma unroll
        for (int k = 0; k < THR_MAXC_REG; k++) { v[k] = nv[k]; w[k] = nw[k]; }
        if (q + waves_total < n) prefetch(q + waves_total);
#pragma unroll
        for (int k = 0; k < THR_MAXC_REG; k++) {
            const int j = lane + k * WAVE;
            if (j >= C) continue;
            const bool y = (w[k] >> (j & 31)) & 1u;
            const bool pos = thr_predicts(v[k], tk[k]);
            tp[k] += pos && y;
            fp[k] += pos && !y;
            fn[k] += !pos && y;
        }
    }
#pragma unroll
    for (int k = 0; k < THR_MAXC_REG; k++) {
        const int j = lane + k * WAVE;
        if (j >= C) continue;
        if (tp[k]) atomicAdd(&sh[j], tp[k]);
        if (fp[k]) atomicAdd(&sh[THR_MAXC_REG * WAVE + j], fp[k]);
        if (fn[k]) atomicAdd(&sh[2 * THR_MAXC_REG * WAVE + j], fn[k]);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < 3 * THR_MAXC_REG * WAVE; c += 256) {
        const int which = c / (THR_MAXC_REG * WAVE), j = c % (THR_MAXC_REG * WAVE);
        const int v = sh[c];
        if (j < C && v) atomicAdd(&counts[which * C + j], v);
    }
}

extern "C" {

int gcnhip_threshold_scan(gcnhip_ctx *c, const uint32_t *pos_keys, const uint32_t *neg_keys, int64_t stride, int n, int segments, const int32_t *d_pos,
                          const int32_t *d_neg, double beta, void *d_work, float *d_thr, int32_t *d_counts, double *d_f, int32_t *d_defined) {
    if (!c || !pos_keys || !neg_keys || !d_pos || !d_neg || !d_work || !d_thr || !d_counts || !d_f || !d_defined)
        return gcnhip_fail("gcnhip_threshold_scan: invalid argument");
    if (!std::isfinite(beta) || !(beta > 0.0)) return gcnhip_fail("gcnhip_threshold_scan: beta must be finite and > 0");
    if (n < 0 || n > THR_N_MAX) return gcnhip_fail("gcnhip_threshold_scan: 0 <= n <= 2^24 keys per class");
    if (segments < 1 || segments > 65535) return gcnhip_fail("gcnhip_threshold_scan: 1 <= classes <= 65535");
    if (stride < n || stride < 1) return gcnhip_fail("gcnhip_threshold_scan: the column stride must be at least max(n, 1)");
    if (((uintptr_t)d_work & 7) != 0) return gcnhip_fail("gcnhip_threshold_scan: the work block must be 8-byte aligned");
    const double w = beta * beta;
    double *part_f = (double *)d_work;
    uint32_t *part_key = (uint32_t *)(part_f + (size_t)segments * GCNHIP_THRESHOLD_SCAN_BLOCKS);
    threshold_scan_kernel<<<dim3(GCNHIP_THRESHOLD_SCAN_BLOCKS, (unsigned)segments), 256, 0, c->stream>>>(pos_keys, neg_keys, stride, n, d_pos, d_neg, w, part_f,
                                                                                                         part_key);
    GCNHIP_LAUNCH_CHECK();
    threshold_fold_kernel<<<ceil_div(segments, 256), 256, 0, c->stream>>>(pos_keys, neg_keys, stride, n, d_pos, d_neg, part_f, part_key, segments,
                                                                          GCNHIP_THRESHOLD_SCAN_BLOCKS, d_thr, d_counts, d_f, d_defined);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_bce_predict_rows_thr(gcnhip_ctx *c, const float *logits, int ld, const int32_t *d_rows, int n_rows, int num_classes, const float *thr,
                                uint32_t *bits, int words_per_row, float *prob, int ld_prob) {
    if (!c || !logits || !bits || !thr || num_classes < 1 || ld < num_classes || n_rows < 0) return gcnhip_fail("gcnhip_bce_predict_rows_thr: invalid argument");
    if (num_classes > THR_MAXC_REG * WAVE) return gcnhip_fail("gcnhip_bce_predict_rows_thr: at most 256 classes (the limit of gcnhip_bce_predict_rows)");
    if (words_per_row < (num_classes + 31) / 32) return gcnhip_fail("gcnhip_bce_predict_rows_thr: words_per_row is below ceil(num_classes / 32)");
    if (prob && ld_prob < num_classes) return gcnhip_fail("gcnhip_bce_predict_rows_thr: the row stride of prob is below num_classes");
    if (n_rows == 0) return 0;
    bce_predict_thr_kernel<<<ceil_div(n_rows, 4), 256, 0, c->stream>>>(logits, ld, d_rows, n_rows, num_classes, thr, bits, words_per_row, prob, ld_prob);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_bce_class_counts_rows_thr(gcnhip_ctx *c, const float *logits, int ld, const uint32_t *truth_bits, int words_per_row, const int32_t *d_rows, int n,
                                     int num_classes, const float *thr, int32_t *counts) {
    if (!c || !logits || !truth_bits || !thr || !counts || n < 0 || num_classes < 1 || ld < num_classes)
        return gcnhip_fail("gcnhip_bce_class_counts_rows_thr: invalid argument");
    if (num_classes > THR_MAXC_REG * WAVE) return gcnhip_fail("gcnhip_bce_class_counts_rows_thr: at most 256 classes (the limit of gcnhip_bce_fwd_rows)");
    if (words_per_row < (num_classes + 31) / 32) return gcnhip_fail("gcnhip_bce_class_counts_rows_thr: words_per_row is below ceil(num_classes / 32)");
    GCNHIP_TRY(hipMemsetAsync(counts, 0, 3 * (size_t)num_classes * sizeof(int32_t), c->stream));
    if (n == 0) return 0;
    int blocks = ceil_div(n, 4 * 16);                          // ~16 rows per wave; the cap decides on large inputs
    if (blocks > THR_MAX_BLOCKS) blocks = THR_MAX_BLOCKS;
    bce_class_counts_thr_kernel<<<blocks, 256, 0, c->stream>>>(logits, ld, truth_bits, words_per_row, d_rows, n, num_classes, thr, counts);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
