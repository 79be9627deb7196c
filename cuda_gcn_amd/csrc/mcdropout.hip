// mcdropout.hip — Monte Carlo dropout (Gal & Ghahramani, 2016): the row-local statistics of S stochastic forwards.  Beyond the
// reference, which stops at accuracy.
//
// Definition.  p = the dropout rate, thr16 = dropout_threshold(p), sc = 1.f / (1.f - p) in f32, seed = a 64-bit seed of the
// query.  Sample s in [first_sample, first_sample + S) is the model's own training forward with the epoch word s:
//   X~[jj]  = X[jj] . (keep(seed ^ KEY_INPUT_DROPOUT, s, jj, thr16) ? sc : 0)          jj: the loader's CSR order (dense: r . F + k)
//   T       = X~ . W1
//   H[r, c] = ReLU((A^ . T)[r, c]) . (keep(seed ^ KEY_HIDDEN_DROPOUT, s, r . h + c, thr16) ? sc : 0)
//   Z       = A^ . (H . W2)
//   l_s     = log_softmax(Z / temperature)               (exactly predict()'s logp for those logits)
// keep, the two keys and the index rules are the training path's (common.h, host/module.h).  The host composes the forward from
// entry points that exist (host/mc_dropout.cpp); this file holds what is new — per listed row, with p_s = exp(l_s), everything
// in float64 until the final store:
//   mean_prob[c]       = (1 / S) sum_s p_s[c]
//   pred               = argmax_c mean_prob[c], lowest class on a tie;  confidence = mean_prob[pred]
//   entropy            = - sum_c mean_prob[c] ln mean_prob[c]                 (predictive; a zero probability contributes 0)
//   expected_entropy   = (1 / S) sum_s (- sum_c p_s[c] l_s[c])                (p_s[c] == 0 contributes 0, whatever l, -inf included)
//   mutual_information = max(0, entropy - expected_entropy)                   (BALD)
//   votes[c]           = #{s : argmax l_s = c}, lowest class on a tie;  variation_ratio = 1 - max_c votes[c] / S
//
// Layout: calib.hip's — one wave64 per listed row, lane j on class j (C <= 64: a row is one register), rows of any stride.  The
// accumulators are indexed by LIST POSITION (a row listed twice has two), acc_f64 [n x (C + 1)] = {sum_s p_s[c] | sum_s H_s} and
// acc_votes [n x C]; each is owned by one lane of one wave, so there are no atomics, a sample is added in launch order and the
// bits depend on the sample sequence alone.  Sums across the 64 lanes are xor butterflies in float64 (every lane gets the same
// bits).  A listed id outside [0, n_table) adds nothing (with first != 0 its accumulators are zeroed).
#include "common.h"
#include <cstdio>
#pragma clang fp contract(off)

constexpr int MC_ROWS_PER_BLOCK = 4 * 16;        // 4 waves x 16 rows; above MC_MAX_BLOCKS blocks the grid-stride loop does the rest
constexpr int MC_MAX_BLOCKS = 2048;

__device__ inline double mc_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
    return v;
}
__device__ inline double mc_wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, WAVE));
    return v;
}
__device__ inline float mc_wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, WAVE));
    return v;
}
__device__ inline int mc_wave_max(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, WAVE));
    return v;
}

__global__ __launch_bounds__(256) void mc_accumulate_kernel(const float *__restrict__ logp, int ld, int n_table, const int32_t *__restrict__ rows,
                                                            int n, int C, int first, double *__restrict__ acc, int32_t *__restrict__ votes) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves_total = gridDim.x * 4;
    const bool live = lane < C;
    for (int q = blockIdx.x * 4 + wave; q < n; q += waves_total) {
        const int r0 = rows ? rows[q] : q;
        const bool inside = r0 >= 0 && r0 < n_table;           // wave-uniform: no id can index past the table
        double *a = acc + (size_t)q * (C + 1);
        int32_t *v = votes + (size_t)q * C;
        if (!inside) {
            if (first) {
                if (live) { a[lane] = 0.0; v[lane] = 0; }
                if (lane == 0) a[C] = 0.0;
            }
            continue;
        }
        const float l = live ? logp[(size_t)r0 * ld + lane] : -INFINITY;
        const double p = live ? exp((double)l) : 0.0;
        const double h = mc_wave_sum(p == 0.0 ? 0.0 : -(p * (double)l));
        // the sample's vote is predict()'s: the largest entry, the lowest class on a tie (a NaN row votes for nobody)
        const float lmax = mc_wave_max(l);
        const int pred = __ffsll((unsigned long long)__ballot(live && l == lmax)) - 1;
        if (live) {
            const int vote = lane == pred ? 1 : 0;
            if (first) { a[lane] = p; v[lane] = vote; }
            else { a[lane] += p; if (vote) v[lane] += 1; }
        }
        if (lane == 0) a[C] = first ? h : a[C] + h;
    }
}

__global__ __launch_bounds__(256) void mc_finalize_kernel(const double *__restrict__ acc, const int32_t *__restrict__ votes, int n, int C, int samples,
                                                          float *mean_prob, int ld_mp, int32_t *pred, float *confidence, float *entropy,
                                                          float *expected_entropy, float *mutual_information, float *variation_ratio) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves_total = gridDim.x * 4;
    const bool live = lane < C;
    const double S = (double)samples;
    for (int q = blockIdx.x * 4 + wave; q < n; q += waves_total) {
        const double *a = acc + (size_t)q * (C + 1);
        const double mp = live ? a[lane] / S : 0.0;
        const int vt = live ? votes[(size_t)q * C + lane] : 0;
        const double ent = mc_wave_sum(mp > 0.0 ? -(mp * log(mp)) : 0.0);
        const double mmax = mc_wave_max(live ? mp : -INFINITY);
        const int best = __ffsll((unsigned long long)__ballot(live && mp == mmax)) - 1;
        const int vmax = mc_wave_max(vt);
        if (mean_prob && live) mean_prob[(size_t)q * ld_mp + lane] = (float)mp;
        if (lane == 0) {
            const double eent = a[C] / S;
            const double mi = ent - eent;
            if (pred) pred[q] = best;
            if (confidence) confidence[q] = (float)mmax;
            if (entropy) entropy[q] = (float)ent;
            if (expected_entropy) expected_entropy[q] = (float)eent;
            if (mutual_information) mutual_information[q] = (float)(mi > 0.0 ? mi : 0.0);
            if (variation_ratio) variation_ratio[q] = (float)(1.0 - (double)vmax / S);
        }
    }
}

static int mc_blocks(int n) {
    int blocks = ceil_div(n, MC_ROWS_PER_BLOCK);
    if (blocks > MC_MAX_BLOCKS) blocks = MC_MAX_BLOCKS;
    return blocks < 1 ? 1 : blocks;
}

#define MC_REFUSE(NAME, WHY)                                                      \
    do {                                                                          \
        char msg[160];                                                            \
        snprintf(msg, sizeof msg, "%s: %s", NAME, WHY);                           \
        return gcnhip_fail(msg);                                                  \
    } while (0)

extern "C" {

int gcnhip_mc_accumulate_rows(gcnhip_ctx *c, const float *logp, int ld, int n_table, const int32_t *d_rows, int n, int num_classes, int first,
                              double *acc_f64, int32_t *acc_votes) {
    const char *name = "gcnhip_mc_accumulate_rows";
    if (!c || !acc_f64 || !acc_votes || n_table < 0 || n < 0) MC_REFUSE(name, "invalid argument");
    if (!logp && n_table > 0) MC_REFUSE(name, "invalid argument");
    if (num_classes < 1 || num_classes > WAVE) MC_REFUSE(name, "1 <= num_classes <= 64 (lane j holds class j)");
    if (ld < num_classes) MC_REFUSE(name, "a row stride is below num_classes");
    if (!d_rows && n > n_table) MC_REFUSE(name, "without a row list n is at most n_table");
    if (n == 0) return 0;
    mc_accumulate_kernel<<<mc_blocks(n), 256, 0, c->stream>>>(logp, ld, n_table, d_rows, n, num_classes, first, acc_f64, acc_votes);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_mc_finalize_rows(gcnhip_ctx *c, const double *acc_f64, const int32_t *acc_votes, int n, int num_classes, int samples, float *mean_prob,
                            int ld_mp, int32_t *pred, float *confidence, float *entropy, float *expected_entropy, float *mutual_information,
                            float *variation_ratio) {
    const char *name = "gcnhip_mc_finalize_rows";
    if (!c || !acc_f64 || !acc_votes || n < 0) MC_REFUSE(name, "invalid argument");
    if (num_classes < 1 || num_classes > WAVE) MC_REFUSE(name, "1 <= num_classes <= 64 (lane j holds class j)");
    if (samples < 1) MC_REFUSE(name, "samples must be >= 1");
    if (mean_prob && ld_mp < num_classes) MC_REFUSE(name, "a row stride is below num_classes");
    if (n == 0) return 0;
    mc_finalize_kernel<<<mc_blocks(n), 256, 0, c->stream>>>(acc_f64, acc_votes, n, num_classes, samples, mean_prob, ld_mp, pred, confidence, entropy,
                                                            expected_entropy, mutual_information, variation_ratio);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
